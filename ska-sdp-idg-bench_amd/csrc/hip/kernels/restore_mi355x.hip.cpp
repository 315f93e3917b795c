// restore_mi355x.hip.cpp -- the restore step on the device:
// restored = residual + model convolved with the clean beam's taps, bit for
// bit the host entry idg_restore (common/restore.hpp holds the arithmetic of
// both).  The model of a CLEAN run is sparse, so no pixel pays for the zeros
// around it: ordered compaction per tile.
//
// The plane is cut into tiles of kTileCols columns x kTileRows rows, one
// workgroup each.  A lane owns one column of the tile and a wave
// kRowsPerThread consecutive rows of it, so every output pixel has one owning
// thread, which keeps the pixel's accumulator in a register.
//   scan     the tile's haloed model window, (rows + 2R) x (cols + 2R)
//            clipped to the image, in row-major rounds of kChunk pixels: a
//            thread takes four consecutive pixels (one float4 when G % 4 == 0
//            and the model is 16-byte aligned, four dwords otherwise)
//   compact  the non-zero pixels of the round go to an LDS list of {value,
//            y, x} in row-major order: a ballot per pixel slot and a prefix
//            popcount give the place inside the wave, four counts in LDS the
//            place of the wave
//   add      every thread walks the list in order; for an entry within +-R of
//            its column and of one of its rows, one fmaf per such row.  The
//            entry is a broadcast read, the taps sit in LDS (loaded when the
//            first list is not empty), and consecutive lanes read consecutive
//            tap dwords.  A wave skips an entry none of its rows can reach.
// A dense window only takes more rounds: the list never outgrows kChunk
// entries, and a pixel's sources still arrive in row-major order.  A tile
// whose every list is empty writes residual + 0.0f and has read no tap.
// No atomics, no scratch, no cross-workgroup wait.  Per buffer:
//   model     read only: every workgroup reads its window, halo included
//   taps      read only
//   residual  a thread reads the pixels it owns, before it writes them
//   restored  a thread writes the pixels it owns (so restored may be
//             residual)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common/clean.hpp"
#include "common/restore.hpp"
#include "hip/util.hpp"

namespace idg_mi355x {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTileCols = 64;  // a lane per column
constexpr int kRowsPerThread = 8;
constexpr int kTileRows = kWaves * kRowsPerThread;
constexpr int kChunk = 4 * kBlock;  // window pixels, so list entries, a round
constexpr int kMaxTaps =
    (2 * restore::kMaxRadius + 1) * (2 * restore::kMaxRadius + 1);

using u64 = unsigned long long;

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_restore_mi355x(restore::Params p, const float *__restrict__ model,
                          const float *residual,
                          const float *__restrict__ taps, float *restored) {
  __shared__ float lds_taps[kMaxTaps];
  __shared__ uint2 lds_list[kChunk];  // {value's bits, y << 16 | x}
  __shared__ int lds_count[2][kWaves];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = p.grid_size, R = p.radius, side = 2 * R + 1;
  const int tx0 = blockIdx.x * kTileCols, ty0 = blockIdx.y * kTileRows;
  const int x = tx0 + lane, row_lo = ty0 + wave * kRowsPerThread;

  // the pixels this thread owns: their residual now, their sum below
  float res[kRowsPerThread], acc[kRowsPerThread];
#pragma unroll
  for (int k = 0; k < kRowsPerThread; ++k) {
    const int y = row_lo + k;
    acc[k] = 0.0f;
    res[k] = 0.0f;
    if (residual != nullptr && x < G && y < G)
      res[k] = residual[static_cast<size_t>(y) * G + x];
  }

  // the window, rows [wy0, wy1) and columns [wx0, wx1), read in groups of
  // four columns from xa
  const int wy0 = ty0 - R > 0 ? ty0 - R : 0;
  const int wy1 = ty0 + kTileRows + R < G ? ty0 + kTileRows + R : G;
  const int wx0 = tx0 - R > 0 ? tx0 - R : 0;
  const int wx1 = tx0 + kTileCols + R < G ? tx0 + kTileCols + R : G;
  const int xa = wx0 & ~3;
  const int quads = (wx1 - xa + 3) >> 2;
  const int groups = quads * (wy1 - wy0);
  const u64 below = (1ull << lane) - 1;

  bool have_taps = false;
  int round = 0;
  for (int g0 = 0; g0 < groups; g0 += kBlock, ++round) {
    const int g = g0 + tid;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int gy = 0, gx = 0;
    if (g < groups) {
      const int row = g / quads;
      gy = wy0 + row;
      gx = xa + 4 * (g - row * quads);
      const float *src = model + static_cast<size_t>(gy) * G + gx;
      if constexpr (kVec) {
        // G % 4 == 0 and gx % 4 == 0: the four are inside the row
        const float4 q = *reinterpret_cast<const float4 *>(src);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (gx + k < wx0 || gx + k >= wx1) v[k] = 0.0f;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (gx + k >= wx0 && gx + k < wx1) v[k] = src[k];
      }
    }
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u64 b = __ballot(restore::taken(v[k]));
      before += __popcll(b & below);
      total += __popcll(b);
    }
    // (the counts of round r + 1 go to the other pair: a wave that found
    // round r empty may be there while another still reads round r's)
    if (lane == 0) lds_count[round & 1][wave] = total;
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = lds_count[round & 1][w];
      base += w < wave ? c : 0;
      all += c;
    }
    if (all == 0) continue;
    if (!have_taps) {
      for (int i = tid; i < side * side; i += kBlock) lds_taps[i] = taps[i];
      have_taps = true;
    }
    int at = base + before;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (restore::taken(v[k]))
        lds_list[at++] =
            make_uint2(clean::bits_of(v[k]),
                       (static_cast<uint32_t>(gy) << 16) |
                           static_cast<uint32_t>(gx + k));
    __syncthreads();
    for (int e = 0; e < all; ++e) {
      const uint2 entry = lds_list[e];
      const uint32_t yx = __builtin_amdgcn_readfirstlane(entry.y);
      const float m =
          clean::float_of(__builtin_amdgcn_readfirstlane(entry.x));
      // the tap row of this wave's first row, and the thread's tap column
      const int dy0 = row_lo - static_cast<int>(yx >> 16) + R;
      if (dy0 + kRowsPerThread - 1 < 0 || dy0 > 2 * R) continue;
      const int dx = x - static_cast<int>(yx & 0xffffu) + R;
      if (dx >= 0 && dx <= 2 * R) {
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
          const int dy = dy0 + k;
          if (dy >= 0 && dy <= 2 * R)
            acc[k] = restore::accumulate(m, lds_taps[dy * side + dx], acc[k]);
        }
      }
    }
    // (the next round's list is written after its barrier)
  }

  if (x < G) {
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
      const int y = row_lo + k;
      if (y < G)
        restored[static_cast<size_t>(y) * G + x] =
            restore::finish(residual != nullptr, res[k], acc[k]);
    }
  }
}

bool aligned(const void *ptr, size_t to) {
  return reinterpret_cast<uintptr_t>(ptr) % to == 0;
}

}  // namespace

hipError_t launch_restore(const restore::Params &params, const float *d_model,
                          const float *d_residual, const float *d_taps,
                          float *d_restored, hipStream_t stream) {
  restore::Params p = params;
  const bool vec = p.grid_size % 4 == 0 && aligned(d_model, 16);
  const dim3 grid((p.grid_size + kTileCols - 1) / kTileCols,
                  (p.grid_size + kTileRows - 1) / kTileRows);
  void *args[] = {&p, &d_model, &d_residual, &d_taps, &d_restored};
  return hipLaunchKernel(
      vec ? reinterpret_cast<const void *>(&kernel_restore_mi355x<true>)
          : reinterpret_cast<const void *>(&kernel_restore_mi355x<false>),
      grid, dim3(kBlock), args, 0, stream);
}

}  // namespace idg_mi355x
