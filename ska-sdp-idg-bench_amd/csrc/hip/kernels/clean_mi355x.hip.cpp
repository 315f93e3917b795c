// clean_mi355x.hip.cpp -- the Hogbom minor cycle on the device,
// bit for bit the host entry idg_clean (common/clean.hpp holds the arithmetic
// of both).  The plane is cut into tiles of kTileCols columns x `rows` rows,
// one workgroup each, at most kMaxTiles of them.
//   search   every tile's peak as a partial: its key (clean::key_of, ordered
//            by |s| then lower index) and the signed value at that pixel
//   iterate  one launch per iteration.  Every workgroup reduces the previous
//            launch's partials, makes the same stop decision from the same
//            inputs, subtracts component k from its tile and leaves the
//            tile's new partial: the search for component k + 1 rides on the
//            pass that subtracts component k.  A tile the patch does not
//            touch copies its old partial and reads no pixel.
//   finish   one workgroup: state.peak / peak_index from the last partials,
//            the state back to the caller's record
// No atomics, no scratch, no cross-workgroup wait: kernel boundaries order the
// launches, and nothing a workgroup reads in a launch is written by another
// workgroup of that launch.  Per buffer:
//   residual    a workgroup reads and writes the pixels of its own tile only
//               (the peak's signed value comes from the partial, never from
//               residual[py][px], which its owner rewrites in this launch)
//   psf, mask   read only
//   model       read and written by the one workgroup whose tile holds
//               (py, px)
//   components  written by workgroup 0, never read
//   partials    double-buffered: launch k reads buffer k & 1 and writes the
//               other (a stopped launch writes neither)
//   state       double-buffered the same way: read by all, the other copy
//               written by workgroup 0; the caller's record is read by the
//               search launch's workgroup 0 and written by finish
// Workspace (util.hpp kWorkspaceClean): the partials and the two states.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "common/clean.hpp"
#include "hip/util.hpp"

namespace idg_mi355x {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTileCols = 256;   // a wave's float4 loads cover one tile row
constexpr int kMinTileRows = 8;
constexpr int kMaxTiles = 2048;

using u64 = unsigned long long;

struct Tiling {
  int tiles_x, tiles_y, rows, nr_tiles;
  int rescan;  // every tile rescans, touched or not (IDG_CLEAN_RESCAN=1)
};

// The state as the launches hand it on: the caller's record and which of the
// two partial buffers describes the residual as it stands.
struct DevState {
  clean::State s;
  int32_t partials_at;
  int32_t pad;
};

// Max of v over the workgroup, in every thread: shuffles per wave, LDS across
// the waves.  Max is exact and associative: any tree, the same answer.
__device__ inline u64 block_max(u64 v, u64 *lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = __shfl_xor(v, d, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 m = lds[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) m = lds[w] > m ? lds[w] : m;
  return m;
}

// One pass over tile `tile`: with kSub, step 7 on its pixels inside the patch;
// then the tile's partial.  kVec: G % 4 == 0 and the planes are aligned, so a
// lane takes four pixels of a row as one float4 (the PSF row is offset by
// px - Gp / 2 against it: dword loads).
template <bool kVec, bool kSub>
__device__ inline void scan_tile(const clean::Params &p, const Tiling &t,
                                 int tile, float c, const clean::Patch &pt,
                                 float *residual,
                                 const float *__restrict__ psf,
                                 const uint8_t *__restrict__ mask,
                                 u64 *keys_out, float *vals_out, u64 *lds) {
  constexpr int kN = kVec ? 4 : 1;
  const int tid = threadIdx.x;
  const int G = p.grid_size, Gp = p.psf_size;
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows;
  const int row1 = row0 + t.rows < G ? row0 + t.rows : G;
  const int col = tx * kTileCols + (kVec ? (tid & 63) * 4 : tid);
  const int first = row0 + (kVec ? tid >> 6 : 0);
  u64 best = 0;
  float best_v = 0.0f;
  if (col < G) {
    for (int y = first; y < row1; y += kVec ? kWaves : 1) {
      const size_t at = static_cast<size_t>(y) * G + col;
      float r[kN];
      uint32_t m = 0x01010101u;
      if constexpr (kVec) {
        const float4 q = *reinterpret_cast<const float4 *>(residual + at);
        r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
        if (mask != nullptr)
          m = *reinterpret_cast<const uint32_t *>(mask + at);
      } else {
        r[0] = residual[at];
        if (mask != nullptr) m = mask[at];
      }
      if (kSub && y >= pt.y0 && y < pt.y1) {
        const size_t prow = static_cast<size_t>(y - pt.oy) * Gp;
        bool any = false;
#pragma unroll
        for (int k = 0; k < kN; ++k) {
          const int x = col + k;
          if (x >= pt.x0 && x < pt.x1) {
            r[k] = clean::subtract(c, psf[prow + (x - pt.ox)], r[k]);
            any = true;
          }
        }
        // (pixels of the float4 outside the patch go back as the bits read)
        if (any) {
          if constexpr (kVec)
            *reinterpret_cast<float4 *>(residual + at) =
                make_float4(r[0], r[1], r[2], r[3]);
          else
            residual[at] = r[0];
        }
      }
#pragma unroll
      for (int k = 0; k < kN; ++k) {
        const u64 key = clean::key_of(r[k], static_cast<uint32_t>(at + k),
                                      ((m >> (8 * k)) & 0xffu) != 0);
        if (key > best) {
          best = key;
          best_v = r[k];
        }
      }
    }
  }
  const u64 top = block_max(best, lds);
  // a pixel's key is its own: one thread holds the tile's
  if (top != 0 ? best == top : tid == 0) {
    keys_out[tile] = top;
    vals_out[tile] = top != 0 ? best_v : 0.0f;
  }
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_clean_search_mi355x(clean::Params p, Tiling t, float *residual,
                               const uint8_t *__restrict__ mask,
                               const clean::State *caller_state,
                               DevState *st_out, u64 *keys_out,
                               float *vals_out) {
  __shared__ u64 lds[kWaves];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    DevState st;
    st.s = *caller_state;
    st.partials_at = 0;
    st.pad = 0;
    *st_out = st;
  }
  const clean::Patch none = {0, 0, 0, 0, 0, 0};
  scan_tile<kVec, false>(p, t, blockIdx.x, 0.0f, none, residual, nullptr, mask,
                         keys_out, vals_out, lds);
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_clean_iterate_mi355x(clean::Params p, Tiling t, float *residual,
                                const float *__restrict__ psf,
                                const uint8_t *__restrict__ mask, float *model,
                                clean::Component *components,
                                const DevState *__restrict__ st_in,
                                DevState *st_out,
                                const u64 *__restrict__ keys_in,
                                const float *__restrict__ vals_in,
                                u64 *keys_out, float *vals_out,
                                int out_index) {
  __shared__ u64 lds_peak[kWaves], lds_tile[kWaves];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const bool scribe = tile == 0 && tid == 0;
  DevState st = *st_in;
  if (st.s.reason != clean::kRunning || !clean::state_ok(st.s, p)) {
    if (scribe) *st_out = st;
    return;
  }
  u64 key = 0;
  for (int i = tid; i < t.nr_tiles; i += kBlock) {
    const u64 k = keys_in[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds_peak);
  const int G = p.grid_size;
  int py = 0, px = 0, owner = -1;
  uint32_t index = 0;
  float v = 0.0f;
  if (key != 0) {
    index = clean::index_of(key);
    py = static_cast<int>(index / static_cast<uint32_t>(G));
    px = static_cast<int>(index - static_cast<uint32_t>(py) * G);
    owner = (py / t.rows) * t.tiles_x + px / kTileCols;
    v = vals_in[owner];
  }
  float c = 0.0f;
  if (!clean::step(&st.s, p, key, v, &c)) {
    if (scribe) *st_out = st;
    return;
  }
  if (scribe) {
    clean::Component rec;
    rec.y = py;
    rec.x = px;
    rec.value = c;
    components[st.s.n_components - 1] = rec;
    st.partials_at = out_index;
    *st_out = st;
  }
  if (tile == owner && tid == 0) model[index] = model[index] + c;

  const clean::Patch pt = clean::patch_of(p, py, px);
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows, col0 = tx * kTileCols;
  const bool touched = row0 < pt.y1 && row0 + t.rows > pt.y0 &&
                       col0 < pt.x1 && col0 + kTileCols > pt.x0;
  if (!touched && !t.rescan) {
    if (tid == 0) {
      keys_out[tile] = keys_in[tile];
      vals_out[tile] = vals_in[tile];
    }
    return;
  }
  scan_tile<kVec, true>(p, t, tile, c, pt, residual, psf, mask, keys_out,
                        vals_out, lds_tile);
}

__global__ void __launch_bounds__(kBlock)
    kernel_clean_finish_mi355x(int nr_tiles,
                               const DevState *__restrict__ st_in,
                               const u64 *__restrict__ keys,
                               clean::State *caller_state) {
  __shared__ u64 lds[kWaves];
  const u64 *from = keys + static_cast<size_t>(st_in->partials_at) * nr_tiles;
  u64 key = 0;
  for (int i = threadIdx.x; i < nr_tiles; i += kBlock) {
    const u64 k = from[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds);
  if (threadIdx.x == 0) {
    clean::State s = st_in->s;
    clean::set_peak(&s, key);
    *caller_state = s;
  }
}

Tiling tiling_of(int grid_size) {
  Tiling t;
  t.tiles_x = (grid_size + kTileCols - 1) / kTileCols;
  const int max_y = kMaxTiles / t.tiles_x;
  t.rows = (grid_size + max_y - 1) / max_y;
  if (t.rows < kMinTileRows) t.rows = kMinTileRows;
  t.tiles_y = (grid_size + t.rows - 1) / t.rows;
  t.nr_tiles = t.tiles_x * t.tiles_y;
  // IDG_CLEAN_RESCAN=1: no tile carries its partial forward (the comparison
  // of tools/debug/clean_rate.py)
  const char *knob = std::getenv("IDG_CLEAN_RESCAN");
  t.rescan = knob && knob[0] == '1' ? 1 : 0;
  return t;
}

bool aligned(const void *ptr, size_t to) {
  return reinterpret_cast<uintptr_t>(ptr) % to == 0;
}

}  // namespace

hipError_t launch_clean(const clean::Params &params, float *d_residual,
                        const float *d_psf, const uint8_t *d_mask,
                        float *d_model, void *d_components, void *d_state,
                        hipStream_t stream) {
  clean::Params p = params;
  Tiling t = tiling_of(p.grid_size);
  const bool vec = p.grid_size % 4 == 0 && aligned(d_residual, 16) &&
                   aligned(d_mask, 4);
  const size_t n = static_cast<size_t>(t.nr_tiles);
  WorkspaceLease lease;
  hipError_t err = lease.acquire(
      stream, kWorkspaceClean,
      2 * n * sizeof(u64) + 2 * n * sizeof(float) + 2 * sizeof(DevState));
  if (err != hipSuccess) return err;
  u64 *keys = static_cast<u64 *>(lease.ptr);
  DevState *states = reinterpret_cast<DevState *>(keys + 2 * n);
  float *vals = reinterpret_cast<float *>(states + 2);

  {
    u64 *keys_out = keys;
    float *vals_out = vals;
    DevState *st_out = states;
    void *args[] = {&p,       &t,      &d_residual, &d_mask,
                    &d_state, &st_out, &keys_out,   &vals_out};
    err = hipLaunchKernel(
        vec ? reinterpret_cast<const void *>(&kernel_clean_search_mi355x<true>)
            : reinterpret_cast<const void *>(
                  &kernel_clean_search_mi355x<false>),
        dim3(t.nr_tiles), dim3(kBlock), args, 0, stream);
    if (err != hipSuccess) return err;
  }
  const void *iterate =
      vec ? reinterpret_cast<const void *>(&kernel_clean_iterate_mi355x<true>)
          : reinterpret_cast<const void *>(
                &kernel_clean_iterate_mi355x<false>);
  for (int k = 0; k < p.nr_iterations; ++k) {
    const int in = k & 1;
    int out = in ^ 1;
    const DevState *st_in = states + in;
    DevState *st_out = states + out;
    const u64 *keys_in = keys + in * n;
    u64 *keys_out = keys + out * n;
    const float *vals_in = vals + in * n;
    float *vals_out = vals + out * n;
    void *args[] = {&p,        &t,        &d_residual,   &d_psf,   &d_mask,
                    &d_model,  &d_components, &st_in,    &st_out,  &keys_in,
                    &vals_in,  &keys_out, &vals_out,     &out};
    err = hipLaunchKernel(iterate, dim3(t.nr_tiles), dim3(kBlock), args, 0,
                          stream);
    if (err != hipSuccess) return err;
  }
  const DevState *st_in = states + (p.nr_iterations & 1);
  const u64 *keys_in = keys;
  void *args[] = {&t.nr_tiles, &st_in, &keys_in, &d_state};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_clean_finish_mi355x), dim3(1),
      dim3(kBlock), args, 0, stream);
}

}  // namespace idg_mi355x
