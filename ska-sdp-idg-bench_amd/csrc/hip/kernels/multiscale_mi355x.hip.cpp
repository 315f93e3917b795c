// multiscale_mi355x.hip.cpp -- multi-scale CLEAN on the device,
// bit for bit the host entries idg_convolve_separable, idg_ms_prepare and
// idg_ms_clean (common/multiscale.hpp holds the arithmetic of both sides).
//
// Convolution.  Two launches, the row pass into tmp and the column pass into
// out; each workgroup stages its tile and the 2 r halo in LDS, so a pixel
// comes from memory once per pass (plus the halo's share), and every thread
// walks the taps in ascending order with one fmaf each.
//   rows     tile kRowTileCols x kRowTileRows, halo left and right
//   columns  tile kColTileCols x kColTileRows, halo above and below
// A workgroup reads `in` (rows) or tmp (columns) and writes only its own tile
// of the other plane: tmp is distinct from both, so out may be in.  No
// scratch, no atomics, no workspace.
//
// Prepare.  Launches of the two passes only, plus one device-to-device copy
// for planes[0]; stream order is the only ordering.
//
// Minor cycle.  The shape of the Hogbom kernels (clean_mi355x.hip.cpp): the
// image is cut into tiles of kTileCols columns x `rows` rows, at most
// kMaxTiles of them, and one workgroup owns its tile in all Ns planes.
//   search   every tile's peak over its pixels and the scales as a partial:
//            the key (ms::key_of: |weight[s] v|, then lower scale, then lower
//            index) and the signed v at that pixel
//   iterate  one launch per iteration.  Every workgroup reduces the previous
//            launch's partials, makes the same stop decision from the same
//            inputs, adds the component's footprint to the model pixels of
//            its tile, subtracts the cross-PSFs from its tile on every plane
//            and leaves the tile's new partial.  A tile the patch does not
//            touch copies its old partial and reads no pixel.
//   finish   one workgroup: state.peak / peak_index / peak_scale from the
//            last partials, the state back to the caller's record
// No atomics, no scratch, no cross-workgroup wait: kernel boundaries order the
// launches, and nothing a workgroup reads in a launch is written by another
// workgroup of that launch.  Per buffer:
//   planes      a workgroup reads and writes the pixels of its own tile only,
//               on every plane (the peak's signed value comes from the
//               partial, never from planes[s][py][px], which its owner
//               rewrites in this launch)
//   cross_psf, taps, mask   read only
//   model       a footprint pixel is read and written by the one workgroup
//               whose tile holds it
//   components  written by workgroup 0, never read
//   partials    double-buffered: launch k reads buffer k & 1 and writes the
//               other (a stopped launch writes neither)
//   state       double-buffered the same way: read by all, the other copy
//               written by workgroup 0; the caller's record is read by the
//               search launch's workgroup 0 and written by finish
// Workspace (util.hpp kWorkspaceMultiscale): the partials and the two states.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common/multiscale.hpp"
#include "hip/util.hpp"

namespace idg_mi355x {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kHalo = ms::kMaxRadius;  // LDS room either side of a tile

using u64 = unsigned long long;

bool aligned(const void *ptr, size_t to) {
  return reinterpret_cast<uintptr_t>(ptr) % to == 0;
}

// ---- the separable convolution ------------------------------------------------
constexpr int kRowTileCols = 256, kRowTileRows = 8;
constexpr int kRowLds = kRowTileCols + 2 * kHalo;
constexpr int kColTileCols = 64, kColTileRows = 64;
constexpr int kColLds = kColTileRows + 2 * kHalo;

// kVec: G % 4 == 0 and the plane is 16-byte aligned, so the tile and its halo
// (widened to a multiple of 4 columns) are staged with float4 loads; a float4
// lies wholly inside a row or wholly outside it.
template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_convolve_rows_mi355x(int G, int r, const float *__restrict__ in,
                                const float *__restrict__ taps,
                                float *__restrict__ tmp) {
  __shared__ __align__(16) float lds[kRowTileRows][kRowLds];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kRowTileCols, y0 = blockIdx.y * kRowTileRows;
  const int reach = kVec ? (r + 3) & ~3 : r;
  const int span = kRowTileCols + 2 * reach;
  if constexpr (kVec) {
    const int quads = span / 4;
    for (int i = tid; i < kRowTileRows * quads; i += kBlock) {
      const int row = i / quads, j = i - row * quads;
      const int y = y0 + row, x = x0 - reach + 4 * j;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (y < G && x >= 0 && x < G)
        v = *reinterpret_cast<const float4 *>(in + static_cast<size_t>(y) * G +
                                              x);
      *reinterpret_cast<float4 *>(&lds[row][kHalo - reach + 4 * j]) = v;
    }
  } else {
    for (int i = tid; i < kRowTileRows * span; i += kBlock) {
      const int row = i / span, j = i - row * span;
      const int y = y0 + row, x = x0 - reach + j;
      lds[row][kHalo - reach + j] =
          y < G && x >= 0 && x < G ? in[static_cast<size_t>(y) * G + x] : 0.0f;
    }
  }
  __syncthreads();
  const int x = x0 + tid;
  if (x >= G) return;
  for (int row = 0; row < kRowTileRows && y0 + row < G; ++row) {
    float acc = 0.0f;
    for (int k = -r; k <= r; ++k)
      if (x + k >= 0 && x + k < G)
        acc = ms::tap(lds[row][kHalo + tid + k], taps[k + r], acc);
    tmp[static_cast<size_t>(y0 + row) * G + x] = acc;
  }
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_convolve_columns_mi355x(int G, int r, const float *__restrict__ tmp,
                                   const float *__restrict__ taps,
                                   float *__restrict__ out) {
  __shared__ __align__(16) float lds[kColLds][kColTileCols];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kColTileCols, y0 = blockIdx.y * kColTileRows;
  const int span = kColTileRows + 2 * r;
  if constexpr (kVec) {
    constexpr int quads = kColTileCols / 4;
    for (int i = tid; i < span * quads; i += kBlock) {
      const int row = i / quads, j = i - row * quads;
      const int y = y0 - r + row, x = x0 + 4 * j;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (y >= 0 && y < G && x < G)
        v = *reinterpret_cast<const float4 *>(tmp + static_cast<size_t>(y) * G +
                                              x);
      *reinterpret_cast<float4 *>(&lds[kHalo - r + row][4 * j]) = v;
    }
  } else {
    for (int i = tid; i < span * kColTileCols; i += kBlock) {
      const int row = i / kColTileCols, j = i - row * kColTileCols;
      const int y = y0 - r + row, x = x0 + j;
      lds[kHalo - r + row][j] = y >= 0 && y < G && x < G
                                    ? tmp[static_cast<size_t>(y) * G + x]
                                    : 0.0f;
    }
  }
  __syncthreads();
  const int cx = tid & (kColTileCols - 1), x = x0 + cx;
  if (x >= G) return;
  constexpr int kRowsPerThread = kColTileRows / (kBlock / kColTileCols);
  const int first = (tid / kColTileCols) * kRowsPerThread;
  for (int i = first; i < first + kRowsPerThread && y0 + i < G; ++i) {
    const int y = y0 + i;
    float acc = 0.0f;
    for (int k = -r; k <= r; ++k)
      if (y + k >= 0 && y + k < G)
        acc = ms::tap(lds[kHalo + i + k][cx], taps[k + r], acc);
    out[static_cast<size_t>(y) * G + x] = acc;
  }
}

// ---- the minor cycle ----------------------------------------------------------
constexpr int kTileCols = 256;  // a wave's float4 loads cover one tile row
constexpr int kMinTileRows = 8;
constexpr int kMaxTiles = 2048;

struct Tiling {
  int tiles_x, tiles_y, rows, nr_tiles;
};

// The state as the launches hand it on: the caller's record and which of the
// two partial buffers describes the planes as they stand.
struct DevState {
  ms::State s;
  int32_t partials_at;
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

// One pass over tile `tile` on every plane: with kSub, step 8 on its pixels
// inside the patch (the component is of scale s); then the tile's partial.
// kVec: G % 4 == 0 and the planes are aligned, so a lane takes four pixels of
// a row as one float4 (the cross-PSF row is offset by px - Gp / 2 against it:
// dword loads).
template <bool kVec, bool kSub>
__device__ inline void scan_tile(const ms::Params &p, const Tiling &t,
                                 int tile, float c, int s,
                                 const clean::Patch &pt, float *planes,
                                 const float *__restrict__ cross_psf,
                                 const uint8_t *__restrict__ mask,
                                 u64 *keys_out, float *vals_out, u64 *lds) {
  constexpr int kN = kVec ? 4 : 1;
  const int tid = threadIdx.x;
  const int G = p.base.grid_size, Gp = p.base.psf_size;
  const size_t cells = static_cast<size_t>(G) * G;
  const size_t pcells = static_cast<size_t>(Gp) * Gp;
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows;
  const int row1 = row0 + t.rows < G ? row0 + t.rows : G;
  const int col = tx * kTileCols + (kVec ? (tid & 63) * 4 : tid);
  const int first = row0 + (kVec ? tid >> 6 : 0);
  u64 best = 0;
  float best_v = 0.0f;
  if (col < G) {
    for (int q = 0; q < p.nr_scales; ++q) {
      float *plane = planes + q * cells;
      const float *cross =
          kSub ? cross_psf + ms::cross_at(p.nr_scales, s, q) * pcells : nullptr;
      for (int y = first; y < row1; y += kVec ? kWaves : 1) {
        const size_t at = static_cast<size_t>(y) * G + col;
        float r[kN];
        uint32_t m = 0x01010101u;
        if constexpr (kVec) {
          const float4 v = *reinterpret_cast<const float4 *>(plane + at);
          r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
          if (mask != nullptr)
            m = *reinterpret_cast<const uint32_t *>(mask + at);
        } else {
          r[0] = plane[at];
          if (mask != nullptr) m = mask[at];
        }
        if (kSub && y >= pt.y0 && y < pt.y1) {
          const size_t prow = static_cast<size_t>(y - pt.oy) * Gp;
          bool any = false;
#pragma unroll
          for (int k = 0; k < kN; ++k) {
            const int x = col + k;
            if (x >= pt.x0 && x < pt.x1) {
              r[k] = clean::subtract(c, cross[prow + (x - pt.ox)], r[k]);
              any = true;
            }
          }
          // (pixels of the float4 outside the patch go back as the bits read)
          if (any) {
            if constexpr (kVec)
              *reinterpret_cast<float4 *>(plane + at) =
                  make_float4(r[0], r[1], r[2], r[3]);
            else
              plane[at] = r[0];
          }
        }
#pragma unroll
        for (int k = 0; k < kN; ++k) {
          const u64 key =
              ms::key_of(ms::weighted(p, q, r[k]), q,
                         static_cast<uint32_t>(at + k),
                         ((m >> (8 * k)) & 0xffu) != 0);
          if (key > best) {
            best = key;
            best_v = r[k];
          }
        }
      }
    }
  }
  const u64 top = block_max(best, lds);
  // a pixel's key on a plane is its own: one thread holds the tile's
  if (top != 0 ? best == top : tid == 0) {
    keys_out[tile] = top;
    vals_out[tile] = top != 0 ? best_v : 0.0f;
  }
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_ms_search_mi355x(ms::Params p, Tiling t, float *planes,
                            const uint8_t *__restrict__ mask,
                            const ms::State *caller_state, DevState *st_out,
                            u64 *keys_out, float *vals_out) {
  __shared__ u64 lds[kWaves];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    DevState st;
    st.s = *caller_state;
    st.partials_at = 0;
    *st_out = st;
  }
  const clean::Patch none = {0, 0, 0, 0, 0, 0};
  scan_tile<kVec, false>(p, t, blockIdx.x, 0.0f, 0, none, planes, nullptr,
                         mask, keys_out, vals_out, lds);
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_ms_iterate_mi355x(ms::Params p, Tiling t, float *planes,
                             const float *__restrict__ cross_psf,
                             const float *__restrict__ taps,
                             const uint8_t *__restrict__ mask, float *model,
                             ms::Component *components,
                             const DevState *__restrict__ st_in,
                             DevState *st_out,
                             const u64 *__restrict__ keys_in,
                             const float *__restrict__ vals_in, u64 *keys_out,
                             float *vals_out, int out_index) {
  __shared__ u64 lds_peak[kWaves], lds_tile[kWaves];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const bool scribe = tile == 0 && tid == 0;
  DevState st = *st_in;
  if (st.s.s.reason != clean::kRunning || !clean::state_ok(st.s.s, p.base)) {
    if (scribe) *st_out = st;
    return;
  }
  u64 key = 0;
  for (int i = tid; i < t.nr_tiles; i += kBlock) {
    const u64 k = keys_in[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds_peak);
  const int G = p.base.grid_size;
  int py = 0, px = 0, s = 0;
  float v = 0.0f;
  if (key != 0) {
    const uint32_t index = ms::index_of(key);
    s = ms::scale_of(key);
    py = static_cast<int>(index / static_cast<uint32_t>(G));
    px = static_cast<int>(index - static_cast<uint32_t>(py) * G);
    v = vals_in[(py / t.rows) * t.tiles_x + px / kTileCols];
  }
  float c = 0.0f;
  if (!ms::step(&st.s, p, key, v, &c)) {
    if (scribe) *st_out = st;
    return;
  }
  if (scribe) {
    ms::Component rec;
    rec.y = py;
    rec.x = px;
    rec.scale = s;
    rec.value = c;
    components[st.s.s.n_components - 1] = rec;
    st.partials_at = out_index;
    *st_out = st;
  }
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows, col0 = tx * kTileCols;
  const int row1 = row0 + t.rows < G ? row0 + t.rows : G;
  const int col1 = col0 + kTileCols < G ? col0 + kTileCols : G;

  // step 7: the footprint's pixels inside this tile
  {
    const int r = p.radius[s];
    const float *h = taps + ms::taps_at(p, s);
    const int ya = py - r > row0 ? py - r : row0;
    const int yb = py + r + 1 < row1 ? py + r + 1 : row1;
    const int xa = px - r > col0 ? px - r : col0;
    const int xb = px + r + 1 < col1 ? px + r + 1 : col1;
    if (ya < yb && xa < xb) {
      const int w = xb - xa, n = w * (yb - ya);
      for (int i = tid; i < n; i += kBlock) {
        const int y = ya + i / w, x = xa + i % w;
        float *m = model + static_cast<size_t>(y) * G + x;
        *m = ms::model_add(c, h[y - py + r], h[x - px + r], *m);
      }
    }
  }

  const clean::Patch pt = clean::patch_of(p.base, py, px);
  const bool touched = row0 < pt.y1 && row0 + t.rows > pt.y0 &&
                       col0 < pt.x1 && col0 + kTileCols > pt.x0;
  if (!touched) {
    if (tid == 0) {
      keys_out[tile] = keys_in[tile];
      vals_out[tile] = vals_in[tile];
    }
    return;
  }
  scan_tile<kVec, true>(p, t, tile, c, s, pt, planes, cross_psf, mask,
                        keys_out, vals_out, lds_tile);
}

__global__ void __launch_bounds__(kBlock)
    kernel_ms_finish_mi355x(int nr_tiles, const DevState *__restrict__ st_in,
                            const u64 *__restrict__ keys,
                            ms::State *caller_state) {
  __shared__ u64 lds[kWaves];
  const u64 *from = keys + static_cast<size_t>(st_in->partials_at) * nr_tiles;
  u64 key = 0;
  for (int i = threadIdx.x; i < nr_tiles; i += kBlock) {
    const u64 k = from[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds);
  if (threadIdx.x == 0) {
    ms::State s = st_in->s;
    ms::set_peak(&s, key);
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
  return t;
}

}  // namespace

hipError_t launch_convolve_separable(int grid_size, int radius,
                                     const float *d_in, const float *d_taps,
                                     float *d_tmp, float *d_out,
                                     hipStream_t stream) {
  int G = grid_size, r = radius;
  const bool vec = G % 4 == 0 && aligned(d_in, 16) && aligned(d_tmp, 16);
  {
    void *args[] = {&G, &r, &d_in, &d_taps, &d_tmp};
    const dim3 grid((G + kRowTileCols - 1) / kRowTileCols,
                    (G + kRowTileRows - 1) / kRowTileRows);
    hipError_t err = hipLaunchKernel(
        vec ? reinterpret_cast<const void *>(&kernel_convolve_rows_mi355x<true>)
            : reinterpret_cast<const void *>(
                  &kernel_convolve_rows_mi355x<false>),
        grid, dim3(kBlock), args, 0, stream);
    if (err != hipSuccess) return err;
  }
  const float *tmp_in = d_tmp;
  void *args[] = {&G, &r, &tmp_in, &d_taps, &d_out};
  const dim3 grid((G + kColTileCols - 1) / kColTileCols,
                  (G + kColTileRows - 1) / kColTileRows);
  return hipLaunchKernel(
      vec ? reinterpret_cast<const void *>(&kernel_convolve_columns_mi355x<true>)
          : reinterpret_cast<const void *>(
                &kernel_convolve_columns_mi355x<false>),
      grid, dim3(kBlock), args, 0, stream);
}

hipError_t launch_ms_prepare(const ms::Params &p, const float *d_residual,
                             const float *d_psf, const float *d_taps,
                             float *d_planes, float *d_cross_psf, float *d_tmp,
                             hipStream_t stream) {
  const int G = p.base.grid_size, Gp = p.base.psf_size, Ns = p.nr_scales;
  const size_t cells = static_cast<size_t>(G) * G;
  const size_t pcells = static_cast<size_t>(Gp) * Gp;
  hipError_t err = hipSuccess;
  if (d_planes != d_residual) {
    err = hipMemcpyAsync(d_planes, d_residual, cells * sizeof(float),
                         hipMemcpyDeviceToDevice, stream);
    if (err != hipSuccess) return err;
  }
  for (int s = 1; s < Ns; ++s) {
    err = launch_convolve_separable(G, p.radius[s], d_residual,
                                    d_taps + ms::taps_at(p, s), d_tmp,
                                    d_planes + s * cells, stream);
    if (err != hipSuccess) return err;
  }
  // the order of host::ms_prepare: cross(s, s)'s patch holds the first
  // convolution until the row's other patches are made from it
  for (int s = 0; s < Ns; ++s) {
    const float *hs = d_taps + ms::taps_at(p, s);
    float *first = d_cross_psf + ms::cross_at(Ns, s, s) * pcells;
    err = launch_convolve_separable(Gp, p.radius[s], d_psf, hs, d_tmp, first,
                                    stream);
    if (err != hipSuccess) return err;
    for (int q = s + 1; q < Ns; ++q) {
      err = launch_convolve_separable(
          Gp, p.radius[q], first, d_taps + ms::taps_at(p, q), d_tmp,
          d_cross_psf + ms::cross_at(Ns, s, q) * pcells, stream);
      if (err != hipSuccess) return err;
    }
    err = launch_convolve_separable(Gp, p.radius[s], first, hs, d_tmp, first,
                                    stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

hipError_t launch_ms_clean(const ms::Params &params, float *d_planes,
                           const float *d_cross_psf, const float *d_taps,
                           const uint8_t *d_mask, float *d_model,
                           void *d_components, void *d_state,
                           hipStream_t stream) {
  ms::Params p = params;
  Tiling t = tiling_of(p.base.grid_size);
  const bool vec = p.base.grid_size % 4 == 0 && aligned(d_planes, 16) &&
                   aligned(d_mask, 4);
  const size_t n = static_cast<size_t>(t.nr_tiles);
  WorkspaceLease lease;
  hipError_t err = lease.acquire(
      stream, kWorkspaceMultiscale,
      2 * n * sizeof(u64) + 2 * n * sizeof(float) + 2 * sizeof(DevState));
  if (err != hipSuccess) return err;
  u64 *keys = static_cast<u64 *>(lease.ptr);
  DevState *states = reinterpret_cast<DevState *>(keys + 2 * n);
  float *vals = reinterpret_cast<float *>(states + 2);

  {
    u64 *keys_out = keys;
    float *vals_out = vals;
    DevState *st_out = states;
    void *args[] = {&p,       &t,      &d_planes, &d_mask,
                    &d_state, &st_out, &keys_out, &vals_out};
    err = hipLaunchKernel(
        vec ? reinterpret_cast<const void *>(&kernel_ms_search_mi355x<true>)
            : reinterpret_cast<const void *>(&kernel_ms_search_mi355x<false>),
        dim3(t.nr_tiles), dim3(kBlock), args, 0, stream);
    if (err != hipSuccess) return err;
  }
  const void *iterate =
      vec ? reinterpret_cast<const void *>(&kernel_ms_iterate_mi355x<true>)
          : reinterpret_cast<const void *>(&kernel_ms_iterate_mi355x<false>);
  for (int k = 0; k < p.base.nr_iterations; ++k) {
    const int in = k & 1;
    int out = in ^ 1;
    const DevState *st_in = states + in;
    DevState *st_out = states + out;
    const u64 *keys_in = keys + in * n;
    u64 *keys_out = keys + out * n;
    const float *vals_in = vals + in * n;
    float *vals_out = vals + out * n;
    void *args[] = {&p,       &t,        &d_planes, &d_cross_psf,  &d_taps,
                    &d_mask,  &d_model,  &d_components, &st_in,    &st_out,
                    &keys_in, &vals_in,  &keys_out, &vals_out,     &out};
    err = hipLaunchKernel(iterate, dim3(t.nr_tiles), dim3(kBlock), args, 0,
                          stream);
    if (err != hipSuccess) return err;
  }
  const DevState *st_in = states + (p.base.nr_iterations & 1);
  const u64 *keys_in = keys;
  void *args[] = {&t.nr_tiles, &st_in, &keys_in, &d_state};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_ms_finish_mi355x), dim3(1),
      dim3(kBlock), args, 0, stream);
}

}  // namespace idg_mi355x
