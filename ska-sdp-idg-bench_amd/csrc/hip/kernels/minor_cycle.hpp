// minor_cycle.hpp -- the CLEAN minor cycle on the device, once for the Hogbom
// cycle (clean_mi355x.hip.cpp) and the multi-scale cycle
// (multiscale_mi355x.hip.cpp), bit for bit the host's
// (host/minor_cycle.hpp).  A cycle is a policy: clean::Cycle or ms::Cycle
// (common/clean.hpp, common/multiscale.hpp) plus the one step that differs on
// the device, add_to_model.  The image is cut into tiles of kTileCols columns
// x `rows` rows, at most kMaxTiles of them, and one workgroup owns its tile
// on every plane (Hogbom: the residual is the one plane, the PSF the one
// patch).
//   search   every tile's peak over its pixels and the planes as a partial:
//            its key (Cycle::key_of: ordered by magnitude, then lower plane,
//            then lower index) and the signed value at that pixel
//   iterate  one launch per iteration.  Every workgroup reduces the previous
//            launch's partials, makes the same stop decision from the same
//            inputs, adds the component to the model pixels of its tile,
//            subtracts component k from its tile on every plane and leaves
//            the tile's new partial: the search for component k + 1 rides on
//            the pass that subtracts component k.  A tile the patch does not
//            touch copies its old partial and reads no pixel.
//   finish   one workgroup: the state's peak from the last partials, the
//            state back to the caller's record
// No atomics, no scratch, no cross-workgroup wait: kernel boundaries order the
// launches, and nothing a workgroup reads in a launch is written by another
// workgroup of that launch.  Per buffer:
//   planes      a workgroup reads and writes the pixels of its own tile only,
//               on every plane (the peak's signed value comes from the
//               partial, never from planes[s][py][px], which its owner
//               rewrites in this launch)
//   psf, taps, mask   read only
//   model       a pixel is read and written by the one workgroup whose tile
//               holds it
//   components  written by workgroup 0, never read
//   partials    double-buffered: launch k reads buffer k & 1 and writes the
//               other (a stopped launch writes neither)
//   state       double-buffered the same way: read by all, the other copy
//               written by workgroup 0; the caller's record is read by the
//               search launch's workgroup 0 and written by finish
// Workspace (the caller's kind, util.hpp): the partials and the two states.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "common/clean.hpp"
#include "hip/util.hpp"

namespace idg_mi355x {
namespace minor {

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
// two partial buffers describes the planes as they stand.  (32 bytes for
// either cycle.)
template <class Cycle>
struct alignas(8) DevState {
  typename Cycle::State s;
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

// One pass over tile `tile` on every plane: with kSub, the subtraction of a
// component c of scale s on its pixels inside the patch; then the tile's
// partial.  kVec: G % 4 == 0 and the planes are aligned, so a lane takes four
// pixels of a row as one float4 (the PSF row is offset by px - Gp / 2 against
// it: dword loads).
template <class Cycle, bool kVec, bool kSub>
__device__ inline void scan_tile(const typename Cycle::Params &p,
                                 const Tiling &t, int tile, float c, int s,
                                 const clean::Patch &pt, float *planes,
                                 const float *__restrict__ psf,
                                 const uint8_t *__restrict__ mask,
                                 u64 *keys_out, float *vals_out, u64 *lds) {
  constexpr int kN = kVec ? 4 : 1;
  const int tid = threadIdx.x;
  const int G = Cycle::base(p).grid_size, Gp = Cycle::base(p).psf_size;
  const size_t cells = static_cast<size_t>(G) * G;
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows;
  const int row1 = row0 + t.rows < G ? row0 + t.rows : G;
  const int col = tx * kTileCols + (kVec ? (tid & 63) * 4 : tid);
  const int first = row0 + (kVec ? tid >> 6 : 0);
  u64 best = 0;
  float best_v = 0.0f;
  if (col < G) {
    for (int q = 0; q < Cycle::planes(p); ++q) {
      float *plane = planes + q * cells;
      const float *patch = kSub ? psf + Cycle::psf_at(p, s, q) : nullptr;
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
              r[k] = clean::subtract(c, patch[prow + (x - pt.ox)], r[k]);
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
              Cycle::key_of(p, q, r[k], static_cast<uint32_t>(at + k),
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

template <class Cycle, bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_minor_search_mi355x(typename Cycle::Params p, Tiling t,
                               float *planes,
                               const uint8_t *__restrict__ mask,
                               const typename Cycle::State *caller_state,
                               DevState<Cycle> *st_out, u64 *keys_out,
                               float *vals_out) {
  __shared__ u64 lds[kWaves];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    DevState<Cycle> st;
    st.s = *caller_state;
    st.partials_at = 0;
    *st_out = st;
  }
  const clean::Patch none = {0, 0, 0, 0, 0, 0};
  scan_tile<Cycle, kVec, false>(p, t, blockIdx.x, 0.0f, 0, none, planes,
                                nullptr, mask, keys_out, vals_out, lds);
}

// taps: what Cycle::add_to_model reads beside the component (Hogbom: null).
template <class Cycle, bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_minor_iterate_mi355x(typename Cycle::Params p, Tiling t,
                                float *planes, const float *__restrict__ psf,
                                const float *__restrict__ taps,
                                const uint8_t *__restrict__ mask, float *model,
                                typename Cycle::Component *components,
                                const DevState<Cycle> *__restrict__ st_in,
                                DevState<Cycle> *st_out,
                                const u64 *__restrict__ keys_in,
                                const float *__restrict__ vals_in,
                                u64 *keys_out, float *vals_out,
                                int out_index) {
  __shared__ u64 lds_peak[kWaves], lds_tile[kWaves];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const bool scribe = tile == 0 && tid == 0;
  const clean::Params &base = Cycle::base(p);
  DevState<Cycle> st = *st_in;
  if (Cycle::base(st.s).reason != clean::kRunning ||
      !clean::state_ok(Cycle::base(st.s), base)) {
    if (scribe) *st_out = st;
    return;
  }
  u64 key = 0;
  for (int i = tid; i < t.nr_tiles; i += kBlock) {
    const u64 k = keys_in[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds_peak);
  const int G = base.grid_size;
  int py = 0, px = 0, s = 0, owner = -1;
  uint32_t index = 0;
  float v = 0.0f;
  if (key != 0) {
    index = Cycle::index_of(key);
    s = Cycle::scale_of(key);
    py = static_cast<int>(index / static_cast<uint32_t>(G));
    px = static_cast<int>(index - static_cast<uint32_t>(py) * G);
    owner = (py / t.rows) * t.tiles_x + px / kTileCols;
    v = vals_in[owner];
  }
  float c = 0.0f;
  if (!Cycle::step(&st.s, p, key, v, &c)) {
    if (scribe) *st_out = st;
    return;
  }
  if (scribe) {
    components[Cycle::base(st.s).n_components - 1] =
        Cycle::record(py, px, s, c);
    st.partials_at = out_index;
    *st_out = st;
  }
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows, col0 = tx * kTileCols;
  const int row1 = row0 + t.rows < G ? row0 + t.rows : G;
  const int col1 = col0 + kTileCols < G ? col0 + kTileCols : G;
  Cycle::add_to_model(p, taps, model, c, s, index, py, px, tile == owner,
                      row0, row1, col0, col1);

  const clean::Patch pt = clean::patch_of(base, py, px);
  const bool touched = row0 < pt.y1 && row0 + t.rows > pt.y0 &&
                       col0 < pt.x1 && col0 + kTileCols > pt.x0;
  if (!touched && !t.rescan) {
    if (tid == 0) {
      keys_out[tile] = keys_in[tile];
      vals_out[tile] = vals_in[tile];
    }
    return;
  }
  scan_tile<Cycle, kVec, true>(p, t, tile, c, s, pt, planes, psf, mask,
                               keys_out, vals_out, lds_tile);
}

template <class Cycle>
__global__ void __launch_bounds__(kBlock)
    kernel_minor_finish_mi355x(int nr_tiles,
                               const DevState<Cycle> *__restrict__ st_in,
                               const u64 *__restrict__ keys,
                               typename Cycle::State *caller_state) {
  __shared__ u64 lds[kWaves];
  const u64 *from = keys + static_cast<size_t>(st_in->partials_at) * nr_tiles;
  u64 key = 0;
  for (int i = threadIdx.x; i < nr_tiles; i += kBlock) {
    const u64 k = from[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds);
  if (threadIdx.x == 0) {
    typename Cycle::State s = st_in->s;
    Cycle::set_peak(&s, key);
    *caller_state = s;
  }
}

inline Tiling tiling_of(int grid_size) {
  Tiling t;
  t.tiles_x = (grid_size + kTileCols - 1) / kTileCols;
  const int max_y = kMaxTiles / t.tiles_x;
  t.rows = (grid_size + max_y - 1) / max_y;
  if (t.rows < kMinTileRows) t.rows = kMinTileRows;
  t.tiles_y = (grid_size + t.rows - 1) / t.rows;
  t.nr_tiles = t.tiles_x * t.tiles_y;
  // IDG_CLEAN_RESCAN=1: no tile of either cycle carries its partial forward
  // (the comparison of tools/debug/clean_rate.py); the same bytes either way
  const char *knob = std::getenv("IDG_CLEAN_RESCAN");
  t.rescan = knob && knob[0] == '1' ? 1 : 0;
  return t;
}

inline bool aligned(const void *ptr, size_t to) {
  return reinterpret_cast<uintptr_t>(ptr) % to == 0;
}

// One search launch, nr_iterations iteration launches and one finish launch
// on a lease of `workspace` (kWorkspaceClean or kWorkspaceMultiscale).
template <class Cycle>
hipError_t launch(int workspace, const typename Cycle::Params &params,
                  float *d_planes, const float *d_psf, const float *d_taps,
                  const uint8_t *d_mask, float *d_model, void *d_components,
                  void *d_state, hipStream_t stream) {
  using State = DevState<Cycle>;
  static_assert(sizeof(State) == 32, "the lease's layout");
  typename Cycle::Params p = params;
  const int G = Cycle::base(p).grid_size;
  const int nr_iterations = Cycle::base(p).nr_iterations;
  Tiling t = tiling_of(G);
  const bool vec = G % 4 == 0 && aligned(d_planes, 16) && aligned(d_mask, 4);
  const size_t n = static_cast<size_t>(t.nr_tiles);
  WorkspaceLease lease;
  hipError_t err = lease.acquire(
      stream, workspace,
      2 * n * sizeof(u64) + 2 * n * sizeof(float) + 2 * sizeof(State));
  if (err != hipSuccess) return err;
  u64 *keys = static_cast<u64 *>(lease.ptr);
  State *states = reinterpret_cast<State *>(keys + 2 * n);
  float *vals = reinterpret_cast<float *>(states + 2);

  {
    u64 *keys_out = keys;
    float *vals_out = vals;
    State *st_out = states;
    void *args[] = {&p,       &t,      &d_planes, &d_mask,
                    &d_state, &st_out, &keys_out, &vals_out};
    err = hipLaunchKernel(
        vec ? reinterpret_cast<const void *>(
                  &kernel_minor_search_mi355x<Cycle, true>)
            : reinterpret_cast<const void *>(
                  &kernel_minor_search_mi355x<Cycle, false>),
        dim3(t.nr_tiles), dim3(kBlock), args, 0, stream);
    if (err != hipSuccess) return err;
  }
  const void *iterate =
      vec ? reinterpret_cast<const void *>(
                &kernel_minor_iterate_mi355x<Cycle, true>)
          : reinterpret_cast<const void *>(
                &kernel_minor_iterate_mi355x<Cycle, false>);
  for (int k = 0; k < nr_iterations; ++k) {
    const int in = k & 1;
    int out = in ^ 1;
    const State *st_in = states + in;
    State *st_out = states + out;
    const u64 *keys_in = keys + in * n;
    u64 *keys_out = keys + out * n;
    const float *vals_in = vals + in * n;
    float *vals_out = vals + out * n;
    void *args[] = {&p,       &t,        &d_planes, &d_psf,        &d_taps,
                    &d_mask,  &d_model,  &d_components, &st_in,    &st_out,
                    &keys_in, &vals_in,  &keys_out, &vals_out,     &out};
    err = hipLaunchKernel(iterate, dim3(t.nr_tiles), dim3(kBlock), args, 0,
                          stream);
    if (err != hipSuccess) return err;
  }
  const State *st_in = states + (nr_iterations & 1);
  const u64 *keys_in = keys;
  void *args[] = {&t.nr_tiles, &st_in, &keys_in, &d_state};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_minor_finish_mi355x<Cycle>),
      dim3(1), dim3(kBlock), args, 0, stream);
}

}  // namespace minor
}  // namespace idg_mi355x
