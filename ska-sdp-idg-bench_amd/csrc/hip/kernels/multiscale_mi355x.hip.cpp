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
// Minor cycle.  The one minor-cycle body of minor_cycle.hpp (the launches and
// who reads and writes which buffer are described there) under ms::Cycle: one
// workgroup owns its tile in all Ns planes, the key is ms::key_of's
// (|weight[s] v|, then lower scale, then lower index), a component of scale s
// subtracts cross(s, q) from plane q, and the model takes the component's
// footprint, each workgroup the pixels of its own tile.  Workspace: util.hpp
// kWorkspaceMultiscale.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common/multiscale.hpp"
#include "hip/kernels/minor_cycle.hpp"
#include "hip/util.hpp"

namespace idg_mi355x {

namespace {

constexpr int kBlock = 256;
constexpr int kHalo = ms::kMaxRadius;  // LDS room either side of a tile

using minor::aligned;

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
struct MultiScaleCycle : ms::Cycle {
  // Step 7: the footprint's pixels inside this workgroup's tile, rows
  // [row0, row1) x columns [col0, col1).
  __device__ static void add_to_model(const Params &p,
                                      const float *__restrict__ taps,
                                      float *model, float c, int s, uint32_t,
                                      int py, int px, bool, int row0, int row1,
                                      int col0, int col1) {
    const int G = p.base.grid_size, r = p.radius[s];
    const float *h = taps + ms::taps_at(p, s);
    const int ya = py - r > row0 ? py - r : row0;
    const int yb = py + r + 1 < row1 ? py + r + 1 : row1;
    const int xa = px - r > col0 ? px - r : col0;
    const int xb = px + r + 1 < col1 ? px + r + 1 : col1;
    if (ya < yb && xa < xb) {
      const int w = xb - xa, n = w * (yb - ya);
      for (int i = threadIdx.x; i < n; i += minor::kBlock) {
        const int y = ya + i / w, x = xa + i % w;
        float *m = model + static_cast<size_t>(y) * G + x;
        *m = ms::model_add(c, h[y - py + r], h[x - px + r], *m);
      }
    }
  }
};

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
  return minor::launch<MultiScaleCycle>(kWorkspaceMultiscale, params, d_planes,
                                        d_cross_psf, d_taps, d_mask, d_model,
                                        d_components, d_state, stream);
}

}  // namespace idg_mi355x
