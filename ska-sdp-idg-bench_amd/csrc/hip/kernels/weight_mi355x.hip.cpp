// weight_mi355x.hip.cpp -- imaging weights on the device: the
// uv sampling density of the samples the gridder will grid, the (a, b) of a
// weighting scheme and the imaging weights f = w / (a + b D), bit for bit what
// the host entries compute (common/weight.hpp holds the arithmetic of both).
//   density  one workgroup per subgrid: the samples' quantised weights summed
//            in an S x S uint64 tile in LDS, its non-zero cells added to the
//            grid with 64-bit integer atomics; a sample outside the tile is
//            added to the grid directly.  Integer sums: any order, the same
//            bits.
//   scheme   sums of D and D^2 over the G^2 cells in a fixed tree (per
//            workgroup partials, then one workgroup over the partials), (a, b)
//   apply    one workgroup per subgrid: f, the weighted visibilities and the
//            subgrid's partial of sum f; then one workgroup over the partials
// No atomics but the density's, no cross-workgroup wait: kernel boundaries
// order the stages.  Workspace (util.hpp kWorkspaceWeight): the partials.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "common/weight.hpp"
#include "hip/util.hpp"

namespace idg_mi355x {

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 8;          // channels of one row a thread walks
constexpr int kMaxTile = 64;       // S above this: no tile (S^2 uint64 of LDS)
constexpr int kSchemeCells = 4096; // cells per workgroup of the scheme's sums
constexpr int kMetaWords = 9;

using u64 = unsigned long long;

// Row of timestep 0 of subgrid s, and its timesteps (include/idg_mi355x.h).
__device__ inline long long first_row(const int32_t *metadata, int s,
                                      int *nr_timesteps) {
  const int32_t *m = metadata + static_cast<size_t>(s) * kMetaWords;
  *nr_timesteps = m[2];
  return (static_cast<long long>(m[0]) - metadata[0]) + m[1];
}

// i / n for 0 <= i, 0 < n; in 32 bits where the (uniform) caller says i fits.
__device__ inline long long split(long long i, int n, bool small) {
  return small ? static_cast<long long>(static_cast<unsigned>(i) /
                                        static_cast<unsigned>(n))
               : i / n;
}

// Sum of v over the workgroup in a fixed order (thread-indexed tree in LDS);
// valid in thread 0.
__device__ inline double block_sum(double v, double *lds) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
#pragma unroll
  for (int d = kBlock / 2; d > 0; d /= 2) {
    if (tid < d) lds[tid] += lds[tid + d];
    __syncthreads();
  }
  return lds[0];
}

__global__ void __launch_bounds__(kBlock)
    kernel_weight_density_mi355x(weight::Geometry g, int tile, int nr_channels,
                                 const int32_t *__restrict__ metadata,
                                 const float *__restrict__ uvw,
                                 const float *__restrict__ wavenumbers,
                                 const float *__restrict__ weights,
                                 u64 *__restrict__ density) {
  extern __shared__ u64 cells[];  // [tile][tile]
  const int s = blockIdx.x, tid = threadIdx.x;
  int T;
  const long long row0 = first_row(metadata, s, &T);
  const int32_t *m = metadata + static_cast<size_t>(s) * kMetaWords;
  const unsigned x0 = static_cast<unsigned>(m[6]);
  const unsigned y0 = static_cast<unsigned>(m[7]);
  const unsigned side = static_cast<unsigned>(tile);
  for (int i = tid; i < tile * tile; i += kBlock) cells[i] = 0;
  __syncthreads();

  const size_t G = static_cast<size_t>(g.grid_size);
  // a run of one row's consecutive channels in one cell is added once
  const auto add = [&](int x, int y, u64 q) {
    const unsigned tx = static_cast<unsigned>(x) - x0;
    const unsigned ty = static_cast<unsigned>(y) - y0;
    if (tx < side && ty < side)
      atomicAdd(&cells[ty * side + tx], q);
    else
      atomicAdd(&density[static_cast<size_t>(y) * G + x], q);
  };
  const int chunks = (nr_channels + kChunk - 1) / kChunk;
  const long long items = static_cast<long long>(T) * chunks;
  const bool small = items <= INT32_MAX;
  for (long long i = tid; i < items; i += kBlock) {
    const long long t = split(i, chunks, small);
    const int c0 = static_cast<int>(i - t * chunks) * kChunk;
    const int c1 = c0 + kChunk < nr_channels ? c0 + kChunk : nr_channels;
    const size_t row = static_cast<size_t>(row0 + t);
    const float u = uvw[row * 3], v = uvw[row * 3 + 1];
    const float *w = weights + row * nr_channels;
    int run_x = 0, run_y = 0;
    u64 run = 0;
    for (int c = c0; c < c1; ++c) {
      int x, y;
      const u64 q = weight::sample(g, u, v, wavenumbers[c], w[c], &x, &y);
      if (q == 0) continue;
      if (run != 0 && (x != run_x || y != run_y)) {
        add(run_x, run_y, run);
        run = 0;
      }
      run_x = x;
      run_y = y;
      run += q;
    }
    if (run != 0) add(run_x, run_y, run);
  }
  __syncthreads();
  // a tile cell that holds something had an in-grid sample: it is in the grid
  for (int i = tid; i < tile * tile; i += kBlock) {
    const u64 q = cells[i];
    if (q == 0) continue;
    const size_t y = static_cast<size_t>(y0 + static_cast<unsigned>(i / tile));
    const size_t x = static_cast<size_t>(x0 + static_cast<unsigned>(i % tile));
    atomicAdd(&density[y * G + x], q);
  }
}

// Partial sums of D and D^2 over cells [blockIdx.x * kSchemeCells, + kSchemeCells).
__global__ void __launch_bounds__(kBlock)
    kernel_weight_sums_mi355x(weight::Geometry g,
                              const u64 *__restrict__ density,
                              double *__restrict__ partials) {
  __shared__ double lds[kBlock];
  const size_t G = static_cast<size_t>(g.grid_size), cells = G * G;
  const size_t base = static_cast<size_t>(blockIdx.x) * kSchemeCells;
  double sd = 0.0, sd2 = 0.0;
  for (int k = threadIdx.x; k < kSchemeCells; k += kBlock) {
    const size_t i = base + k;
    if (i >= cells) break;
    const double D = weight::density_of(
        weight::count_at(g, reinterpret_cast<const uint64_t *>(density),
                         static_cast<int>(i % G), static_cast<int>(i / G)),
        g.quantum_log2);
    sd += D;
    sd2 += D * D;
  }
  sd = block_sum(sd, lds);
  __syncthreads();
  sd2 = block_sum(sd2, lds);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = sd;
    partials[2 * blockIdx.x + 1] = sd2;
  }
}

// One workgroup: the partials summed in a fixed order, then (a, b).
__global__ void __launch_bounds__(kBlock)
    kernel_weight_scheme_mi355x(int scheme, double briggs_scale, int nr_partials,
                                const double *__restrict__ partials,
                                float *__restrict__ ab) {
  __shared__ double lds[kBlock];
  double sd = 0.0, sd2 = 0.0;
  for (int i = threadIdx.x; i < nr_partials; i += kBlock) {
    sd += partials[2 * i];
    sd2 += partials[2 * i + 1];
  }
  sd = block_sum(sd, lds);
  __syncthreads();
  sd2 = block_sum(sd2, lds);
  if (threadIdx.x == 0)
    weight::scheme_ab(scheme, briggs_scale, sd, sd2, &ab[0], &ab[1]);
}

__global__ void __launch_bounds__(kBlock)
    kernel_weight_apply_mi355x(weight::Geometry g, int nr_channels,
                               const int32_t *__restrict__ metadata,
                               const float *__restrict__ uvw,
                               const float *__restrict__ wavenumbers,
                               const float *__restrict__ weights,
                               const u64 *__restrict__ density,
                               const float *__restrict__ ab,
                               const float4 *visibilities,
                               float *__restrict__ imaging_weights,
                               float4 *out, double *__restrict__ partials) {
  __shared__ double lds[kBlock];
  const int s = blockIdx.x;
  int T;
  const long long row0 = first_row(metadata, s, &T);
  const float a = ab[0], b = ab[1];
  const long long items = static_cast<long long>(T) * nr_channels;
  const bool small = items <= INT32_MAX;
  double sum = 0.0;
  for (long long i = threadIdx.x; i < items; i += kBlock) {
    const long long t = split(i, nr_channels, small);
    const size_t row = static_cast<size_t>(row0 + t);
    const int c = static_cast<int>(i - t * nr_channels);
    const size_t at = row * nr_channels + c;
    const float w = weights[at];
    int x, y;
    float f = 0.0f;
    const bool live = weight::sample(g, uvw[row * 3], uvw[row * 3 + 1],
                                     wavenumbers[c], w, &x, &y) != 0;
    if (live)
      f = weight::imaging_weight(
          w, a, b,
          weight::density_of(
              weight::count_at(g, reinterpret_cast<const uint64_t *>(density),
                               x, y),
              g.quantum_log2));
    // (xx, xy) and (yx, yy) as two float4; a flagged sample writes literal
    // zeros, whatever its visibility holds
    float4 lo = make_float4(f, 0.0f, 0.0f, 0.0f);
    float4 hi = make_float4(0.0f, 0.0f, f, 0.0f);
    if (visibilities != nullptr) {
      if (live) {
        const float4 p = visibilities[2 * at], q = visibilities[2 * at + 1];
        lo = make_float4(f * p.x, f * p.y, f * p.z, f * p.w);
        hi = make_float4(f * q.x, f * q.y, f * q.z, f * q.w);
      } else {
        lo = hi = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
    }
    imaging_weights[at] = f;
    out[2 * at] = lo;
    out[2 * at + 1] = hi;
    sum += f;
  }
  sum = block_sum(sum, lds);
  if (threadIdx.x == 0) partials[s] = sum;
}

// One workgroup: sum f over the subgrids' partials in a fixed order.
__global__ void __launch_bounds__(kBlock)
    kernel_weight_total_mi355x(int nr_partials,
                               const double *__restrict__ partials,
                               double *__restrict__ sum_weights) {
  __shared__ double lds[kBlock];
  double sum = 0.0;
  for (int i = threadIdx.x; i < nr_partials; i += kBlock) sum += partials[i];
  sum = block_sum(sum, lds);
  if (threadIdx.x == 0) *sum_weights = sum;
}

}  // namespace

hipError_t launch_weight_density(const weight::Geometry &geometry,
                                 int nr_subgrids, int subgrid_size,
                                 int nr_channels, const void *d_metadata,
                                 const void *d_uvw, const float *d_wavenumbers,
                                 const float *d_weights, void *d_density,
                                 hipStream_t stream) {
  if (nr_subgrids <= 0) return hipSuccess;
  weight::Geometry g = geometry;
  // IDG_WEIGHT_TILE=0: every sample down the global-atomic path (the
  // comparison of tools/debug/weight_rate.py)
  const char *knob = std::getenv("IDG_WEIGHT_TILE");
  int tile = subgrid_size <= kMaxTile && !(knob && knob[0] == '0')
                 ? subgrid_size
                 : 0;
  void *args[] = {&g,     &tile,          &nr_channels, &d_metadata,
                  &d_uvw, &d_wavenumbers, &d_weights,   &d_density};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_weight_density_mi355x),
      dim3(nr_subgrids), dim3(kBlock), args,
      static_cast<size_t>(tile) * tile * sizeof(u64), stream);
}

hipError_t launch_weight_scheme(const weight::Geometry &geometry, int scheme,
                                double briggs_scale, const void *d_density,
                                float *d_ab, hipStream_t stream) {
  weight::Geometry g = geometry;
  const size_t cells = static_cast<size_t>(g.grid_size) * g.grid_size;
  int nr_partials = scheme == weight::kBriggs
                        ? static_cast<int>((cells + kSchemeCells - 1) /
                                           kSchemeCells)
                        : 0;
  WorkspaceLease lease;
  hipError_t err = lease.acquire(
      stream, kWorkspaceWeight,
      sizeof(double) * 2 * static_cast<size_t>(nr_partials > 0 ? nr_partials
                                                                : 1));
  if (err != hipSuccess) return err;
  void *ws = lease.ptr;
  if (nr_partials > 0) {
    void *args[] = {&g, &d_density, &ws};
    err = hipLaunchKernel(
        reinterpret_cast<const void *>(&kernel_weight_sums_mi355x),
        dim3(nr_partials), dim3(kBlock), args, 0, stream);
    if (err != hipSuccess) return err;
  }
  void *args[] = {&scheme, &briggs_scale, &nr_partials, &ws, &d_ab};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_weight_scheme_mi355x), dim3(1),
      dim3(kBlock), args, 0, stream);
}

hipError_t launch_weight_apply(const weight::Geometry &geometry,
                               int nr_subgrids, int nr_channels,
                               const void *d_metadata, const void *d_uvw,
                               const float *d_wavenumbers,
                               const float *d_weights, const void *d_density,
                               const float *d_ab, const void *d_visibilities,
                               float *d_imaging_weights, void *d_out,
                               double *d_sum_weights, hipStream_t stream) {
  weight::Geometry g = geometry;
  WorkspaceLease lease;
  hipError_t err = lease.acquire(
      stream, kWorkspaceWeight,
      sizeof(double) * static_cast<size_t>(nr_subgrids > 0 ? nr_subgrids : 1));
  if (err != hipSuccess) return err;
  void *ws = lease.ptr;
  if (nr_subgrids > 0) {
    void *args[] = {&g,          &nr_channels, &d_metadata, &d_uvw,
                    &d_wavenumbers, &d_weights, &d_density, &d_ab,
                    &d_visibilities, &d_imaging_weights, &d_out, &ws};
    err = hipLaunchKernel(
        reinterpret_cast<const void *>(&kernel_weight_apply_mi355x),
        dim3(nr_subgrids), dim3(kBlock), args, 0, stream);
    if (err != hipSuccess) return err;
  }
  void *args[] = {&nr_subgrids, &ws, &d_sum_weights};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_weight_total_mi355x), dim3(1),
      dim3(kBlock), args, 0, stream);
}

}  // namespace idg_mi355x
