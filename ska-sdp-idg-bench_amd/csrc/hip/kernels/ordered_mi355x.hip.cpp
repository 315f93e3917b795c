// ordered_mi355x.hip.cpp -- the "ordered" gridder for MI355X (gfx950): the
// reference's summation order with the hardware's sin / cos.
//
// The reference's own f32 sum is 1.27e-5 from the exact sum at T x C =
// 32,768 (BASELINE configs[2], the -c NR_CHANNELS=256 shape), so a kernel
// that sums in another sequence -- the default matrix-core gridder, itself
// closer to exact -- lands one such error away from the reference and misses
// the reference's 1e-5 bar there.  The sequential gridder
// (sequential_mi355x.hip.cpp) passes by repeating every bit, at the price of
// a restated glibc sincosf in f64.  The bar needs the order
// only.  This kernel keeps, per pixel and correlation,
//
//   for t, for c (in that order)
//     phase   = fma(-phase_index, k_c, phase_offset)     (f32, as reference)
//     (s, c)  = sincos_rev(revolutions(phase))           (device.hpp)
//     prod    = (fma(vr, c, -(vi*s)), fma(vi, c, vr*s))  (cmul_b)
//     pixel  += prod                                     (two f32 adds)
//   then A1^H P A2 with the reference's product forms, then * taper,
//
// so its output differs from the reference's only by what the phasor's
// error (revolutions(): <~ 3e-8 revolutions; v_sin_f32 / v_cos_f32:
// ~1.2e-7 absolute) adds to each term of the same rounding sequence
// (tests/emul/ordered_emul.py).  The phase is reduced whole,
// per phasor: the MFMA kernels' anchored / incremental reduction rounds the
// phase differently and is not used here.
//
// Selected by Options::gridder_impl = kImplOrdered (IDG_GRIDDER_IMPL=ordered;
// util.hpp select_gridder); the 13-argument kernel ABI, grid = nr_subgrids,
// block = 256.  The auto gridder's queue-fed variant is at the end of this
// file.  The work is laid out as in the sequential gridder, by the same code
// (seq_common.hpp order_grid_pixels; this file supplies HardwarePhasor and
// the kernels): a lane owns pixels whole (8 f32 accumulators each), the
// visibilities and (u, v, w, k) come through LDS kSeqStage (t, c) items at a
// time, and on mirror subgrids (even S, w = 0 and w_offset = 0) pixel
// npix-1-p takes the base pixel's phasor conjugated wherever its own phase
// is the bitwise negation of the base phase -- checked per phasor; where it
// is not, the mirror's own phasor is evaluated.  No sincosf tables: the LDS
// holds the staged block only.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../util.hpp"
#include "device.hpp"
#include "seq_common.hpp"

namespace idg_mi355x {

namespace {

// The phasor policy of seq_common.hpp's order_grid_pixels: Dekker reduction
// of the phase (radians) to revolutions, then v_sin_f32 / v_cos_f32 on |r| <=
// 0.5.  The mirror's phasor is evaluated on every lane, then replaced by the
// conjugate where its phase is the negation: the same value whichever branch
// the wave takes.
struct HardwarePhasor {
  __device__ __forceinline__ void operator()(float ph, float *sn,
                                             float *cs) const {
    sincos_rev(revolutions(ph), sn, cs);
  }
  __device__ __forceinline__ void mirror(float phm, bool neg, float sn,
                                         float cs, float *snm,
                                         float *csm) const {
    (*this)(phm, snm, csm);
    if (neg) {
      *snm = -sn;
      *csm = cs;
    }
  }
};

}  // namespace

// grid = nr_subgrids, block = kSeqBlock; the 13-argument kernel ABI.
template <int S_CT>
__global__ void __launch_bounds__(kSeqBlock)
    kernel_gridder_ordered_mi355x(
        const int grid_size, int subgrid_size, float image_size,
        float w_step_in_lambda, int nr_channels, int nr_stations,
        const idg::UVWCoordinate<float> *__restrict__ uvw,
        const float *__restrict__ wavenumbers,
        const float2 *__restrict__ visibilities,
        const float *__restrict__ spheroidal,
        const float2 *__restrict__ aterms,
        const idg::Metadata *__restrict__ metadata,
        float2 *__restrict__ subgrids) {
  __shared__ float4 st_vis[kSeqStage * 2];  // staged visibilities (24 KB
  __shared__ float4 st_uvwk[kSeqStage];     // with their (u, v, w, k))
  const int S = S_CT > 0 ? S_CT : subgrid_size;
  const int npix = S * S;
  const int s = xcd_subgrid(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  const SubgridSetup g = setup_subgrid(metadata, s, grid_size, S, image_size,
                                       w_step_in_lambda);
  float2 *out = subgrids + static_cast<size_t>(s) * 4 * npix;
  const bool mirror = mirror_eligible(g, S, uvw, tid);
  if (mirror) {
    constexpr int NP = 2;
    const int half = npix / 2;
    for (int tile = 0; tile < half; tile += kSeqBlock * NP) {
      int base[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) base[i] = tile + i * kSeqBlock + tid;
      order_grid_pixels<NP, true>(base, half, S, npix, image_size, g,
                                  nr_channels, nr_stations, uvw, wavenumbers,
                                  visibilities, spheroidal, aterms, out,
                                  st_vis, st_uvwk, HardwarePhasor{});
    }
    return;
  }
  constexpr int NP = 4;
  for (int tile = 0; tile < npix; tile += kSeqBlock * NP) {
    int base[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) base[i] = tile + i * kSeqBlock + tid;
    order_grid_pixels<NP, false>(base, npix, S, npix, image_size, g,
                                 nr_channels, nr_stations, uvw, wavenumbers,
                                 visibilities, spheroidal, aterms, out,
                                 st_vis, st_uvwk, HardwarePhasor{});
  }
}

// The ordered gridder of subgrid size S (32, 64, or 0 = runtime S).
const void *ordered_gridder(int S) {
  return kernel_for_size(S, [](auto s) {
    return reinterpret_cast<const void *>(
        &kernel_gridder_ordered_mi355x<decltype(s)::value>);
  });
}

int ordered_block() { return kSeqBlock; }

// ---------------------------------------------------------------------------
// The auto gridder's two kernels (util.hpp launch_auto_classify /
// launch_ordered_queue).  Workspace, in ints: [0] the count
// of queued subgrids (zeroed by a memset before the classification), [16,
// 16 + ns) the queue, then the shadow metadata (ns records).
// ---------------------------------------------------------------------------
namespace {
constexpr int kAutoQueue = 16;  // the count has a 64-byte line of its own
constexpr int kClassifyBlock = 256;
}  // namespace

size_t auto_workspace_bytes(int ns) {
  return (kAutoQueue + static_cast<size_t>(ns)) * sizeof(int) +
         static_cast<size_t>(ns) * sizeof(idg::Metadata);
}

const void *auto_shadow(void *ws, int ns) {
  return static_cast<int *>(ws) + kAutoQueue + ns;
}

// One thread per subgrid.  A wave's pushes take one atomic (a count per push
// serializes: device.hpp, the queue of the two-kernel form); the queue's
// order is therefore not fixed from launch to launch, which no output
// depends on: a queue position only names the subgrid a workgroup computes.
__global__ void __launch_bounds__(kClassifyBlock)
    kernel_auto_classify_mi355x(int nr_subgrids, int nr_channels,
                                unsigned threshold,
                                const idg::Metadata *__restrict__ metadata,
                                int *__restrict__ ws) {
  // a record as its 9 ints (nr_timesteps is the third), kept in registers
  constexpr int kWords = sizeof(idg::Metadata) / sizeof(int);
  static_assert(sizeof(idg::Metadata) == 36 &&
                    offsetof(idg::Metadata, nr_timesteps) == 2 * sizeof(int),
                "metadata layout");
  const int s = blockIdx.x * kClassifyBlock + threadIdx.x;
  const bool live = s < nr_subgrids;
  const int *src = reinterpret_cast<const int *>(metadata) +
                   static_cast<size_t>(live ? s : 0) * kWords;
  int w[kWords];
#pragma unroll
  for (int i = 0; i < kWords; ++i) w[i] = src[i];
  const bool selected =
      live && w[2] > 0 &&
      static_cast<long long>(w[2]) * nr_channels >
          static_cast<long long>(threshold);
  const unsigned long long mask = __ballot(selected);
  const int lane = threadIdx.x & 63;
  int first = 0;
  if (lane == 0 && mask != 0) first = atomicAdd(ws, __popcll(mask));
  first = __shfl(first, 0);
  if (selected) {
    ws[kAutoQueue + first + __popcll(mask & ((1ull << lane) - 1))] = s;
    w[2] = 0;
  }
  if (!live) return;
  int *dst = ws + kAutoQueue + nr_subgrids + static_cast<size_t>(s) * kWords;
#pragma unroll
  for (int i = 0; i < kWords; ++i) dst[i] = w[i];
}

// kernel_gridder_ordered_mi355x over the queue: workgroup b takes slice
// b % slices of the subgrid at queue position b / slices and returns if that
// is past the count.  A slice is a contiguous range of the base pixels (the
// half subgrid on mirror subgrids, else all of it); a lane owns NPM base
// pixels with their mirrors, or 2 NPM pixels (the ordered kernel: NPM = 2).
// Every pixel's sum runs whole, in the same order, in one lane, and the
// mirror check is per lane, so the output is the ordered kernel's bit for
// bit whatever the slicing.  grid = nr_subgrids x slices.
template <int S_CT, int NPM>
__global__ void __launch_bounds__(kSeqBlock)
    kernel_gridder_ordered_queue_mi355x(
        const int grid_size, int subgrid_size, float image_size,
        float w_step_in_lambda, int nr_channels, int nr_stations,
        const idg::UVWCoordinate<float> *__restrict__ uvw,
        const float *__restrict__ wavenumbers,
        const float2 *__restrict__ visibilities,
        const float *__restrict__ spheroidal,
        const float2 *__restrict__ aterms,
        const idg::Metadata *__restrict__ metadata,
        float2 *__restrict__ subgrids, const int *__restrict__ ws,
        int slices) {
  __shared__ float4 st_vis[kSeqStage * 2];
  __shared__ float4 st_uvwk[kSeqStage];
  const int position = blockIdx.x / slices, slice = blockIdx.x % slices;
  if (position >= ws[0]) return;
  const int s = ws[kAutoQueue + position];
  const int S = S_CT > 0 ? S_CT : subgrid_size;
  const int npix = S * S;
  const int tid = threadIdx.x;
  const SubgridSetup g = setup_subgrid(metadata, s, grid_size, S, image_size,
                                       w_step_in_lambda);
  float2 *out = subgrids + static_cast<size_t>(s) * 4 * npix;
  const bool mirror = mirror_eligible(g, S, uvw, tid);
  const int nbase = mirror ? npix / 2 : npix;
  const int span = (nbase + slices - 1) / slices;
  const int lo = slice * span, hi = min(nbase, lo + span);
  if (mirror) {
    constexpr int NP = NPM;
    for (int tile = lo; tile < hi; tile += kSeqBlock * NP) {
      int base[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) base[i] = tile + i * kSeqBlock + tid;
      order_grid_pixels<NP, true>(base, hi, S, npix, image_size, g,
                                  nr_channels, nr_stations, uvw, wavenumbers,
                                  visibilities, spheroidal, aterms, out,
                                  st_vis, st_uvwk, HardwarePhasor{});
    }
    return;
  }
  constexpr int NP = 2 * NPM;
  for (int tile = lo; tile < hi; tile += kSeqBlock * NP) {
    int base[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) base[i] = tile + i * kSeqBlock + tid;
    order_grid_pixels<NP, false>(base, hi, S, npix, image_size, g,
                                 nr_channels, nr_stations, uvw, wavenumbers,
                                 visibilities, spheroidal, aterms, out,
                                 st_vis, st_uvwk, HardwarePhasor{});
  }
}

hipError_t launch_auto_classify(int nr_subgrids, int nr_channels,
                                unsigned threshold, const void *d_metadata,
                                void *ws, hipStream_t stream) {
  hipError_t err = hipMemsetAsync(ws, 0, sizeof(int), stream);
  if (err != hipSuccess) return err;
  void *args[] = {&nr_subgrids, &nr_channels, &threshold, &d_metadata, &ws};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_auto_classify_mi355x),
      dim3((nr_subgrids + kClassifyBlock - 1) / kClassifyBlock),
      dim3(kClassifyBlock), args, 0, stream);
}

hipError_t launch_ordered_queue(const Problem &p, void **args13, void *ws,
                                int slices, hipStream_t stream) {
  // whole pixels per lane: one slice keeps the ordered kernel's 2 (+ their
  // mirrors), finer slicings take 1
  const void *func = kernel_for_size(p.subgrid_size, [slices](auto s) {
    constexpr int S_CT = decltype(s)::value;
    return slices > 1 ? reinterpret_cast<const void *>(
                            &kernel_gridder_ordered_queue_mi355x<S_CT, 1>)
                      : reinterpret_cast<const void *>(
                            &kernel_gridder_ordered_queue_mi355x<S_CT, 2>);
  });
  void *args[15];
  for (int i = 0; i < 13; ++i) args[i] = args13[i];
  args[13] = &ws;
  args[14] = &slices;
  const long long grid = static_cast<long long>(p.nr_subgrids) * slices;
  if (slices < 1 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
  return hipLaunchKernel(func, dim3(static_cast<unsigned>(grid)),
                         dim3(kSeqBlock), args, 0, stream);
}

}  // namespace idg_mi355x
