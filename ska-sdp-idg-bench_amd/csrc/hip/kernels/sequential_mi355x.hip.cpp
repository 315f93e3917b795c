// sequential_mi355x.hip.cpp -- the order-preserving ("sequential") gridder
// and degridder for MI355X (gfx950): the reference's CPU arithmetic, bit for
// bit, on the GPU.
//
// The default kernels (gridder_mi355x.hip.cpp, degridder_mi355x.hip.cpp) run
// the complex MAC on the matrix cores in K-blocked f16x2-split GEMMs: closer
// to the exact sum of the reference's phases than the reference itself, but
// in a different rounding sequence.  At T x C = 32,768 (BASELINE configs[2])
// the reference metric puts that 1.30e-5 from the reference's own output
// (DESIGN.md §3.1), because the reference's output is itself 1.27e-5 from
// exact.  These kernels instead repeat the reference's rounding sequence:
//
//   gridder   (app/CPU/kernels/gridder_reference.cpp:42-110)
//     per pixel, per correlation: for t, for c (in that order)
//       phase   = fma(-phase_index, k_c, phase_offset)          (f32, a3)
//       (s, c)  = glibc sincosf(phase)      (common/sincosf_glibc.hpp)
//       prod    = (fma(vr, c, -(vi*s)), fma(vi, c, vr*s))        (cmul_b)
//       pixel  += prod                               (two f32 adds)
//     then A1^H P A2 with the reference's product forms, then * taper;
//   degridder (app/CPU/kernels/degridder_reference.cpp:35-125)
//     P' = A1 (sph P) A2^H per pixel, then per (t, c): for y, for x (in that
//     order) sum += P'(y, x) * (s, c) (cmul_b), phase = fma(phase_index, k,
//     -phase_offset) with phase_index = fma(u, l, v*m) + w*n.
//
// Every operation is the one GCC emitted for the reference (oracle/
// idg_oracle.c is the same arithmetic restated in C and is bit-exact to the
// reference build on every golden case), so the outputs are the reference's
// bits.  Selected by IDG_GRIDDER_IMPL=sequential / IDG_DEGRIDDER_IMPL=
// sequential (read per call, util.hpp select_*); same 13-argument kernel ABI
// and launch shape (grid = nr_subgrids, block = 256) as every other kernel.
//
// Layout of the work:
//  * gridder: one workgroup of 256 lanes per subgrid; a lane owns pixels
//    whole (all four correlations, 8 f32 accumulators each), loops t then c
//    with the timestep's uvw and the visibility (wave-uniform: scalar loads)
//    and sums in the reference order.  Mirror pairs (even S, w = 0 and
//    w_offset = 0 on the subgrid, as the MFMA kernels): pixel npix-1-p has
//    the exact negated phase, and glibc's sincosf is exactly odd / even
//    (tests/test_host.py: every finite float), so one sincosf serves both;
//    the lane checks the negation bit for bit per phasor and evaluates the
//    mirror's own sincosf where it does not hold.  The pixel sums are
//    seq_common.hpp's order_grid_pixels, the body the ordered gridder runs
//    too; this file supplies its phasor (GlibcPhasor) and the kernel.
//  * degridder: one workgroup per subgrid; the A-termed, tapered pixels and
//    their (l, m, n, phase_offset) go to LDS in chunks of 1,024 pixels; a
//    lane owns (t, c) visibilities and sums over the pixels in y, x order,
//    its partial sums carried from one chunk to the next.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "../util.hpp"
#include "common/sincosf_glibc.hpp"
#include "device.hpp"
#include "seq_common.hpp"

namespace idg_mi355x {

namespace {

// The phasor policy of seq_common.hpp's order_grid_pixels: glibc's sincosf
// from the LDS windows.  The mirror starts from the conjugate (glibc's
// sincosf is exactly odd / even) and evaluates its own sincosf only where
// its phase is not the negation.
struct GlibcPhasor {
  const idg::SincosfWindow *__restrict__ win;
  __device__ __forceinline__ void operator()(float ph, float *sn,
                                             float *cs) const {
    idg::sincosf_glibc_dev(ph, sn, cs, win);
  }
  __device__ __forceinline__ void mirror(float phm, bool neg, float sn,
                                         float cs, float *snm,
                                         float *csm) const {
    *snm = -sn;
    *csm = cs;
    if (!neg) idg::sincosf_glibc_dev(phm, snm, csm, win);
  }
};

}  // namespace

// grid = nr_subgrids, block = kSeqBlock; the 13-argument kernel ABI.
template <int S_CT>
__global__ void __launch_bounds__(kSeqBlock)
    kernel_gridder_sequential_mi355x(
        const int grid_size, int subgrid_size, float image_size,
        float w_step_in_lambda, int nr_channels, int nr_stations,
        const idg::UVWCoordinate<float> *__restrict__ uvw,
        const float *__restrict__ wavenumbers,
        const float2 *__restrict__ visibilities,
        const float *__restrict__ spheroidal,
        const float2 *__restrict__ aterms,
        const idg::Metadata *__restrict__ metadata,
        float2 *__restrict__ subgrids) {
  __shared__ idg::SincosfWindow win[idg::kSincosfWindows];
  __shared__ float4 st_vis[kSeqStage * 2];  // staged visibilities (24 KB
  __shared__ float4 st_uvwk[kSeqStage];     // with their (u, v, w, k))
  const int S = S_CT > 0 ? S_CT : subgrid_size;
  const int npix = S * S;
  const int s = xcd_subgrid(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  idg::sincosf_windows_to_lds(win, tid);  // the barrier below publishes it
  const SubgridSetup g = setup_subgrid(metadata, s, grid_size, S, image_size,
                                       w_step_in_lambda);
  float2 *out = subgrids + static_cast<size_t>(s) * 4 * npix;
  const GlibcPhasor phasor{win};
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
                                  st_vis, st_uvwk, phasor);
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
                                 st_vis, st_uvwk, phasor);
  }
}

// ---------------------------------------------------------------------------
// Degridder.
// ---------------------------------------------------------------------------
constexpr int kSeqChunk = 1024;  // pixels per LDS chunk
constexpr int kSeqItems = 4;     // (t, c) visibilities per lane per pass

// One LDS chunk of np pixels, in y, x order, into the lane's kSeqItems
// partial sums.
//  WZ      every item's w is +0.0 (the wave's choice), so w * n is +0 (n =
//          compute_n is finite and >= +0) and phase_index = fma(u, l, v*m) +
//          w*n is fma(u, l, v*m) + 0.0f bit for bit, one multiply fewer;
//  SAME_T  the lane's items are consecutive channels of one timestep (C a
//          multiple of kSeqItems), so they share phase_index: formed once
//          per pixel instead of once per item.
template <bool WZ, bool SAME_T>
__device__ __forceinline__ void seq_degrid_chunk(
    int np, const float4 *__restrict__ lds_geo,
    const float4 *__restrict__ lds_pix, const float (&u)[kSeqItems],
    const float (&v)[kSeqItems], const float (&w)[kSeqItems],
    const float (&k)[kSeqItems], f2v (&sum)[kSeqItems][4],
    const idg::SincosfWindow *__restrict__ win) {
  for (int e = 0; e < np; ++e) {
    const float4 geo = lds_geo[e];
    const float4 pa = lds_pix[2 * e], pb = lds_pix[2 * e + 1];
    float pidx[kSeqItems];
#pragma unroll
    for (int j = 0; j < kSeqItems; ++j) {
      // phase_index = fma(u, l, v*m) + w*n
      if (SAME_T && j > 0) {
        pidx[j] = pidx[0];
      } else {
        pidx[j] = fma_(u[j], geo.x, v[j] * geo.y) +
                  (WZ ? 0.0f : w[j] * geo.z);
      }
    }
#pragma unroll
    for (int j = 0; j < kSeqItems; ++j) {
      const float ph = fma_(pidx[j], k[j], -geo.w);  // fma(pidx, k, -poff)
      float sn, cs;
      idg::sincosf_glibc_dev(ph, &sn, &cs, win);
      mac_ref(sum[j], pa, pb, cs, sn);
    }
  }
}

template <int S_CT>
__global__ void __launch_bounds__(kSeqBlock)
    kernel_degridder_sequential_mi355x(
        const int grid_size, int subgrid_size, float image_size,
        float w_step_in_lambda, int nr_channels, int nr_stations,
        const idg::UVWCoordinate<float> *__restrict__ uvw,
        const float *__restrict__ wavenumbers,
        float2 *__restrict__ visibilities,
        const float *__restrict__ spheroidal,
        const float2 *__restrict__ aterms,
        const idg::Metadata *__restrict__ metadata,
        const float2 *__restrict__ subgrids) {
  __shared__ float4 lds_pix[kSeqChunk * 2];  // P' of the chunk: xx|xy, yx|yy
  __shared__ float4 lds_geo[kSeqChunk];      // (l, m, n, phase_offset)
  __shared__ idg::SincosfWindow win[idg::kSincosfWindows];
  const int S = S_CT > 0 ? S_CT : subgrid_size;
  const int npix = S * S;
  const int s = xcd_subgrid(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x;
  // published by the chunk loop's first barrier, before any phasor
  idg::sincosf_windows_to_lds(win, tid);
  const SubgridSetup g = setup_subgrid(metadata, s, grid_size, S, image_size,
                                       w_step_in_lambda);
  const int C = nr_channels;
  const float2 *sg = subgrids + static_cast<size_t>(s) * 4 * npix;
  const long long items = static_cast<long long>(g.nr_timesteps) * C;
  // C a multiple of kSeqItems: a lane's items are kSeqItems consecutive
  // channels of one timestep (all valid or all past the end together, since
  // items and every i0 are multiples of kSeqItems); otherwise kSeqBlock
  // apart
  const bool same_t = C % kSeqItems == 0;
  for (long long i0 = 0; i0 < items; i0 += kSeqBlock * kSeqItems) {
    f2v sum[kSeqItems][4];
    float u[kSeqItems], v[kSeqItems], w[kSeqItems], k[kSeqItems];
#pragma unroll
    for (int j = 0; j < kSeqItems; ++j) {
      const long long it =
          min(i0 + (same_t ? kSeqItems * tid + j : j * kSeqBlock + tid),
              items - 1);
      const int t = static_cast<int>(it / C), c = static_cast<int>(it % C);
      const idg::UVWCoordinate<float> c3 = uvw[g.time_offset + t];
      u[j] = c3.u;
      v[j] = c3.v;
      w[j] = c3.w;
      k[j] = wavenumbers[c];
#pragma unroll
      for (int q = 0; q < 4; ++q) sum[j][q] = f2v{0.0f, 0.0f};
    }
    bool wz = true;
#pragma unroll
    for (int j = 0; j < kSeqItems; ++j)
      wz = wz && __builtin_bit_cast(unsigned, w[j]) == 0u;
    for (int p0 = 0; p0 < npix; p0 += kSeqChunk) {
      const int np = min(kSeqChunk, npix - p0);
      __syncthreads();  // the previous chunk's readers are done
      for (int e = tid; e < np; e += kSeqBlock) {
        const int p = p0 + e, y = p / S, x = p - y * S;
        const float sph = spheroidal[p];
        idg::cfloat pix[4], a1[4], a2[4];
#pragma unroll
        for (int cr = 0; cr < 4; ++cr) {
          const float2 q = sg[static_cast<size_t>(cr) * npix + p];
          pix[cr] = {sph * q.x, sph * q.y};
        }
        load_jones(aterm_ptr(aterms, nr_stations, S, g.aterm_index,
                             g.station1, y, x), a1);
        load_jones(aterm_ptr(aterms, nr_stations, S, g.aterm_index,
                             g.station2, y, x), a2);
        idg::apply_aterm_degridder(pix, a1, a2);
        const float l = idg::compute_l(x, S, image_size);
        const float m = idg::compute_m(y, S, image_size);
        const float n = idg::compute_n(l, m);
        // phase_offset = fma(u_o, l, v_o*m) + w_o*n (degridder fusion)
        const float poff = fma_(g.u_offset, l, g.v_offset * m) + g.w_offset * n;
        lds_pix[2 * e] = make_float4(pix[0].re, pix[0].im, pix[1].re, pix[1].im);
        lds_pix[2 * e + 1] =
            make_float4(pix[2].re, pix[2].im, pix[3].re, pix[3].im);
        lds_geo[e] = make_float4(l, m, n, poff);
      }
      __syncthreads();
      if (same_t) {
        if (__all(wz))
          seq_degrid_chunk<true, true>(np, lds_geo, lds_pix, u, v, w, k, sum,
                                       win);
        else
          seq_degrid_chunk<false, true>(np, lds_geo, lds_pix, u, v, w, k, sum,
                                        win);
      } else {
        if (__all(wz))
          seq_degrid_chunk<true, false>(np, lds_geo, lds_pix, u, v, w, k, sum,
                                        win);
        else
          seq_degrid_chunk<false, false>(np, lds_geo, lds_pix, u, v, w, k,
                                         sum, win);
      }
    }
#pragma unroll
    for (int j = 0; j < kSeqItems; ++j) {
      const long long it =
          i0 + (same_t ? kSeqItems * tid + j : j * kSeqBlock + tid);
      if (it >= items) continue;
      const int t = static_cast<int>(it / C), c = static_cast<int>(it % C);
      float4 *dst = reinterpret_cast<float4 *>(
          visibilities + ((g.time_offset + t) * C + c) * 4);
      dst[0] = make_float4(sum[j][0].x, sum[j][0].y, sum[j][1].x, sum[j][1].y);
      dst[1] = make_float4(sum[j][2].x, sum[j][2].y, sum[j][3].x, sum[j][3].y);
    }
  }
}

// The sequential kernels of subgrid size S (32, 64, or 0 = runtime S).
const void *sequential_gridder(int S) {
  return kernel_for_size(S, [](auto s) {
    return reinterpret_cast<const void *>(
        &kernel_gridder_sequential_mi355x<decltype(s)::value>);
  });
}

const void *sequential_degridder(int S) {
  return kernel_for_size(S, [](auto s) {
    return reinterpret_cast<const void *>(
        &kernel_degridder_sequential_mi355x<decltype(s)::value>);
  });
}

int sequential_block() { return kSeqBlock; }

}  // namespace idg_mi355x
