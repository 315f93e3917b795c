// seq_common.hpp -- what the kernels that keep the reference's summation
// order share: the reference's complex multiply-accumulate restated for
// gfx950, the mirror-eligibility check, and the gridders' pixel-sum body
// (order_grid_pixels, the phasor a policy).  Included by
// sequential_mi355x.hip.cpp (glibc sincosf: the reference's bits) and
// ordered_mi355x.hip.cpp (hardware sin / cos: the reference's order).
#pragma once

#include <hip/hip_runtime.h>

#include "device.hpp"

namespace idg_mi355x {

namespace {

constexpr int kSeqBlock = 256;
constexpr int kSeqStage = 512;  // gridder: (t, c) items per LDS block

__device__ __forceinline__ unsigned fbits(float x) {
  return __builtin_bit_cast(unsigned, x);
}

// Packed f32 pairs (re, im): v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32
// round each half exactly as the scalar instruction does, so the packed MACs
// below are the reference's scalar arithmetic two lanes at a time (round 6:
// one packed instruction issues in 4.7-4.8 cycles against 2.5-2.7 for each
// of the two scalar ones, profiles/r02/rates/).
typedef float f2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2v pk_fma(f2v a, f2v b, f2v c) {
  return __builtin_elementwise_fma(a, b, c);
}

// pixel += V_p * (c, s) for the 4 correlations, the reference's product form
// (gridder_reference.cpp:79; oracle cmul_b) then the two f32 adds:
//   re = fma(vr, c, -(vi * s)),  im = fma(vi, c, vr * s),
// with t = (vi, vr) * (-s, s) = (-(vi * s), vr * s) exactly (negation is
// exact), so re, im = fma((vr, vi), (c, c), t) in one packed FMA.
__device__ __forceinline__ void mac_ref(f2v (&a)[4], const float4 &va,
                                        const float4 &vb, float cs, float sn) {
  const f2v v[4] = {{va.x, va.y}, {va.z, va.w}, {vb.x, vb.y}, {vb.z, vb.w}};
  const f2v ns = {-sn, sn}, cc = {cs, cs};
#pragma unroll
  for (int q = 0; q < 4; ++q)
    a[q] = a[q] + pk_fma(v[q], cc, v[q].yx * ns);
}

// The same for a base pixel (phasor (c, s)) and its mirror (phasor (c, -s),
// exactly: the mirror phase is the negated base phase and sincosf is odd /
// even), sharing the products: the mirror's t is (vi * s, -(vr * s)) = -t
// exactly, so its re, im = fma((vr, vi), (c, c), -t) (the packed FMA's
// negate modifiers).
__device__ __forceinline__ void mac_ref_pair(f2v (&a)[4], f2v (&b)[4],
                                             const float4 &va,
                                             const float4 &vb, float cs,
                                             float sn) {
  const f2v v[4] = {{va.x, va.y}, {va.z, va.w}, {vb.x, vb.y}, {vb.z, vb.w}};
  const f2v ns = {-sn, sn}, cc = {cs, cs};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f2v t = v[q].yx * ns;
    a[q] = a[q] + pk_fma(v[q], cc, t);
    b[q] = b[q] + pk_fma(v[q], cc, -t);
  }
}

// Output pixel p: device.hpp's epilogue and correlation-planar store on the
// packed accumulators.
__device__ __forceinline__ void seq_store_pixel(
    const f2v (&a)[4], int p, int S, int npix, const SubgridSetup &g,
    int nr_stations, const float *__restrict__ spheroidal,
    const float2 *__restrict__ aterms, float2 *__restrict__ out) {
  float r[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    r[2 * q] = a[q].x;
    r[2 * q + 1] = a[q].y;
  }
  store_pixel(r, p, S, npix, g, nr_stations, spheroidal, aterms, out);
}

// Mirror pairs need an even S and w = 0 on every timestep and in the offset
// of the subgrid (as the MFMA kernels).  A barrier: every lane of the
// workgroup calls it.  Not called by the VALU gridder (its block is
// blockDim.x), the degridder (its check avoids __syncthreads_or's LDS) and
// the MFMA gridder's prologue_scan (fused with the max scan).
__device__ __forceinline__ bool mirror_eligible(
    const SubgridSetup &g, int S,
    const idg::UVWCoordinate<float> *__restrict__ uvw, int tid) {
  bool w_nonzero = false;
  for (int t = tid; t < g.nr_timesteps; t += kSeqBlock)
    w_nonzero |= uvw[g.time_offset + t].w != 0.0f;
  return __syncthreads_or(w_nonzero) == 0 && S % 2 == 0 && g.w_offset == 0.0f;
}

// The pixel sums of the order-preserving gridders: NP base pixels of this
// lane (base[i] < nbase; clamped duplicates are computed and not stored) and,
// with MIRROR, their mirrors npix-1-base[i], each summed over t then c as
// the reference sums it.  The two gridders share this body and differ in the
// Phasor policy alone:
//   phasor(ph, &sn, &cs)                          sin / cos of the phase ph;
//   phasor.mirror(phm, neg, sn, cs, &snm, &csm)   the same for the mirror's
//     phase phm: the conjugate of (sn, cs) on lanes where neg (phm is the
//     bitwise negation of ph), the mirror's own phasor elsewhere.
template <int NP, bool MIRROR, typename Phasor>
__device__ __forceinline__ void order_grid_pixels(
    const int (&base)[NP], int nbase, int S, int npix, float image_size,
    const SubgridSetup &g, int C, int nr_stations,
    const idg::UVWCoordinate<float> *__restrict__ uvw,
    const float *__restrict__ wavenumbers,
    const float2 *__restrict__ visibilities,
    const float *__restrict__ spheroidal, const float2 *__restrict__ aterms,
    float2 *__restrict__ out, float4 *__restrict__ st_vis,
    float4 *__restrict__ st_uvwk, const Phasor &phasor) {
  constexpr int NQ = MIRROR ? 2 * NP : NP;
  float l[NQ], m[NQ], n[NQ], po[NQ];
  f2v acc[NQ][4];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int b = min(base[i % NP], nbase - 1);
    const int p = i < NP ? b : npix - 1 - b;
    pixel_geometry<true>(p, S, image_size, g, l[i], m[i], n[i], po[i]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f2v{0.0f, 0.0f};
  }
  // The visibilities come through LDS, kSeqStage (t, c) items at a time,
  // in the reference's t-then-c order: the workgroup stages a block (both
  // correlation quads of each item and its (u, v, w, k)) between two
  // barriers, and every wave walks it.  Loaded per wave from global memory
  // instead (wave-uniform scalar loads), each channel waited on its loads
  // at the top of the loop -- the lgkm counter they share with the LDS
  // reads of the sincosf windows makes every window wait a wait for them
  // too (the sequential gridder issued at 0.90 of its instruction stream,
  // round 6).
  const long long items = static_cast<long long>(g.nr_timesteps) * C;
  const float4 *vis4 = reinterpret_cast<const float4 *>(visibilities) +
                       g.time_offset * C * 2;
  float pidx[NQ];
  for (long long i0 = 0; i0 < items; i0 += kSeqStage) {
    const int ne = static_cast<int>(items - i0 < kSeqStage ? items - i0 : kSeqStage);
    __syncthreads();  // the previous block's readers are done
    for (int e = threadIdx.x; e < ne; e += kSeqBlock) {
      const long long it = i0 + e;
      const int t = static_cast<int>(it / C), c = static_cast<int>(it % C);
      st_vis[2 * e] = vis4[it * 2];
      st_vis[2 * e + 1] = vis4[it * 2 + 1];
      const idg::UVWCoordinate<float> c3 = uvw[g.time_offset + t];
      st_uvwk[e] = make_float4(c3.u, c3.v, c3.w, wavenumbers[c]);
    }
    __syncthreads();
    int ch = static_cast<int>(i0 % C);
    for (int e = 0; e < ne; ++e) {
      const float4 uvwk = st_uvwk[e];
      const float4 va = st_vis[2 * e], vb = st_vis[2 * e + 1];
      if (ch == 0 || e == 0) {  // a new timestep (or block): phase_index
#pragma unroll
        for (int i = 0; i < NQ; ++i)
          pidx[i] = fma_(uvwk.z, n[i], fma_(uvwk.x, l[i], uvwk.y * m[i]));
      }
      ch = ch + 1 == C ? 0 : ch + 1;
      const float k = uvwk.w;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const float ph = fma_(-pidx[i], k, po[i]);
        float sn, cs;
        phasor(ph, &sn, &cs);
        if constexpr (MIRROR) {
          // the mirror's own phase, formed as the reference forms it; where
          // it is the exact negation (every lane of every wave on the
          // benchmark data) its phasor is the conjugate, and one set of
          // products serves both pixels
          const float phm = fma_(-pidx[NP + i], k, po[NP + i]);
          const bool neg = fbits(phm) == (fbits(ph) ^ 0x80000000u);
          if (__all(neg)) {
            mac_ref_pair(acc[i], acc[NP + i], va, vb, cs, sn);
          } else {
            float snm, csm;
            phasor.mirror(phm, neg, sn, cs, &snm, &csm);
            mac_ref(acc[i], va, vb, cs, sn);
            mac_ref(acc[NP + i], va, vb, csm, snm);
          }
        } else {
          mac_ref(acc[i], va, vb, cs, sn);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    if (base[i % NP] >= nbase) continue;
    const int p = i < NP ? base[i] : npix - 1 - base[i - NP];
    seq_store_pixel(acc[i], p, S, npix, g, nr_stations, spheroidal, aterms,
                    out);
  }
}

}  // namespace

}  // namespace idg_mi355x
