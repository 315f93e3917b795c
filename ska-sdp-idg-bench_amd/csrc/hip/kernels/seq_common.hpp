// seq_common.hpp -- what the kernels that keep the reference's summation
// order share: the reference's complex multiply-accumulate, pixel geometry
// and output epilogue, restated for gfx950.  Included by
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

// Output pixel p: sph * (A1^H P A2) with the reference's forms (common/
// math.hpp apply_aterm_gridder), correlation-planar store.
__device__ __forceinline__ void seq_store_pixel(
    const f2v (&a)[4], int p, int S, int npix, const SubgridSetup &g,
    int nr_stations, const float *__restrict__ spheroidal,
    const float2 *__restrict__ aterms, float2 *__restrict__ out) {
  const int y = p / S, x = p - y * S;
  idg::cfloat pix[4], a1[4], a2[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) pix[q] = {a[q].x, a[q].y};
  load_jones(aterm_ptr(aterms, nr_stations, S, g.aterm_index, g.station1, y,
                       x), a1);
  load_jones(aterm_ptr(aterms, nr_stations, S, g.aterm_index, g.station2, y,
                       x), a2);
  idg::apply_aterm_gridder(pix, a1, a2);
  const float sph = spheroidal[p];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    out[static_cast<size_t>(q) * npix + p] =
        make_float2(pix[q].re * sph, pix[q].im * sph);
}

// Pixel geometry as the reference gridder forms it (gridder_reference.cpp:
// 49-64): l, m via double, n = compute_n, phase_offset = fma(w_o, n,
// fma(u_o, l, v_o*m)) -- with n on mirror subgrids too (w_offset = 0 there,
// but fma(0, n, x) is formed exactly as the reference forms it).
__device__ __forceinline__ void seq_geometry(int p, int S, float image_size,
                                             const SubgridSetup &g, float &l,
                                             float &m, float &n, float &poff) {
  const int y = p / S, x = p - y * S;
  l = idg::compute_l(x, S, image_size);
  m = idg::compute_m(y, S, image_size);
  n = idg::compute_n(l, m);
  poff = fma_(g.w_offset, n, fma_(g.u_offset, l, g.v_offset * m));
}

}  // namespace

}  // namespace idg_mi355x
