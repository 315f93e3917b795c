// multiscale.hpp -- the arithmetic of multi-scale CLEAN: one
// tap of the separable convolution, the order of peaks over the scale planes,
// one iteration's component, what it adds to a model pixel and where the
// cross-PSF of two scales is stored.  Shared by the host twin
// (host/multiscale.cpp) and the device kernels
// (hip/kernels/multiscale_mi355x.hip.cpp), whose outputs are bit for bit the
// same; the minor cycle's loop is the one both CLEANs share
// (host/minor_cycle.hpp, hip/kernels/minor_cycle.hpp).  The key's magnitude bits, the stop decision, the patch and the
// subtraction of one pixel are those of common/clean.hpp, used from there:
// with one scale of weight 1 an iteration is a Hogbom iteration.
#pragma once

#include <cmath>
#include <cstdint>

#include "common/clean.hpp"

namespace idg_mi355x {
namespace ms {

constexpr int kMaxGridSize = clean::kMaxGridSize;
constexpr int kMaxRadius = 48;  // a scale's taps: at most 97 floats
constexpr int kMaxScales = 8;   // a scale index fits the key's 3 bits

// idg_ms_params_t without its struct_size: `base` holds the fields it shares
// with idg_clean_params_t.
struct Params {
  clean::Params base;
  int nr_scales;
  int radius[kMaxScales];
  float weight[kMaxScales];
  float inv_peak[kMaxScales];
};

// idg_ms_component_t and idg_ms_state_t (include/idg_mi355x.h).
struct Component {
  int32_t y, x, scale;
  float value;
};
struct State {
  clean::State s;
  int32_t peak_scale;
};

// One tap of a pass onto a pixel's accumulator (which starts at +0).
IDG_PLAN_HD inline float tap(float pixel, float h, float acc) {
  return fmaf(pixel, h, acc);
}

// Where scale s's taps start in the concatenated table.
IDG_PLAN_HD inline int taps_at(const Params &p, int s) {
  int at = 0;
  for (int j = 0; j < s; ++j) at += 2 * p.radius[j] + 1;
  return at;
}

// The patch of cross(s, q) = cross(q, s) among the Ns (Ns + 1) / 2 stored:
// row-major over s <= q.
IDG_PLAN_HD inline int cross_at(int nr_scales, int s, int q) {
  const int lo = s < q ? s : q, hi = s < q ? q : s;
  return lo * nr_scales - lo * (lo - 1) / 2 + (hi - lo);
}

// What the search compares at a pixel of plane s holding v.
IDG_PLAN_HD inline float weighted(const Params &p, int s, float v) {
  return p.weight[s] * v;
}

// The key of pixel `index` of plane s whose weighted value is u: the bits of
// |u| above ~((s << 28) | index), so that an integer max over keys finds the
// largest |u| and, among equals, the lowest scale, then the lowest index.  0
// for a NaN u (a NaN v makes one) or an unsearchable pixel; no pixel's key is
// 0 (index < 2^28 and s < 8: the low word's complement has bit 31 set).
IDG_PLAN_HD inline uint64_t key_of(float u, int s, uint32_t index,
                                   bool searchable) {
  const uint32_t mag = clean::bits_of(u) & 0x7fffffffu;
  if (!searchable || mag > 0x7f800000u) return 0;
  const uint32_t low = (static_cast<uint32_t>(s) << 28) | index;
  return (static_cast<uint64_t>(mag) << 32) | static_cast<uint32_t>(~low);
}
IDG_PLAN_HD inline int scale_of(uint64_t key) {
  return static_cast<int>((~static_cast<uint32_t>(key)) >> 28);
}
IDG_PLAN_HD inline uint32_t index_of(uint64_t key) {
  return (~static_cast<uint32_t>(key)) & 0x0fffffffu;
}

// state.peak, peak_index and peak_scale of planes whose peak has this key.
IDG_PLAN_HD inline void set_peak(State *st, uint64_t key) {
  st->s.peak = key != 0 ? clean::magnitude_of(key) : 0.0f;
  st->s.peak_index = key != 0 ? static_cast<int32_t>(index_of(key)) : -1;
  st->peak_scale = key != 0 ? scale_of(key) : -1;
}

// Steps 1-6 of one iteration but the write of the record: the peak's key and
// the signed value v of its pixel in, the state advanced by clean::step on
// the weighted value.  True when a component c = (gain * v) * inv_peak[s] is
// taken (n_components already counts it).
IDG_PLAN_HD inline bool step(State *st, const Params &p, uint64_t key, float v,
                             float *c) {
  const int s = key != 0 ? scale_of(key) : 0;
  float unused = 0.0f;
  if (!clean::step(&st->s, p.base, key, weighted(p, s, v), &unused))
    return false;
  const float gv = p.base.gain * v;
  *c = gv * p.inv_peak[s];
  return true;
}

// Step 7 at one pixel of the footprint: hy and hx are the scale's taps at the
// pixel's row and column offsets.
IDG_PLAN_HD inline float model_add(float c, float hy, float hx, float model) {
  const float a = c * hy;
  const float b = a * hx;
  return model + b;
}

// Multi-scale CLEAN as the policy of the one minor-cycle body (clean::Cycle,
// common/clean.hpp, names the members): nr_scales planes, the key carries the
// scale, and a component of scale s subtracts cross(s, q) from plane q.
struct Cycle {
  using Params = ms::Params;
  using State = ms::State;
  using Component = ms::Component;
  IDG_PLAN_HD static const clean::Params &base(const Params &p) {
    return p.base;
  }
  IDG_PLAN_HD static const clean::State &base(const State &st) { return st.s; }
  IDG_PLAN_HD static int planes(const Params &p) { return p.nr_scales; }
  IDG_PLAN_HD static uint64_t key_of(const Params &p, int q, float v,
                                     uint32_t index, bool searchable) {
    return ms::key_of(weighted(p, q, v), q, index, searchable);
  }
  IDG_PLAN_HD static int scale_of(uint64_t key) { return ms::scale_of(key); }
  IDG_PLAN_HD static uint32_t index_of(uint64_t key) {
    return ms::index_of(key);
  }
  IDG_PLAN_HD static bool step(State *st, const Params &p, uint64_t key,
                               float v, float *c) {
    return ms::step(st, p, key, v, c);
  }
  IDG_PLAN_HD static void set_peak(State *st, uint64_t key) {
    ms::set_peak(st, key);
  }
  IDG_PLAN_HD static size_t psf_at(const Params &p, int s, int q) {
    const size_t Gp = static_cast<size_t>(p.base.psf_size);
    return cross_at(p.nr_scales, s, q) * (Gp * Gp);
  }
  IDG_PLAN_HD static Component record(int y, int x, int s, float c) {
    return {y, x, s, c};
  }
};

}  // namespace ms
}  // namespace idg_mi355x
