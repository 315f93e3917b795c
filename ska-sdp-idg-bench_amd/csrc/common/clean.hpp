// clean.hpp -- the arithmetic of the Hogbom minor cycle: the
// order of peaks, the stop decision of one iteration and the subtraction of
// one pixel.  Shared by the host twin (host::clean; host/clean.cpp over
// host/minor_cycle.hpp) and the device kernels
// (hip/kernels/clean_mi355x.hip.cpp over hip/kernels/minor_cycle.hpp), whose
// outputs are bit for bit the same: every float operation below is one
// rounded float32 operation (the library is built -ffp-contract=off), the one
// fused operation is an explicit fmaf, and the peak is an integer max, exact
// in any order.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "common/plan.hpp"

namespace idg_mi355x {
namespace clean {

constexpr int kMaxGridSize = 16384;  // G^2 <= 2^28: a pixel index fits 32 bits

// state.reason
constexpr int kRunning = 0, kBelowLevel = 1, kNoPeak = 2, kComponentsFull = 3;

// idg_clean_params_t without its struct_size.
struct Params {
  int grid_size;
  int psf_size;
  int max_components;
  int nr_iterations;
  float gain;
  float threshold;
  float cycle_fraction;
};

// idg_clean_component_t and idg_clean_state_t (include/idg_mi355x.h).
struct Component {
  int32_t y, x;
  float value;
};
struct State {
  int32_t n_components;
  int32_t reason;
  int32_t started;
  int32_t peak_index;
  float level;
  float peak;
};

IDG_PLAN_HD inline uint32_t bits_of(float s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(s);
#else
  uint32_t b;
  std::memcpy(&b, &s, sizeof b);
  return b;
#endif
}

IDG_PLAN_HD inline float float_of(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float s;
  std::memcpy(&s, &b, sizeof s);
  return s;
#endif
}

// The key of pixel `index` holding s: the bits of |s| above ~index, so that an
// integer max over keys finds the largest |s| and, among equals (+v and -v
// too), the lowest index.  0 for a NaN or an unsearchable pixel: no pixel's
// key is 0 (index < 2^28, so ~index != 0), 0 is "no peak".
IDG_PLAN_HD inline uint64_t key_of(float s, uint32_t index, bool searchable) {
  const uint32_t mag = bits_of(s) & 0x7fffffffu;
  if (!searchable || mag > 0x7f800000u) return 0;
  return (static_cast<uint64_t>(mag) << 32) | static_cast<uint32_t>(~index);
}

// key != 0: the pixel's linear index and its |s|.
IDG_PLAN_HD inline uint32_t index_of(uint64_t key) {
  return ~static_cast<uint32_t>(key);
}
IDG_PLAN_HD inline float magnitude_of(uint64_t key) {
  return float_of(static_cast<uint32_t>(key >> 32));
}

// state.peak and state.peak_index of a residual whose peak has this key.
IDG_PLAN_HD inline void set_peak(State *s, uint64_t key) {
  s->peak = key != 0 ? magnitude_of(key) : 0.0f;
  s->peak_index = key != 0 ? static_cast<int32_t>(index_of(key)) : -1;
}

// A state no iteration may run from: the host entry refuses it, the device
// entry (which reads nothing back) runs no iteration on it.
IDG_PLAN_HD inline bool state_ok(const State &s, const Params &p) {
  return s.n_components >= 0 && s.n_components <= p.max_components;
}

// Steps 1-6 of one iteration but the writes to components and model: the
// peak's key and signed value v in, the state advanced.  True when a
// component c = gain * v is taken (n_components already counts it): the
// caller records it and subtracts c * psf.
IDG_PLAN_HD inline bool step(State *s, const Params &p, uint64_t key, float v,
                             float *c) {
  if (s->reason != kRunning || !state_ok(*s, p)) return false;
  if (key == 0) {
    s->reason = kNoPeak;
    return false;
  }
  const float a = fabsf(v);
  if (s->started == 0) {
    const float part = p.cycle_fraction * a;
    s->level = fmaxf(p.threshold, part);
    s->started = 1;
  }
  if (!(a > s->level)) {
    s->reason = kBelowLevel;
    return false;
  }
  if (s->n_components == p.max_components) {
    s->reason = kComponentsFull;
    return false;
  }
  *c = p.gain * v;
  s->n_components += 1;
  return true;
}

// Step 7 at one pixel of the patch.
IDG_PLAN_HD inline float subtract(float c, float psf, float residual) {
  return fmaf(-c, psf, residual);
}

// The patch of a component at (py, px): rows [y0, y1) and columns [x0, x1) of
// the image, row y reading psf row y - oy (columns alike).
struct Patch {
  int y0, y1, x0, x1, oy, ox;
};
IDG_PLAN_HD inline Patch patch_of(const Params &p, int py, int px) {
  Patch t;
  t.oy = py - p.psf_size / 2;
  t.ox = px - p.psf_size / 2;
  t.y0 = t.oy > 0 ? t.oy : 0;
  t.x0 = t.ox > 0 ? t.ox : 0;
  t.y1 = t.oy + p.psf_size < p.grid_size ? t.oy + p.psf_size : p.grid_size;
  t.x1 = t.ox + p.psf_size < p.grid_size ? t.ox + p.psf_size : p.grid_size;
  return t;
}

// The Hogbom cycle as the policy of the one minor-cycle body (host:
// host/minor_cycle.hpp; device: hip/kernels/minor_cycle.hpp): what a cycle's
// records are and which of the functions above it calls.  One plane and one
// PSF patch, both known at compile time, so the body's loop over the planes
// folds away.  ms::Cycle (common/multiscale.hpp) is the other policy.
struct Cycle {
  using Params = clean::Params;
  using State = clean::State;
  using Component = clean::Component;
  // the clean::Params / clean::State inside the cycle's own
  IDG_PLAN_HD static const clean::Params &base(const Params &p) { return p; }
  IDG_PLAN_HD static const clean::State &base(const State &s) { return s; }
  IDG_PLAN_HD static constexpr int planes(const Params &) { return 1; }
  // the key of pixel `index` of plane q holding v; its plane and its index
  IDG_PLAN_HD static uint64_t key_of(const Params &, int, float v,
                                     uint32_t index, bool searchable) {
    return clean::key_of(v, index, searchable);
  }
  IDG_PLAN_HD static constexpr int scale_of(uint64_t) { return 0; }
  IDG_PLAN_HD static uint32_t index_of(uint64_t key) {
    return clean::index_of(key);
  }
  IDG_PLAN_HD static bool step(State *s, const Params &p, uint64_t key,
                               float v, float *c) {
    return clean::step(s, p, key, v, c);
  }
  IDG_PLAN_HD static void set_peak(State *s, uint64_t key) {
    clean::set_peak(s, key);
  }
  // where the patch that a component of scale s subtracts from plane q
  // starts, in floats from the PSF buffer's first
  IDG_PLAN_HD static constexpr size_t psf_at(const Params &, int, int) {
    return 0;
  }
  IDG_PLAN_HD static Component record(int y, int x, int, float c) {
    return {y, x, c};
  }
};

}  // namespace clean
}  // namespace idg_mi355x
