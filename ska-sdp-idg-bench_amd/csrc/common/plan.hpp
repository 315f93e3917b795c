// plan.hpp -- the plan step's arithmetic: uvw rows of one
// baseline -> subgrids (row range, A-term slot, w layer, corner).  Shared by
// the host twin (host::plan, host/plan.cpp) and the device kernels
// (hip/kernels/plan_mi355x.hip.cpp), whose outputs are bit for bit the same:
// every float operation below is one rounded float32 operation (the library
// is built -ffp-contract=off), there is no division, and everything after the
// floorf is integer arithmetic.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define IDG_PLAN_HD __host__ __device__
#else
#define IDG_PLAN_HD
#endif

namespace idg_mi355x {
namespace plan {

constexpr float kInv2Pi = static_cast<float>(0.15915494309189535);  // 1/(2 pi)
constexpr float kCellLimit = 1073741824.0f;  // 2^30: |floored product| below
constexpr float kFloatMax = 3.402823466e+38f;

// The caller's parameters plus the three scales derived from them.
struct Geometry {
  int grid_size;
  int subgrid_size;
  int kernel_size;    // uv cells kept free at the subgrid's edge
  int max_timesteps;  // per subgrid, >= 1
  int aterm_steps;    // timesteps per A-term slot, 0 = one slot
  int nr_w_layers;
  int use_w;          // w_step_in_lambda != 0
  float s0, s1;       // uv cells per metre at the first / last channel
  float ws;           // w layers per metre at the mean wavenumber
};

// wn0 / wn1: the first and last wavenumber; inv_w_step = 1.0f / w_step,
// computed once on the host (unused when use_w == 0).
IDG_PLAN_HD inline void set_scales(Geometry *g, float image_size, float wn0,
                                   float wn1, float inv_w_step) {
  const float cells = image_size * kInv2Pi;
  g->s0 = wn0 * cells;
  g->s1 = wn1 * cells;
  g->ws = g->use_w ? ((0.5f * (wn0 + wn1)) * kInv2Pi) * inv_w_step : 0.0f;
}

// uv cells [x0, x1] x [y0, y1], inclusive.
struct Box {
  int x0, x1, y0, y1;
};

IDG_PLAN_HD inline Box empty_box() {
  return Box{INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN};
}

IDG_PLAN_HD inline Box merge(const Box &a, const Box &b) {
  return Box{a.x0 < b.x0 ? a.x0 : b.x0, a.x1 > b.x1 ? a.x1 : b.x1,
             a.y0 < b.y0 ? a.y0 : b.y0, a.y1 > b.y1 ? a.y1 : b.y1};
}

IDG_PLAN_HD inline bool is_finite(float x) { return fabsf(x) <= kFloatMax; }

// The cell of a product `p` (one rounded multiply): false when floorf(p) is
// NaN or its magnitude is >= 2^30.
IDG_PLAN_HD inline bool cell_of(float p, int half, int *cell) {
  p = floorf(p);
  if (!(fabsf(p) < kCellLimit)) return false;
  *cell = static_cast<int>(p) + half;
  return true;
}

// Whether a subgrid can hold `b` with kernel_size cells to spare, centred,
// wholly inside the grid (the adder skips any other); its corner if so.
IDG_PLAN_HD inline bool place(const Geometry &g, const Box &b, int *x,
                              int *y) {
  const int S = g.subgrid_size;
  const long long wx = static_cast<long long>(b.x1) - b.x0 + 1;
  const long long wy = static_cast<long long>(b.y1) - b.y0 + 1;
  const long long room = S - g.kernel_size;
  if (wx < 1 || wy < 1 || wx > room || wy > room) return false;
  const int cx = b.x0 - (S - static_cast<int>(wx)) / 2;
  const int cy = b.y0 - (S - static_cast<int>(wy)) / 2;
  if (cx < 0 || cx > g.grid_size - S || cy < 0 || cy > g.grid_size - S)
    return false;
  *x = cx;
  *y = cy;
  return true;
}

// floorf(w * ws) clamped into [0, nr_w_layers - 1] as a float, then
// converted; 0 without w layers.  Negative w lands in layer 0.
IDG_PLAN_HD inline int layer_of(const Geometry &g, float w) {
  if (!g.use_w) return 0;
  float l = floorf(w * g.ws);
  const float top = static_cast<float>(g.nr_w_layers - 1);
  if (!(l > 0.0f)) l = 0.0f;
  if (l > top) l = top;
  return static_cast<int>(l);
}

// One timestep: its box over the first and last channel and its layer;
// invalid when a coordinate is not finite, a cell is out of range, or its
// own box does not fit.
struct Step {
  Box box;
  int layer;
  bool valid;
};

IDG_PLAN_HD inline Step eval_step(const Geometry &g, float u, float v,
                                  float w) {
  Step s;
  s.box = empty_box();
  s.layer = 0;
  s.valid = false;
  if (!(is_finite(u) && is_finite(v) && is_finite(w))) return s;
  const int half = g.grid_size / 2;
  int xa, xb, ya, yb;
  if (!cell_of(u * g.s0, half, &xa) || !cell_of(u * g.s1, half, &xb) ||
      !cell_of(v * g.s0, half, &ya) || !cell_of(v * g.s1, half, &yb))
    return s;
  const Box b{xa < xb ? xa : xb, xa > xb ? xa : xb, ya < yb ? ya : yb,
              ya > yb ? ya : yb};
  int x, y;
  if (!place(g, b, &x, &y)) return s;
  s.box = b;
  s.layer = layer_of(g, w);
  s.valid = true;
  return s;
}

IDG_PLAN_HD inline int slot_of(const Geometry &g, int t) {
  return g.aterm_steps > 0 ? t / g.aterm_steps : 0;
}

// A closed subgrid as the 9 words of an idg::Metadata record.
IDG_PLAN_HD inline void record_words(const Geometry &g, int row0, int n,
                                     int slot, int layer, uint32_t station1,
                                     uint32_t station2, const Box &box,
                                     int32_t words[9]) {
  int x = 0, y = 0;
  place(g, box, &x, &y);
  words[0] = 0;     // baseline_offset
  words[1] = row0;  // time_offset, as a row: bl * T + t0
  words[2] = n;
  words[3] = slot;
  words[4] = static_cast<int32_t>(station1);
  words[5] = static_cast<int32_t>(station2);
  words[6] = x;
  words[7] = y;
  words[8] = layer;
}

// The greedy walk over one baseline's T rows (uvw: that baseline's first
// row), t ascending, at most one open subgrid: emit(words) per closed
// subgrid, in t0 order; returns the dropped (invalid) timesteps.  The device
// kernel computes the same closures 64 candidates at a time.
template <typename Emit>
inline int walk_baseline(const Geometry &g, const float *uvw, int row0, int T,
                         uint32_t station1, uint32_t station2, Emit &&emit) {
  int dropped = 0, n = 0, t0 = 0, slot0 = 0, layer0 = 0;
  Box box = empty_box();
  int32_t words[9];
  const auto close = [&]() {
    if (n == 0) return;
    record_words(g, row0 + t0, n, slot0, layer0, station1, station2, box,
                 words);
    emit(words);
    n = 0;
  };
  for (int t = 0; t < T; ++t) {
    const float *r = uvw + static_cast<size_t>(t) * 3;
    const Step s = eval_step(g, r[0], r[1], r[2]);
    if (!s.valid) {
      close();
      ++dropped;
      continue;
    }
    const int slot = slot_of(g, t);
    if (n > 0) {
      const Box m = merge(box, s.box);
      int x, y;
      if (n < g.max_timesteps && slot == slot0 && s.layer == layer0 &&
          place(g, m, &x, &y)) {
        box = m;
        ++n;
        continue;
      }
      close();
    }
    t0 = t;
    slot0 = slot;
    layer0 = s.layer;
    box = s.box;
    n = 1;
  }
  close();
  return dropped;
}

}  // namespace plan
}  // namespace idg_mi355x
