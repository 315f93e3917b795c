// weight.hpp -- the imaging-weight arithmetic: the uv cell of
// a sample, its quantised weight q, the density D at a cell and the imaging
// weight f = w / (a + b D).  Shared by the host twins (host::weight_density,
// weight_scheme, weight_apply; host/weight.cpp) and the device
// kernels (hip/kernels/weight_mi355x.hip.cpp), whose outputs are bit for bit
// the same: every float operation below is one rounded float32 operation (the
// library is built -ffp-contract=off), the density is a sum of integers.
#pragma once

#include <cmath>
#include <cstdint>

#include "common/plan.hpp"

namespace idg_mi355x {
namespace weight {

constexpr float kScaledLimit = 1099511627776.0f;  // 2^40: scaled weights below
constexpr uint64_t kCellLimit = 1ull << 62;        // a cell's sum of q below
constexpr int kQuantumLog2Min = -64, kQuantumLog2Max = 64;

constexpr int kNatural = 0, kUniform = 1, kBriggs = 2;

// The caller's parameters; cells = image_size * kInv2Pi, so that a channel's
// uv cells per metre are wavenumber * cells (plan::set_scales, per channel).
struct Geometry {
  int grid_size;
  int quantum_log2;
  int hermitian;
  float cells;
};

IDG_PLAN_HD inline float cells_of(float image_size) {
  return image_size * plan::kInv2Pi;
}

// The nearest integer-centred cell of (u, v) at `scale` cells per metre;
// false when it is not finite or lies outside [0, G)^2.
IDG_PLAN_HD inline bool cell_of(const Geometry &g, float u, float v,
                                float scale, int *x, int *y) {
  const int half = g.grid_size / 2;
  if (!plan::cell_of(u * scale + 0.5f, half, x) ||
      !plan::cell_of(v * scale + 0.5f, half, y))
    return false;
  return *x >= 0 && *x < g.grid_size && *y >= 0 && *y < g.grid_size;
}

// rintf(w * 2^-quantum_log2) for a finite w > 0 whose scaled value is below
// 2^40, else 0 (a flag).
IDG_PLAN_HD inline uint64_t quantise(float w, int quantum_log2) {
  if (!(plan::is_finite(w) && w > 0.0f)) return 0;
  const float scaled = ldexpf(w, -quantum_log2);
  if (!(scaled < kScaledLimit)) return 0;
  return static_cast<uint64_t>(rintf(scaled));
}

// The sum of q behind D at cell (x, y): the cell's own and, with `hermitian`,
// that of the mirror cell (G - x, G - y) where it lies inside the grid.
IDG_PLAN_HD inline uint64_t count_at(const Geometry &g,
                                     const uint64_t *density, int x, int y) {
  const size_t G = static_cast<size_t>(g.grid_size);
  uint64_t n = density[static_cast<size_t>(y) * G + x];
  if (g.hermitian && x > 0 && y > 0)
    n += density[(G - y) * G + (G - x)];
  return n;
}

// D = (float)n * 2^quantum_log2: the conversion is the one rounding.
IDG_PLAN_HD inline float density_of(uint64_t n, int quantum_log2) {
  return ldexpf(static_cast<float>(n), quantum_log2);
}

// f = w / (a + b D): one multiply, one add, one correctly rounded divide.
IDG_PLAN_HD inline float imaging_weight(float w, float a, float b, float D) {
  const float bd = b * D;
  const float den = a + bd;
  return w / den;
}

// Everything the density and the apply step need of one sample: q (0 = the
// sample is flagged or off the grid) and its cell.
IDG_PLAN_HD inline uint64_t sample(const Geometry &g, float u, float v,
                                   float wavenumber, float w, int *x,
                                   int *y) {
  const uint64_t q = quantise(w, g.quantum_log2);
  if (q == 0) return 0;
  return cell_of(g, u, v, wavenumber * g.cells, x, y) ? q : 0;
}

// (a, b) of a scheme from the sums over all cells of D and D^2 (doubles);
// briggs_scale = (5 * 10^-robust)^2, computed once on the host.
IDG_PLAN_HD inline void scheme_ab(int scheme, double briggs_scale,
                                  double sum_d, double sum_d2, float *a,
                                  float *b) {
  if (scheme == kUniform) {
    *a = 0.0f;
    *b = 1.0f;
  } else if (scheme == kBriggs) {
    *a = 1.0f;
    *b = sum_d2 > 0.0 ? static_cast<float>(briggs_scale * sum_d / sum_d2)
                      : 0.0f;
  } else {
    *a = 1.0f;
    *b = 0.0f;
  }
}

}  // namespace weight
}  // namespace idg_mi355x
