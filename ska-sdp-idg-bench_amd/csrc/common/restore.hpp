// restore.hpp -- the arithmetic of the restore step: which
// model pixels count, what one of them adds to an output pixel, and the final
// add of the residual.  Shared by the host twin (host::restore;
// host/restore.cpp) and the device kernel
// (hip/kernels/restore_mi355x.hip.cpp), whose outputs are bit for bit the
// same: the library is built -ffp-contract=off, the one fused operation is an
// explicit fmaf, and both sides add a pixel's contributions in the row-major
// order of their sources.
#pragma once

#include <cmath>
#include <cstdint>

#include "common/plan.hpp"

namespace idg_mi355x {
namespace restore {

constexpr int kMaxGridSize = 16384;
constexpr int kMaxRadius = 32;  // the taps: at most 65 x 65 floats

// idg_restore_params_t without its struct_size.
struct Params {
  int grid_size;
  int radius;
};

// A model pixel that contributes: anything but +0 and -0 (a NaN does).  The
// skip is part of the contract: with it the bytes do not depend on whether an
// implementation visits the zero pixels, whatever the taps hold.
IDG_PLAN_HD inline bool taken(float m) { return !(m == 0.0f); }

// One source onto one output pixel's accumulator (which starts at +0).
IDG_PLAN_HD inline float accumulate(float m, float tap, float acc) {
  return fmaf(m, tap, acc);
}

// The output pixel: one rounded add (without a residual, 0 + acc).
IDG_PLAN_HD inline float finish(bool has_residual, float residual, float acc) {
  return (has_residual ? residual : 0.0f) + acc;
}

}  // namespace restore
}  // namespace idg_mi355x
