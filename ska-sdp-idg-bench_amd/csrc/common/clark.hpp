// clark.hpp -- the arithmetic of Clark CLEAN beyond the Hogbom
// minor cycle's (common/clean.hpp, used as it is): the bin of a pixel in the
// magnitude histogram, the limit of a round's candidate list and the test
// that keeps a round going.  Shared by the host twin (host/clark.cpp) and the
// device kernels (hip/kernels/clark_mi355x.hip.cpp), whose outputs are bit
// for bit the same: the limit is integer arithmetic on float bits but for one
// rounded multiply and one fmaxf, the histogram holds integer counts, exact
// in any order, and the list is a set whose order nothing visible depends on.
#pragma once

#include <cstdint>

#include "common/clean.hpp"

namespace idg_mi355x {
namespace clark {

constexpr int kMaxCandidates = 16384;
// the exponent and four mantissa bits of |s|
constexpr int kBinShift = 19;
constexpr int kBins = 4096;

// state.reason beyond clean::k*
constexpr int kNoCandidate = 4;

// idg_clark_params_t without its struct_size (base.nr_iterations is unused).
struct Params {
  clean::Params base;
  int nr_rounds;
  int iterations_per_round;
  int max_candidates;
  float select_fraction;
};

// idg_clark_state_t.
struct State {
  clean::State base;
  int32_t n_candidates;
  float round_limit;
  int32_t rounds;
};

IDG_PLAN_HD inline uint32_t magnitude_bits(float s) {
  return clean::bits_of(s) & 0x7fffffffu;
}

IDG_PLAN_HD inline uint32_t bin_of(float s) {
  return magnitude_bits(s) >> kBinShift;
}

// Step 1 of a round but the search: the residual's peak (key, signed value v)
// in, the state advanced.  True when the round goes on to its limit.
IDG_PLAN_HD inline bool begin_round(State *s, const Params &p, uint64_t key,
                                    float v) {
  s->rounds += 1;
  if (key == 0) {
    s->base.reason = clean::kNoPeak;
    return false;
  }
  const float a = fabsf(v);
  if (s->base.started == 0) {
    const float part = p.base.cycle_fraction * a;
    s->base.level = fmaxf(p.base.threshold, part);
    s->base.started = 1;
  }
  if (!(a > s->base.level)) {
    s->base.reason = clean::kBelowLevel;
    return false;
  }
  return true;
}

// The magnitude bits from which a pixel is a candidate.  bins_over: the number
// of bins b whose suffix count -- the searchable, non-NaN pixels in the bins
// >= b -- exceeds max_candidates; bins_occupied: the number whose suffix count
// is not 0.  The suffix does not grow with b, so bins_over is the least bin
// whose suffix fits; where nothing is left at or above that bin -- even the
// top occupied bin overflows -- the limit is kBins, above every pixel.  Whole
// bins below bin_of(level) never decide: where the suffix of bin_of(level)
// fits, the least bin that fits lies at or below it and the other argument of
// the max is above that; where it does not, every lower bin's suffix does not
// either, counted or not; and the peak's bin is not below the level's.  So a
// histogram that leaves out the bins below bin_of(level) -- whole bins, the
// level's own bin counted in full -- gives the same bits.
IDG_PLAN_HD inline uint32_t limit_bits(float level, float select_fraction,
                                       float peak, uint32_t bins_over,
                                       uint32_t bins_occupied) {
  const float part = select_fraction * fabsf(peak);
  const float f = fmaxf(level, part);
  const uint32_t least = bins_over == bins_occupied ? kBins : bins_over;
  const uint32_t by_count = least << kBinShift;
  const uint32_t by_level = clean::bits_of(f) + 1;
  return by_level > by_count ? by_level : by_count;
}

// A pixel holding s is a candidate of a round with these limit bits.
IDG_PLAN_HD inline bool is_candidate(float s, bool searchable,
                                     uint32_t tbits) {
  const uint32_t mag = magnitude_bits(s);
  return searchable && mag <= 0x7f800000u && mag >= tbits;
}

// The list's peak keeps the round going.
IDG_PLAN_HD inline bool in_round(uint64_t key, uint32_t tbits) {
  return key != 0 && static_cast<uint32_t>(key >> 32) >= tbits;
}

}  // namespace clark
}  // namespace idg_mi355x
