// clark.cpp -- the host twin of Clark CLEAN (host.hpp): rounds
// of peak, limit, candidate list, minor cycle on the list and apply, over the
// arithmetic of common/clark.hpp and common/clean.hpp.
#include <algorithm>
#include <vector>

#include "host/host.hpp"

namespace idg_mi355x {
namespace host {

namespace {

struct Candidate {
  uint32_t index;
  float value;
};

// The key of the plane's peak (clean::key_of; 0: none).
uint64_t peak_key(const float *plane, const uint8_t *mask, size_t cells) {
  uint64_t key = 0;
  for (size_t i = 0; i < cells; ++i) {
    const uint64_t at = clean::key_of(plane[i], static_cast<uint32_t>(i),
                                      mask == nullptr || mask[i] != 0);
    if (at > key) key = at;
  }
  return key;
}

}  // namespace

std::string clark(const clark::Params &p, float *residual, const float *psf,
                  const uint8_t *mask, float *model,
                  clean::Component *components, clark::State *state) {
  clark::State st = *state;
  if (!clean::state_ok(st.base, p.base))
    return "idg_clark: state.n_components " +
           std::to_string(st.base.n_components) + " outside [0, " +
           std::to_string(p.base.max_components) + "]";
  const size_t G = static_cast<size_t>(p.base.grid_size);
  const size_t Gp = static_cast<size_t>(p.base.psf_size);
  const size_t cells = G * G;
  std::vector<uint32_t> hist(clark::kBins + 1);
  std::vector<Candidate> list;
  list.reserve(static_cast<size_t>(p.max_candidates));

  for (int r = 0; r < p.nr_rounds && st.base.reason == clean::kRunning; ++r) {
    // 1. the peak
    const uint64_t top = peak_key(residual, mask, cells);
    const float v = top != 0 ? residual[clean::index_of(top)] : 0.0f;
    if (!clark::begin_round(&st, p, top, v)) break;
    // 2. the limit: hist[b] becomes the suffix count of bin b
    std::fill(hist.begin(), hist.end(), 0u);
    for (size_t i = 0; i < cells; ++i)
      if (clean::key_of(residual[i], static_cast<uint32_t>(i),
                        mask == nullptr || mask[i] != 0) != 0)
        hist[clark::bin_of(residual[i])] += 1;
    uint32_t bins_over = 0, bins_occupied = 0;
    for (int b = clark::kBins - 1; b >= 0; --b) {
      hist[b] += hist[b + 1];
      if (hist[b] > static_cast<uint32_t>(p.max_candidates)) bins_over += 1;
      if (hist[b] > 0) bins_occupied += 1;
    }
    const uint32_t tbits = clark::limit_bits(
        st.base.level, p.select_fraction, v, bins_over, bins_occupied);
    st.round_limit = clean::float_of(tbits);
    // 3. the candidates
    list.clear();
    for (size_t i = 0; i < cells; ++i)
      if (clark::is_candidate(residual[i], mask == nullptr || mask[i] != 0,
                              tbits))
        list.push_back({static_cast<uint32_t>(i), residual[i]});
    st.n_candidates = static_cast<int32_t>(list.size());
    if (list.empty()) {
      st.base.reason = clark::kNoCandidate;
      break;
    }
    // 4. the cycle on the list
    const int n0 = st.base.n_components;
    for (int k = 0; k < p.iterations_per_round; ++k) {
      uint64_t key = 0;
      size_t at = 0;
      for (size_t j = 0; j < list.size(); ++j) {
        const uint64_t kj = clean::key_of(list[j].value, list[j].index, true);
        if (kj > key) key = kj, at = j;
      }
      if (!clark::in_round(key, tbits)) break;
      float c = 0.0f;
      if (!clean::step(&st.base, p.base, key, list[at].value, &c)) break;
      const uint32_t index = clean::index_of(key);
      const int py = static_cast<int>(index / G), px = static_cast<int>(index % G);
      components[st.base.n_components - 1] = {py, px, c};
      model[index] = model[index] + c;
      const clean::Patch pt = clean::patch_of(p.base, py, px);
      for (Candidate &e : list) {
        const int y = static_cast<int>(e.index / G);
        const int x = static_cast<int>(e.index % G);
        if (y >= pt.y0 && y < pt.y1 && x >= pt.x0 && x < pt.x1)
          e.value = clean::subtract(
              c, psf[static_cast<size_t>(y - pt.oy) * Gp + (x - pt.ox)],
              e.value);
      }
    }
    // 5. apply: the round's components onto the whole residual, in order
    for (int n = n0; n < st.base.n_components; ++n) {
      const clean::Component &rec = components[n];
      const clean::Patch pt = clean::patch_of(p.base, rec.y, rec.x);
      for (int y = pt.y0; y < pt.y1; ++y) {
        float *row = residual + static_cast<size_t>(y) * G;
        const float *prow = psf + static_cast<size_t>(y - pt.oy) * Gp;
        for (int x = pt.x0; x < pt.x1; ++x)
          row[x] = clean::subtract(rec.value, prow[x - pt.ox], row[x]);
      }
    }
  }
  clean::set_peak(&st.base, peak_key(residual, mask, cells));
  *state = st;
  return {};
}

}  // namespace host
}  // namespace idg_mi355x
