// minor_cycle.hpp -- the host twin of the CLEAN minor cycle, once for
// host::clean (Cycle = clean::Cycle) and host::ms_clean (ms::Cycle): the peak
// over the planes, the stop decision, the record, the model and the
// subtraction of the patch on every plane.  The device's is
// hip/kernels/minor_cycle.hpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "common/clean.hpp"

namespace idg_mi355x {
namespace host {

// nr_iterations iterations from *state on planes[Cycle::planes(p)][G][G].
// entry: the C ABI entry a refusal names.  add_to_model(c, scale, index, py,
// px): the one step the cycles do not share.  Not empty: the state no
// iteration may run from (clean::state_ok), every buffer left as it was.
template <class Cycle, class AddToModel>
std::string minor_cycle(const char *entry, const typename Cycle::Params &p,
                        float *planes, const float *psf, const uint8_t *mask,
                        typename Cycle::Component *components,
                        typename Cycle::State *state,
                        AddToModel add_to_model) {
  const clean::Params &base = Cycle::base(p);
  typename Cycle::State st = *state;
  if (!clean::state_ok(Cycle::base(st), base))
    return std::string(entry) + ": state.n_components " +
           std::to_string(Cycle::base(st).n_components) + " outside [0, " +
           std::to_string(base.max_components) + "]";
  const size_t G = static_cast<size_t>(base.grid_size);
  const size_t Gp = static_cast<size_t>(base.psf_size);
  const size_t cells = G * G;
  uint64_t key = 0;
  for (int k = 0;; ++k) {
    // the key of the planes' peak (Cycle::key_of; 0: none)
    key = 0;
    for (int q = 0; q < Cycle::planes(p); ++q) {
      const float *plane = planes + q * cells;
      for (size_t i = 0; i < cells; ++i) {
        const uint64_t at =
            Cycle::key_of(p, q, plane[i], static_cast<uint32_t>(i),
                          mask == nullptr || mask[i] != 0);
        if (at > key) key = at;
      }
    }
    if (k == base.nr_iterations) break;
    float c = 0.0f;
    const uint32_t index = key != 0 ? Cycle::index_of(key) : 0;
    const int s = key != 0 ? Cycle::scale_of(key) : 0;
    if (!Cycle::step(&st, p, key,
                     key != 0 ? planes[s * cells + index] : 0.0f, &c))
      break;
    const int py = static_cast<int>(index / G), px = static_cast<int>(index % G);
    components[Cycle::base(st).n_components - 1] = Cycle::record(py, px, s, c);
    add_to_model(c, s, index, py, px);
    const clean::Patch pt = clean::patch_of(base, py, px);
    for (int q = 0; q < Cycle::planes(p); ++q) {
      float *plane = planes + q * cells;
      const float *patch = psf + Cycle::psf_at(p, s, q);
      for (int y = pt.y0; y < pt.y1; ++y) {
        float *row = plane + static_cast<size_t>(y) * G;
        const float *prow = patch + static_cast<size_t>(y - pt.oy) * Gp;
        for (int x = pt.x0; x < pt.x1; ++x)
          row[x] = clean::subtract(c, prow[x - pt.ox], row[x]);
      }
    }
  }
  Cycle::set_peak(&st, key);
  *state = st;
  return {};
}

}  // namespace host
}  // namespace idg_mi355x
