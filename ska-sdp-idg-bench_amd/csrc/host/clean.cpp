// clean.cpp -- the host twin of the Hogbom minor cycle (host.hpp).
#include "host/host.hpp"

namespace idg_mi355x {
namespace host {

namespace {

namespace cl = idg_mi355x::clean;

// The key of the residual's peak (clean::key_of; 0: none), row-major.
uint64_t clean_peak(const cl::Params &p, const float *residual,
                    const uint8_t *mask) {
  const size_t cells = static_cast<size_t>(p.grid_size) * p.grid_size;
  uint64_t best = 0;
  for (size_t i = 0; i < cells; ++i) {
    const uint64_t key = cl::key_of(residual[i], static_cast<uint32_t>(i),
                                    mask == nullptr || mask[i] != 0);
    if (key > best) best = key;
  }
  return best;
}

}  // namespace

std::string clean(const cl::Params &p, float *residual, const float *psf,
                  const uint8_t *mask, float *model,
                  cl::Component *components, cl::State *state) {
  cl::State s = *state;
  if (!cl::state_ok(s, p))
    return "idg_clean: state.n_components " + std::to_string(s.n_components) +
           " outside [0, " + std::to_string(p.max_components) + "]";
  const size_t G = static_cast<size_t>(p.grid_size);
  const size_t Gp = static_cast<size_t>(p.psf_size);
  uint64_t key = 0;
  for (int k = 0;; ++k) {
    key = clean_peak(p, residual, mask);
    if (k == p.nr_iterations) break;
    float c = 0.0f;
    const uint32_t index = key != 0 ? cl::index_of(key) : 0;
    if (!cl::step(&s, p, key, key != 0 ? residual[index] : 0.0f, &c)) break;
    const int py = static_cast<int>(index / G), px = static_cast<int>(index % G);
    components[s.n_components - 1] = {py, px, c};
    model[index] = model[index] + c;
    const cl::Patch pt = cl::patch_of(p, py, px);
    for (int y = pt.y0; y < pt.y1; ++y) {
      float *row = residual + static_cast<size_t>(y) * G;
      const float *prow = psf + static_cast<size_t>(y - pt.oy) * Gp;
      for (int x = pt.x0; x < pt.x1; ++x)
        row[x] = cl::subtract(c, prow[x - pt.ox], row[x]);
    }
  }
  cl::set_peak(&s, key);
  *state = s;
  return {};
}

}  // namespace host
}  // namespace idg_mi355x
