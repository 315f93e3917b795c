// clean.cpp -- the host twin of the Hogbom minor cycle (host.hpp): the one
// minor cycle of host/minor_cycle.hpp under clean::Cycle.
#include "host/host.hpp"
#include "host/minor_cycle.hpp"

namespace idg_mi355x {
namespace host {

std::string clean(const clean::Params &p, float *residual, const float *psf,
                  const uint8_t *mask, float *model,
                  clean::Component *components, clean::State *state) {
  return minor_cycle<clean::Cycle>(
      "idg_clean", p, residual, psf, mask, components, state,
      [&](float c, int, uint32_t index, int, int) {
        model[index] = model[index] + c;
      });
}

}  // namespace host
}  // namespace idg_mi355x
