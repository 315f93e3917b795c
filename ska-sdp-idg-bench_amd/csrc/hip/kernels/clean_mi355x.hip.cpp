// clean_mi355x.hip.cpp -- the Hogbom minor cycle on the device,
// bit for bit the host entry idg_clean: the one minor-cycle body of
// minor_cycle.hpp (the launches and who reads and writes which buffer are
// described there) under clean::Cycle, with the residual as the one plane and
// the PSF as the one patch.  Workspace: util.hpp kWorkspaceClean.
#include "hip/kernels/minor_cycle.hpp"

namespace idg_mi355x {

namespace {

struct HogbomCycle : clean::Cycle {
  // The component onto the peak's pixel, by the first thread of the workgroup
  // whose tile holds it.
  __device__ static void add_to_model(const Params &, const float *,
                                      float *model, float c, int,
                                      uint32_t index, int, int, bool owner,
                                      int, int, int, int) {
    if (owner && threadIdx.x == 0) model[index] = model[index] + c;
  }
};

}  // namespace

hipError_t launch_clean(const clean::Params &params, float *d_residual,
                        const float *d_psf, const uint8_t *d_mask,
                        float *d_model, void *d_components, void *d_state,
                        hipStream_t stream) {
  return minor::launch<HogbomCycle>(kWorkspaceClean, params, d_residual, d_psf,
                                    nullptr, d_mask, d_model, d_components,
                                    d_state, stream);
}

}  // namespace idg_mi355x
