// host.hpp -- the host twins of the device steps: the plan walk, the imaging
// weights, the Hogbom minor cycle, multi-scale CLEAN, Clark CLEAN, the restore
// step and the taper's image.  Plain C++ over the per-element rules of
// common/{plan,weight,clean,multiscale,clark,restore}.hpp, no HIP call, so they
// run (and compile) without a GPU; the GPU suites compare the device kernels
// against them bit for bit.  Each takes the parsed values its launch_*
// counterpart (hip/util.hpp) takes; the C ABI (capi/idg_capi.cpp) validates
// the arguments, calls one of them and reports what it returns.
#pragma once

#include <complex>
#include <cstddef>
#include <cstdint>
#include <string>

#include "common/clark.hpp"
#include "common/clean.hpp"
#include "common/multiscale.hpp"
#include "common/plan.hpp"
#include "common/restore.hpp"
#include "common/types.hpp"
#include "common/weight.hpp"

namespace idg_mi355x {
namespace host {

using UVW = idg::UVWCoordinate<float>;

// An IDG_E_* code of include/idg_mi355x.h and its message; 0: success.
struct Status {
  int code = 0;
  std::string message;
};

// host/plan.cpp.  The count, prefix and fill passes over
// nr_baselines x nr_timesteps uvw rows, the baselines split over at most
// `nthreads` threads (the bytes do not depend on it): counts = {subgrids
// needed, dropped timesteps}; records past `capacity` are not written.
void plan(plan::Geometry geometry, float image_size, float inv_w_step,
          int nr_baselines, int nr_timesteps, int nr_channels,
          const uint32_t *baselines, const UVW *uvw, const float *wavenumbers,
          idg::Metadata *metadata, int capacity, int32_t counts[2],
          int nthreads);

// host/weight.cpp.  IDG_E_OUT_OF_BOUNDS: a record's rows
// outside [0, uvw_rows); IDG_E_INVALID_ARGUMENT: a density cell at or above
// 2^62, on entry or (weight_density, which then leaves `density` as it was)
// while summing.  They check rows first, then cells.
Status weight_density(const weight::Geometry &geometry, int nr_subgrids,
                      int nr_channels, const idg::Metadata *metadata,
                      const UVW *uvw, size_t uvw_rows,
                      const float *wavenumbers, const float *weights,
                      uint64_t *density);
Status weight_scheme(const weight::Geometry &geometry, int scheme,
                     double briggs_scale, const uint64_t *density,
                     float ab[2]);
// visibilities null: out = (f, 0, 0, f).
Status weight_apply(const weight::Geometry &geometry, int nr_subgrids,
                    int nr_channels, const idg::Metadata *metadata,
                    const UVW *uvw, size_t uvw_rows, const float *wavenumbers,
                    const float *weights, const uint64_t *density,
                    const float ab[2],
                    const std::complex<float> *visibilities,
                    float *imaging_weights, std::complex<float> *out,
                    double *sum_weights);

// host/clean.cpp.  params.nr_iterations iterations from
// *state; mask may be null.  Not empty: the state no iteration may run from
// (clean::state_ok), every buffer left as it was.
std::string clean(const clean::Params &params, float *residual,
                  const float *psf, const uint8_t *mask, float *model,
                  clean::Component *components, clean::State *state);

// host/restore.cpp.  The clean beam exp(-(a dx^2 + 2 b dx dy +
// c dy^2)) with its FWHMs and the major axis' angle (idg_beam_t without its
// struct_size); all of it in doubles, host only.
struct Beam {
  double a, b, c;
  double major, minor, pa;
};
// a, b, c finite and the form positive definite.
bool beam_ok(const Beam &beam);
// Not empty: the refusal, *out untouched.
std::string beam_from_axes(double major, double minor, double pa, Beam *out);
std::string beam_fit(int psf_size, const float *psf, float level, Beam *out);
// floor(sqrt(-ln(cutoff) / the smaller eigenvalue)), as a double.
double beam_reach(const Beam &beam, double cutoff);
// taps[2 radius + 1][2 radius + 1]; dx^2, dx dy and dy^2 are exact integers.
void beam_taps(const Beam &beam, int radius, float *taps);
// The restore step: the non-zero model pixels in row-major order, each one's
// footprint added onto an accumulator plane, then the add of the residual
// (null: none).  Its cost follows the number of non-zero pixels.  Not empty:
// no memory for the accumulator, nothing written.
std::string restore(const restore::Params &params, const float *model,
                    const float *residual, const float *taps,
                    float *restored);

// host/multiscale.cpp.  A scale's Gaussian in doubles: its
// radius ceil(3 sigma), sigma = scale * 3 / 16 (-1: scale negative, NaN or
// wider than ms::kMaxRadius), and its 2 radius + 1 normalised taps.
int ms_scale_radius(double scale);
void ms_scale_taps(double scale, int radius, float *taps);
// The dense separable convolution of a [G][G] plane that is zero beyond its
// edge: the row pass into tmp, the column pass into out (which may be `in`).
void convolve_separable(int grid_size, int radius, const float *in,
                        const float *taps, float *tmp, float *out);
// planes[Ns][G][G] and cross_psf[Ns (Ns + 1) / 2][Gp][Gp] from the residual
// and the PSF; taps: every scale's, one after the other; tmp[G][G].
void ms_prepare(const ms::Params &params, const float *residual,
                const float *psf, const float *taps, float *planes,
                float *cross_psf, float *tmp);
// params.base.nr_iterations iterations from *state; mask may be null.  Not
// empty: the state no iteration may run from, every buffer left as it was.
std::string ms_clean(const ms::Params &params, float *planes,
                     const float *cross_psf, const float *taps,
                     const uint8_t *mask, float *model,
                     ms::Component *components, ms::State *state);

// host/clark.cpp.  params.nr_rounds rounds from *state, each
// at most params.iterations_per_round components on a candidate list, then
// subtracted from the whole residual; mask may be null.  Not empty: the state
// no round may run from (clean::state_ok), every buffer left as it was.
std::string clark(const clark::Params &params, float *residual,
                  const float *psf, const uint8_t *mask, float *model,
                  clean::Component *components, clark::State *state);

// host/image.cpp.  out[G][G]: the [S][S] taper interpolated
// to the image's pixels, in doubles.
void taper_to_image(int subgrid_size, int grid_size, const float *spheroidal,
                    double *out);

}  // namespace host
}  // namespace idg_mi355x
