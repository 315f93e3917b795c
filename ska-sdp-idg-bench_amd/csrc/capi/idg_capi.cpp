// idg_capi.cpp -- the extern "C" boundary (include/idg_mi355x.h): every entry
// validates its arguments and calls the launch layer (hip/util.hpp) or a host
// twin (host/host.hpp).
#include "idg_mi355x.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "hip/util.hpp"
#include "host/host.hpp"
#include "lib-hip.hpp"

static_assert(sizeof(idg_metadata_t) == sizeof(idg::Metadata),
              "metadata layout");
static_assert(sizeof(idg_uvw_t) == sizeof(idg::UVWCoordinate<float>),
              "uvw layout");
static_assert(sizeof(idg_cfloat_t) == sizeof(std::complex<float>),
              "complex layout");

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

int from_hip(hipError_t e, const char *what) {
  if (e == hipSuccess) return IDG_OK;
  return fail(static_cast<int>(e),
              std::string(what) + ": " + hipGetErrorString(e));
}

idg_mi355x::Problem make_problem(int nr_subgrids, int grid_size,
                                 int subgrid_size, float image_size,
                                 float w_step, int nr_channels,
                                 int nr_stations) {
  idg_mi355x::Problem p;
  p.nr_subgrids = nr_subgrids;
  p.grid_size = grid_size;
  p.subgrid_size = subgrid_size;
  p.image_size = image_size;
  p.w_step_in_lambda = w_step;
  p.nr_channels = nr_channels;
  p.nr_stations = nr_stations;
  return p;
}

// The struct_size rules of include/idg_mi355x.h for every versioned struct T
// (`name`: its type name): *out = the caller's fields, zero-extended to this
// library's struct; bytes of a newer, larger struct must be zero (a field
// this library cannot honour).
template <typename T>
int read_struct(const T *in, const char *name, T *out) {
  const std::string who = name;
  if (in == nullptr) return fail(IDG_E_INVALID_ARGUMENT, who + ": null");
  const uint32_t size = in->struct_size;
  if (size < sizeof(uint32_t) || size % 4 != 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                who + ": struct_size " + std::to_string(size) +
                    " (set it to sizeof(" + who + "), a multiple of 4)");
  if (size > (1u << 16))
    return fail(IDG_E_INVALID_ARGUMENT,
                who + ": struct_size " + std::to_string(size) + " is no " +
                    who + " of any version");
  std::memset(out, 0, sizeof *out);
  std::memcpy(out, in, std::min<size_t>(size, sizeof *out));
  const unsigned char *raw = reinterpret_cast<const unsigned char *>(in);
  for (size_t i = sizeof *out; i < size; ++i)
    if (raw[i] != 0)
      return fail(IDG_E_INVALID_ARGUMENT,
                  who + ": struct_size " + std::to_string(size) +
                      " with a field set that this library (struct_size " +
                      std::to_string(sizeof *out) + ") does not know");
  return IDG_OK;
}

// idg_options_t -> idg_mi355x::Options (still a request: unset fields are
// resolved from the environment where they are used).  Null: all unset.
int parse_options(const idg_options_t *o, idg_mi355x::Options *out) {
  *out = idg_mi355x::Options();
  if (o == nullptr) return IDG_OK;
  idg_options_t v;
  if (int rc = read_struct(o, "idg_options_t", &v)) return rc;
  if (v.gridder_impl > IDG_IMPL_AUTO)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_options_t: unknown gridder_impl " +
                    std::to_string(v.gridder_impl));
  if (v.degridder_impl != IDG_IMPL_ENV && v.degridder_impl != IDG_IMPL_DEFAULT &&
      v.degridder_impl != IDG_IMPL_SEQUENTIAL)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_options_t: degridder_impl " +
                    std::to_string(v.degridder_impl) +
                    " (IDG_IMPL_DEFAULT or IDG_IMPL_SEQUENTIAL)");
  if (v.precision != 0 && (v.precision & ~7u) != IDG_PREC_SET)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_options_t: precision " + std::to_string(v.precision) +
                    " (0, or IDG_PREC_SET | bits 0..7)");
  if (v.kernel_form > IDG_FORM_SPLIT)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_options_t: unknown kernel_form " +
                                            std::to_string(v.kernel_form));
  if (v.fft_fusion > IDG_FFT_FUSION_ON)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_options_t: unknown fft_fusion " +
                                            std::to_string(v.fft_fusion));
  out->gridder_impl = static_cast<int>(v.gridder_impl);
  out->degridder_impl = static_cast<int>(v.degridder_impl);
  out->precision = static_cast<int>(v.precision);
  out->kernel_form = static_cast<int>(v.kernel_form);
  out->fft_fusion = static_cast<int>(v.fft_fusion);
  out->auto_threshold = v.auto_threshold;
  return IDG_OK;
}
static_assert(IDG_IMPL_DEFAULT == idg_mi355x::kImplDefault &&
                  IDG_IMPL_VALU == idg_mi355x::kImplValu &&
                  IDG_IMPL_SEQUENTIAL == idg_mi355x::kImplSequential &&
                  IDG_IMPL_ORDERED == idg_mi355x::kImplOrdered &&
                  IDG_IMPL_AUTO == idg_mi355x::kImplAuto &&
                  IDG_PREC_SET == idg_mi355x::kPrecSet &&
                  IDG_FORM_COMBINED == idg_mi355x::kFormCombined &&
                  IDG_FORM_SPLIT == idg_mi355x::kFormSplit &&
                  IDG_FFT_FUSION_OFF == idg_mi355x::kFftFusionOff &&
                  IDG_FFT_FUSION_ON == idg_mi355x::kFftFusionOn &&
                  IDG_AUTO_THRESHOLD_DEFAULT == idg_mi355x::kAutoThreshold,
              "idg_options_t values are idg_mi355x::Options values");

// idg_plan_params_t (read_struct) and the sizes of a plan call ->
// plan::Geometry without its scales, image_size and 1 / w_step_in_lambda
// (computed here, once, for the host and the device).
int parse_plan(const idg_plan_params_t *params, int nr_baselines,
               int nr_timesteps, int nr_channels, int capacity,
               idg_mi355x::plan::Geometry *g, float *image_size,
               float *inv_w_step) {
  idg_plan_params_t v;
  if (int rc = read_struct(params, "idg_plan_params_t", &v)) return rc;
  if (nr_baselines < 1 || nr_timesteps < 1 || nr_channels < 1 || capacity < 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "plan: nr_baselines, nr_timesteps, nr_channels >= 1 and "
                "capacity >= 0 required");
  if (static_cast<long long>(nr_baselines) * nr_timesteps >= (1ll << 31))
    return fail(IDG_E_INVALID_ARGUMENT,
                "plan: nr_baselines * nr_timesteps must be below 2^31");
  if (v.subgrid_size < 1 || v.grid_size < v.subgrid_size)
    return fail(IDG_E_INVALID_ARGUMENT,
                "plan: 1 <= subgrid_size <= grid_size required");
  if (v.kernel_size < 0 || v.kernel_size >= v.subgrid_size)
    return fail(IDG_E_INVALID_ARGUMENT,
                "plan: 0 <= kernel_size < subgrid_size required");
  if (v.max_nr_timesteps_per_subgrid < 1 || v.nr_timesteps_per_aterm < 0 ||
      v.nr_w_layers < 1 || v.nr_w_layers > (1 << 24))
    return fail(IDG_E_INVALID_ARGUMENT,
                "plan: max_nr_timesteps_per_subgrid >= 1, "
                "nr_timesteps_per_aterm >= 0, 1 <= nr_w_layers <= 2^24 "
                "(a layer index is clamped as a float) required");
  g->grid_size = v.grid_size;
  g->subgrid_size = v.subgrid_size;
  g->kernel_size = v.kernel_size;
  g->max_timesteps = v.max_nr_timesteps_per_subgrid;
  g->aterm_steps = v.nr_timesteps_per_aterm;
  g->nr_w_layers = v.nr_w_layers;
  g->use_w = v.w_step_in_lambda != 0.0f ? 1 : 0;
  g->s0 = g->s1 = g->ws = 0.0f;
  *image_size = v.image_size;
  *inv_w_step = g->use_w ? 1.0f / v.w_step_in_lambda : 0.0f;
  return IDG_OK;
}

// idg_weight_params_t (read_struct) and the sizes of a weight call -> weight::Geometry, the scheme and (5 * 10^-robust)^2.
struct WeightCall {
  idg_mi355x::weight::Geometry g;
  int scheme = 0;
  double briggs_scale = 0.0;
};

int parse_weight(const idg_weight_params_t *params, int nr_subgrids,
                 int subgrid_size, int nr_channels, WeightCall *out) {
  namespace wt = idg_mi355x::weight;
  idg_weight_params_t v;
  if (int rc = read_struct(params, "idg_weight_params_t", &v)) return rc;
  if (nr_subgrids < 0 || subgrid_size < 1 || nr_channels < 1)
    return fail(IDG_E_INVALID_ARGUMENT,
                "weight: nr_subgrids >= 0, subgrid_size >= 1 and "
                "nr_channels >= 1 required");
  if (v.grid_size < 1 || v.grid_size > 16384)
    return fail(IDG_E_INVALID_ARGUMENT,
                "weight: 1 <= grid_size <= 16384 required");
  if (v.quantum_log2 < wt::kQuantumLog2Min ||
      v.quantum_log2 > wt::kQuantumLog2Max)
    return fail(IDG_E_INVALID_ARGUMENT,
                "weight: quantum_log2 must lie in [-64, 64]");
  if (v.scheme != IDG_WEIGHT_NATURAL && v.scheme != IDG_WEIGHT_UNIFORM &&
      v.scheme != IDG_WEIGHT_BRIGGS)
    return fail(IDG_E_INVALID_ARGUMENT,
                "weight: unknown scheme " + std::to_string(v.scheme));
  if (!std::isfinite(v.image_size) || !std::isfinite(v.robust))
    return fail(IDG_E_INVALID_ARGUMENT,
                "weight: image_size and robust must be finite");
  out->g.grid_size = v.grid_size;
  out->g.quantum_log2 = v.quantum_log2;
  out->g.hermitian = v.hermitian != 0 ? 1 : 0;
  out->g.cells = wt::cells_of(v.image_size);
  out->scheme = v.scheme;
  const double r = 5.0 * std::pow(10.0, -static_cast<double>(v.robust));
  out->briggs_scale = r * r;
  return IDG_OK;
}
static_assert(IDG_WEIGHT_NATURAL == idg_mi355x::weight::kNatural &&
                  IDG_WEIGHT_UNIFORM == idg_mi355x::weight::kUniform &&
                  IDG_WEIGHT_BRIGGS == idg_mi355x::weight::kBriggs,
              "idg_weight_params_t scheme values are weight:: values");

// What a host twin (host/host.hpp) returns -> the entry's return value.
int from_host(const idg_mi355x::host::Status &st) {
  return st.code ? fail(st.code, st.message) : IDG_OK;
}

// idg_clean_params_t (read_struct) -> clean::Params.
int parse_clean(const idg_clean_params_t *params,
                idg_mi355x::clean::Params *out) {
  idg_clean_params_t v;
  if (int rc = read_struct(params, "idg_clean_params_t", &v)) return rc;
  if (v.psf_size < 1 || v.grid_size < v.psf_size ||
      v.grid_size > idg_mi355x::clean::kMaxGridSize)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clean: 1 <= psf_size <= grid_size <= 16384 required");
  if (!std::isfinite(v.gain) || !std::isfinite(v.threshold) ||
      !std::isfinite(v.cycle_fraction) || v.threshold < 0.0f ||
      v.cycle_fraction < 0.0f)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clean: gain, threshold and cycle_fraction must be finite, "
                "threshold and cycle_fraction not negative");
  if (v.nr_iterations < 0 || v.max_components < 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clean: nr_iterations >= 0 and max_components >= 0 required");
  out->grid_size = v.grid_size;
  out->psf_size = v.psf_size;
  out->max_components = v.max_components;
  out->nr_iterations = v.nr_iterations;
  out->gain = v.gain;
  out->threshold = v.threshold;
  out->cycle_fraction = v.cycle_fraction;
  return IDG_OK;
}
static_assert(IDG_CLEAN_RUNNING == idg_mi355x::clean::kRunning &&
                  IDG_CLEAN_BELOW_LEVEL == idg_mi355x::clean::kBelowLevel &&
                  IDG_CLEAN_NO_PEAK == idg_mi355x::clean::kNoPeak &&
                  IDG_CLEAN_COMPONENTS_FULL ==
                      idg_mi355x::clean::kComponentsFull &&
                  sizeof(idg_clean_component_t) ==
                      sizeof(idg_mi355x::clean::Component) &&
                  sizeof(idg_clean_component_t) == 12 &&
                  sizeof(idg_clean_state_t) ==
                      sizeof(idg_mi355x::clean::State) &&
                  sizeof(idg_clean_state_t) == 24,
              "idg_clean_* records are clean:: records");

// idg_clark_params_t (read_struct) -> clark::Params.
int parse_clark(const idg_clark_params_t *params,
                idg_mi355x::clark::Params *out) {
  idg_clark_params_t v;
  if (int rc = read_struct(params, "idg_clark_params_t", &v)) return rc;
  if (v.psf_size < 1 || v.grid_size < v.psf_size ||
      v.grid_size > idg_mi355x::clean::kMaxGridSize)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clark: 1 <= psf_size <= grid_size <= 16384 required");
  if (!std::isfinite(v.gain) || !std::isfinite(v.threshold) ||
      !std::isfinite(v.cycle_fraction) || v.threshold < 0.0f ||
      v.cycle_fraction < 0.0f)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clark: gain, threshold and cycle_fraction must be finite, "
                "threshold and cycle_fraction not negative");
  if (!std::isfinite(v.select_fraction) || v.select_fraction < 0.0f ||
      v.select_fraction > 1.0f)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clark: select_fraction must be in [0, 1]");
  if (v.nr_rounds < 0 || v.iterations_per_round < 0 || v.max_components < 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clark: nr_rounds >= 0, iterations_per_round >= 0 and "
                "max_components >= 0 required");
  if (v.max_candidates < 1 ||
      v.max_candidates > idg_mi355x::clark::kMaxCandidates)
    return fail(IDG_E_INVALID_ARGUMENT,
                "clark: 1 <= max_candidates <= 16384 required");
  out->base.grid_size = v.grid_size;
  out->base.psf_size = v.psf_size;
  out->base.max_components = v.max_components;
  out->base.nr_iterations = 0;
  out->base.gain = v.gain;
  out->base.threshold = v.threshold;
  out->base.cycle_fraction = v.cycle_fraction;
  out->nr_rounds = v.nr_rounds;
  out->iterations_per_round = v.iterations_per_round;
  out->max_candidates = v.max_candidates;
  out->select_fraction = v.select_fraction;
  return IDG_OK;
}
static_assert(IDG_CLARK_NO_CANDIDATE == idg_mi355x::clark::kNoCandidate &&
                  sizeof(idg_clark_state_t) ==
                      sizeof(idg_mi355x::clark::State) &&
                  sizeof(idg_clark_state_t) == 36,
              "idg_clark_state_t is clark::State");

// Half-open byte ranges of a call's buffers: `who`: "a and b overlap" for the
// first pair that does and is not listed in `may` (pairs of indices that may
// be the same pointer).  Null buffers are skipped.
struct Span {
  const char *name;
  const void *at;
  size_t bytes;
};
int no_overlap(const char *who, const std::vector<Span> &spans,
               const std::vector<std::pair<int, int>> &may = {}) {
  for (size_t i = 0; i < spans.size(); ++i)
    for (size_t j = i + 1; j < spans.size(); ++j) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(spans[i].at);
      const uintptr_t b = reinterpret_cast<uintptr_t>(spans[j].at);
      if (a == 0 || b == 0) continue;
      bool allowed = false;
      for (const auto &m : may)
        allowed |= m.first == static_cast<int>(i) &&
                   m.second == static_cast<int>(j) && a == b;
      if (allowed) continue;
      if (a < b + spans[j].bytes && b < a + spans[i].bytes)
        return fail(IDG_E_INVALID_ARGUMENT,
                    std::string(who) + ": " + spans[i].name + " and " +
                        spans[j].name + " overlap");
    }
  return IDG_OK;
}

// The sizes and buffers of a convolution call (`entry`: which of the two).
int parse_convolve(const char *entry, int grid_size, int radius,
                   const float *in, const float *taps, const float *tmp,
                   const float *out) {
  namespace ms = idg_mi355x::ms;
  if (grid_size < 1 || grid_size > ms::kMaxGridSize || radius < 0 ||
      radius > ms::kMaxRadius)
    return fail(IDG_E_INVALID_ARGUMENT,
                std::string(entry) + ": 1 <= grid_size <= 16384 and 0 <= "
                                     "radius <= 48 required");
  if (!in || !taps || !tmp || !out)
    return fail(IDG_E_INVALID_ARGUMENT, std::string(entry) + ": null buffer");
  const size_t plane = sizeof(float) * grid_size * grid_size;
  return no_overlap(entry,
                    {{"in", in, plane},
                     {"out", out, plane},
                     {"tmp", tmp, plane},
                     {"taps", taps, sizeof(float) * (2 * radius + 1)}},
                    {{0, 1}});
}

// idg_ms_params_t (read_struct) -> ms::Params.  minor_cycle: the fields only
// idg_ms_clean reads are checked too.
int parse_ms(const idg_ms_params_t *params, bool minor_cycle,
             idg_mi355x::ms::Params *out) {
  namespace ms = idg_mi355x::ms;
  idg_ms_params_t v;
  if (int rc = read_struct(params, "idg_ms_params_t", &v)) return rc;
  if (v.psf_size < 1 || v.grid_size < v.psf_size ||
      v.grid_size > ms::kMaxGridSize)
    return fail(IDG_E_INVALID_ARGUMENT,
                "multiscale: 1 <= psf_size <= grid_size <= 16384 required");
  if (v.nr_scales < 1 || v.nr_scales > ms::kMaxScales)
    return fail(IDG_E_INVALID_ARGUMENT,
                "multiscale: 1 <= nr_scales <= 8 required");
  if (v.radius[0] != 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "multiscale: radius[0] must be 0 (scale 0 is the delta)");
  for (int s = 0; s < v.nr_scales; ++s)
    if (v.radius[s] < 0 || v.radius[s] > ms::kMaxRadius)
      return fail(IDG_E_INVALID_ARGUMENT,
                  "multiscale: 0 <= radius <= 48 required");
  if (minor_cycle) {
    if (!std::isfinite(v.gain) || !std::isfinite(v.threshold) ||
        !std::isfinite(v.cycle_fraction) || v.threshold < 0.0f ||
        v.cycle_fraction < 0.0f)
      return fail(IDG_E_INVALID_ARGUMENT,
                  "multiscale: gain, threshold and cycle_fraction must be "
                  "finite, threshold and cycle_fraction not negative");
    if (v.nr_iterations < 0 || v.max_components < 0)
      return fail(IDG_E_INVALID_ARGUMENT,
                  "multiscale: nr_iterations >= 0 and max_components >= 0 "
                  "required");
    for (int s = 0; s < v.nr_scales; ++s)
      if (!std::isfinite(v.weight[s]) || !std::isfinite(v.inv_peak[s]))
        return fail(IDG_E_INVALID_ARGUMENT,
                    "multiscale: weight and inv_peak must be finite");
  }
  *out = ms::Params();
  out->base.grid_size = v.grid_size;
  out->base.psf_size = v.psf_size;
  out->base.max_components = v.max_components;
  out->base.nr_iterations = v.nr_iterations;
  out->base.gain = v.gain;
  out->base.threshold = v.threshold;
  out->base.cycle_fraction = v.cycle_fraction;
  out->nr_scales = v.nr_scales;
  for (int s = 0; s < v.nr_scales; ++s) {
    out->radius[s] = v.radius[s];
    out->weight[s] = v.weight[s];
    out->inv_peak[s] = v.inv_peak[s];
  }
  return IDG_OK;
}
static_assert(IDG_MS_MAX_SCALES == idg_mi355x::ms::kMaxScales &&
                  IDG_MS_MAX_RADIUS == idg_mi355x::ms::kMaxRadius &&
                  sizeof(idg_ms_component_t) ==
                      sizeof(idg_mi355x::ms::Component) &&
                  sizeof(idg_ms_component_t) == 16 &&
                  sizeof(idg_ms_state_t) == sizeof(idg_mi355x::ms::State) &&
                  sizeof(idg_ms_state_t) == 28,
              "idg_ms_* records are ms:: records");

// The buffers of a prepare call and of a minor-cycle call (`entry`: which
// form): none null but the mask, none overlapping.
int ms_prepare_buffers(const char *entry, const idg_mi355x::ms::Params &p,
                       const float *residual, const float *psf,
                       const float *taps, const float *planes,
                       const float *cross_psf, const float *tmp) {
  namespace ms = idg_mi355x::ms;
  if (!residual || !psf || !taps || !planes || !cross_psf || !tmp)
    return fail(IDG_E_INVALID_ARGUMENT, std::string(entry) + ": null buffer");
  const size_t plane = sizeof(float) * p.base.grid_size * p.base.grid_size;
  const size_t patch = sizeof(float) * p.base.psf_size * p.base.psf_size;
  const int Ns = p.nr_scales;
  // (residual may be planes[0] itself: the same pointer)
  return no_overlap(
      entry,
      {{"residual", residual, plane},
       {"planes", planes, plane * Ns},
       {"psf", psf, patch},
       {"taps", taps, sizeof(float) * ms::taps_at(p, Ns)},
       {"cross_psf", cross_psf, patch * (Ns * (Ns + 1) / 2)},
       {"tmp", tmp, plane}},
      {{0, 1}});
}
int ms_clean_buffers(const char *entry, const idg_mi355x::ms::Params &p,
                     const float *planes, const float *cross_psf,
                     const float *taps, const uint8_t *mask,
                     const float *model, const void *components,
                     const void *state) {
  namespace ms = idg_mi355x::ms;
  if (!planes || !cross_psf || !taps || !model || !components || !state)
    return fail(IDG_E_INVALID_ARGUMENT, std::string(entry) + ": null buffer");
  const size_t cells =
      static_cast<size_t>(p.base.grid_size) * p.base.grid_size;
  const size_t patch = sizeof(float) * p.base.psf_size * p.base.psf_size;
  const int Ns = p.nr_scales;
  return no_overlap(
      entry,
      {{"planes", planes, sizeof(float) * cells * Ns},
       {"cross_psf", cross_psf, patch * (Ns * (Ns + 1) / 2)},
       {"taps", taps, sizeof(float) * ms::taps_at(p, Ns)},
       {"mask", mask, cells},
       {"model", model, sizeof(float) * cells},
       {"components", components,
        sizeof(idg_ms_component_t) * p.base.max_components},
       {"state", state, sizeof(idg_ms_state_t)}});
}

// idg_beam_t (read_struct) -> host::Beam; `who`: the entry.  The form must be
// positive definite.
int parse_beam(const idg_beam_t *beam, const char *who,
               idg_mi355x::host::Beam *out) {
  idg_beam_t v;
  if (int rc = read_struct(beam, "idg_beam_t", &v)) return rc;
  const idg_mi355x::host::Beam b = {v.a, v.b, v.c, v.major, v.minor, v.pa};
  if (!idg_mi355x::host::beam_ok(b))
    return fail(IDG_E_INVALID_ARGUMENT,
                std::string(who) + ": a, b, c must be finite with a > 0, "
                                   "c > 0 and a c - b^2 > 0");
  *out = b;
  return IDG_OK;
}

// A beam back to the caller's idg_beam_t (already through read_struct): the
// fields its struct_size has room for; struct_size stays the caller's.
void store_beam(const idg_mi355x::host::Beam &b, idg_beam_t *beam) {
  idg_beam_t v;
  std::memset(&v, 0, sizeof v);
  v.struct_size = beam->struct_size;
  v.a = b.a, v.b = b.b, v.c = b.c;
  v.major = b.major, v.minor = b.minor, v.pa = b.pa;
  std::memcpy(beam, &v, std::min<size_t>(v.struct_size, sizeof v));
}

// idg_restore_params_t (read_struct) and the buffers of a restore call
// (`entry`: which of the two) -> restore::Params.  Pointer values only: the
// _launch form's are device pointers.
int parse_restore(const char *entry, const idg_restore_params_t *params,
                  const float *model, const float *residual,
                  const float *taps, const float *restored,
                  idg_mi355x::restore::Params *out) {
  namespace rs = idg_mi355x::restore;
  idg_restore_params_t v;
  if (int rc = read_struct(params, "idg_restore_params_t", &v)) return rc;
  if (v.grid_size < 1 || v.grid_size > rs::kMaxGridSize || v.radius < 0 ||
      v.radius > rs::kMaxRadius)
    return fail(IDG_E_INVALID_ARGUMENT,
                "restore: 1 <= grid_size <= 16384 and 0 <= radius <= 32 "
                "required");
  if (!model || !taps || !restored)
    return fail(IDG_E_INVALID_ARGUMENT, std::string(entry) + ": null buffer");
  const size_t plane = sizeof(float) * v.grid_size * v.grid_size;
  const size_t side = 2 * static_cast<size_t>(v.radius) + 1;
  struct Span {
    const char *name;
    uintptr_t at;
    size_t bytes;
  };
  const Span spans[4] = {
      {"model", reinterpret_cast<uintptr_t>(model), plane},
      {"residual", reinterpret_cast<uintptr_t>(residual), plane},
      {"taps", reinterpret_cast<uintptr_t>(taps), sizeof(float) * side * side},
      {"restored", reinterpret_cast<uintptr_t>(restored), plane}};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) {
      const Span &a = spans[i], &b = spans[j];
      if (a.at == 0 || b.at == 0) continue;  // (no residual)
      if (i == 1 && j == 3 && a.at == b.at) continue;  // restored is residual
      if (a.at < b.at + b.bytes && b.at < a.at + a.bytes)
        return fail(IDG_E_INVALID_ARGUMENT,
                    std::string(entry) + ": " + a.name + " and " + b.name +
                        " overlap (only restored == residual may)");
    }
  out->grid_size = v.grid_size;
  out->radius = v.radius;
  return IDG_OK;
}

// The null-buffer test that a host entry and its _launch twin (`entry`: which
// of the two) share.
int null_buffer(const char *entry, bool any_null) {
  if (!any_null) return IDG_OK;
  return fail(IDG_E_INVALID_ARGUMENT, std::string(entry) + ": null buffer");
}
int plan_buffers(const char *entry, const void *baselines, const void *uvw,
                 const void *wavenumbers, const void *metadata, int capacity,
                 const void *counts) {
  return null_buffer(entry, !baselines || !uvw || !wavenumbers || !counts ||
                                (capacity > 0 && !metadata));
}
int density_buffers(const char *entry, const void *metadata, const void *uvw,
                    const void *wavenumbers, const void *weights,
                    const void *density) {
  return null_buffer(entry,
                     !metadata || !uvw || !wavenumbers || !weights || !density);
}
int scheme_buffers(const char *entry, const void *density, const void *ab) {
  return null_buffer(entry, !density || !ab);
}
int clean_buffers(const char *entry, const void *residual, const void *psf,
                  const void *model, const void *components,
                  const void *state) {
  return null_buffer(entry,
                     !residual || !psf || !model || !components || !state);
}

int check_geometry(const idg_mi355x::Problem &p) {
  if (p.nr_subgrids < 0 || p.subgrid_size <= 0 || p.nr_channels <= 0 ||
      p.nr_stations <= 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "nr_subgrids >= 0, subgrid_size, nr_channels, nr_stations > 0 "
                "required");
  return IDG_OK;
}

int run_host(idg_mi355x::Direction dir, const idg_mi355x::Problem &p,
             size_t uvw_rows, size_t aterm_slots, const void *uvw,
             const float *wn, void *vis, const float *sph, const void *at,
             const idg_metadata_t *md, void *sg,
             const idg_options_t *options) {
  idg_mi355x::Options opt;
  if (int rc = parse_options(options, &opt)) return rc;
  if (int rc = check_geometry(p)) return rc;
  if (p.nr_subgrids == 0) return IDG_OK;
  if (!uvw || !wn || !vis || !sph || !at || !md || !sg)
    return fail(IDG_E_INVALID_ARGUMENT, "null buffer");
  idg_mi355x::Extents e;
  e.uvw_rows = uvw_rows;
  e.aterm_slots = aterm_slots;
  std::string msg;
  const hipError_t err = idg_mi355x::run_host(
      dir, p, e, uvw, wn, vis, sph, at,
      reinterpret_cast<const idg::Metadata *>(md), sg, &msg, nullptr, opt);
  if (!msg.empty()) return fail(IDG_E_OUT_OF_BOUNDS, msg);
  return from_hip(err, dir == idg_mi355x::Direction::kGridder
                           ? "idg_c_run_gridder"
                           : "idg_c_run_degridder");
}

int launch(idg_mi355x::Direction dir, const idg_mi355x::Problem &p,
           const void *uvw, const float *wn, void *vis, const float *sph,
           const void *at, const void *md, void *sg, void *stream,
           const idg_options_t *options) {
  idg_mi355x::Options opt;
  if (int rc = parse_options(options, &opt)) return rc;
  if (int rc = check_geometry(p)) return rc;
  if (p.nr_subgrids == 0) return IDG_OK;
  if (!uvw || !wn || !vis || !sph || !at || !md || !sg)
    return fail(IDG_E_INVALID_ARGUMENT, "null buffer");
  return from_hip(
      idg_mi355x::launch(dir, p, uvw, wn, vis, sph, at, md, sg,
                         static_cast<hipStream_t>(stream), nullptr, opt),
      "hipLaunchKernel");
}

}  // namespace

extern "C" {

int idg_abi_version(void) { return IDG_MI355X_ABI_VERSION; }

const char *idg_last_error(void) { return g_last_error.c_str(); }

int idg_release_workspaces(void *stream, int all) {
  return from_hip(idg_mi355x::release_workspaces(
                      static_cast<hipStream_t>(stream), all != 0),
                  "idg_release_workspaces");
}

int idg_subgrid_fft_launch(int nr_subgrids, int subgrid_size, int sign,
                           float scale, idg_cfloat_t *subgrids, void *stream) {
  if (nr_subgrids < 0 || subgrid_size <= 0 || subgrid_size > 64 ||
      (sign != 1 && sign != -1))
    return fail(IDG_E_INVALID_ARGUMENT,
                "nr_subgrids >= 0, 0 < subgrid_size <= 64, sign = +1 or -1");
  return from_hip(idg_mi355x::launch_subgrid_fft(
                      nr_subgrids, subgrid_size, sign, scale, subgrids,
                      static_cast<hipStream_t>(stream)),
                  "idg_subgrid_fft_launch");
}

int idg_adder_launch(int nr_subgrids, int grid_size, int subgrid_size,
                     int nr_w_layers, const idg_metadata_t *metadata,
                     const idg_cfloat_t *subgrids, idg_cfloat_t *grid,
                     void *stream) {
  if (nr_subgrids < 0 || subgrid_size <= 0 || subgrid_size % 2 ||
      grid_size < subgrid_size || nr_w_layers <= 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "even subgrid_size <= grid_size, nr_w_layers > 0 required");
  return from_hip(idg_mi355x::launch_adder(
                      nr_subgrids, grid_size, subgrid_size, nr_w_layers,
                      metadata, subgrids, grid,
                      static_cast<hipStream_t>(stream)),
                  "idg_adder_launch");
}

int idg_splitter_launch(int nr_subgrids, int grid_size, int subgrid_size,
                        int nr_w_layers, const idg_metadata_t *metadata,
                        const idg_cfloat_t *grid, idg_cfloat_t *subgrids,
                        void *stream) {
  if (nr_subgrids < 0 || subgrid_size <= 0 || subgrid_size % 2 ||
      grid_size < subgrid_size || nr_w_layers <= 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "even subgrid_size <= grid_size, nr_w_layers > 0 required");
  return from_hip(idg_mi355x::launch_splitter(
                      nr_subgrids, grid_size, subgrid_size, nr_w_layers,
                      metadata, grid, subgrids,
                      static_cast<hipStream_t>(stream)),
                  "idg_splitter_launch");
}

int idg_splitter_fft_launch(int nr_subgrids, int grid_size, int subgrid_size,
                            int nr_w_layers, const idg_metadata_t *metadata,
                            const idg_cfloat_t *grid, idg_cfloat_t *subgrids,
                            void *stream) {
  if (nr_subgrids < 0 || subgrid_size <= 0 || subgrid_size % 2 ||
      subgrid_size > 64 || grid_size < subgrid_size || nr_w_layers <= 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "even subgrid_size <= min(64, grid_size), nr_w_layers > 0 "
                "required");
  return from_hip(idg_mi355x::launch_splitter_fft(
                      nr_subgrids, grid_size, subgrid_size, nr_w_layers,
                      metadata, grid, subgrids,
                      static_cast<hipStream_t>(stream)),
                  "idg_splitter_fft_launch");
}

int idg_grid_fft_launch(int grid_size, int nr_planes, int sign, float scale,
                        idg_cfloat_t *planes, void *stream) {
  if (!idg_mi355x::grid_fft_supported(grid_size) || nr_planes < 0 ||
      (sign != 1 && sign != -1))
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_grid_fft_launch: grid_size a power of two in [64, 4096] "
                "(got " + std::to_string(grid_size) +
                    "), nr_planes >= 0, sign = +1 or -1");
  if (nr_planes > 0 && planes == nullptr)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_grid_fft_launch: null buffer");
  return from_hip(idg_mi355x::launch_grid_fft(
                      grid_size, nr_planes, sign, scale, planes,
                      static_cast<hipStream_t>(stream)),
                  "idg_grid_fft_launch");
}

namespace {
int check_image_step(const char *what, int grid_size, int nr_w_layers,
                     float image_size, const void *grid, const void *image) {
  if (!idg_mi355x::grid_fft_supported(grid_size) || nr_w_layers < 1 ||
      nr_w_layers > 16383 || !(image_size > 0.0f))
    return fail(IDG_E_INVALID_ARGUMENT,
                std::string(what) +
                    ": grid_size a power of two in [64, 4096] (got " +
                    std::to_string(grid_size) +
                    "), 1 <= nr_w_layers <= 16383, image_size > 0");
  if (grid == nullptr || image == nullptr)
    return fail(IDG_E_INVALID_ARGUMENT, std::string(what) + ": null buffer");
  return IDG_OK;
}
}  // namespace

int idg_grid_to_image_launch(int grid_size, int nr_w_layers, float image_size,
                             float w_step_in_lambda, const float *correction,
                             idg_cfloat_t *grid, idg_cfloat_t *image,
                             void *stream) {
  if (int rc = check_image_step("idg_grid_to_image_launch", grid_size,
                                nr_w_layers, image_size, grid, image))
    return rc;
  return from_hip(idg_mi355x::launch_grid_to_image(
                      grid_size, nr_w_layers, image_size, w_step_in_lambda,
                      correction, grid, image,
                      static_cast<hipStream_t>(stream)),
                  "idg_grid_to_image_launch");
}

int idg_image_to_grid_launch(int grid_size, int nr_w_layers, float image_size,
                             float w_step_in_lambda, const float *correction,
                             const idg_cfloat_t *image, idg_cfloat_t *grid,
                             void *stream) {
  if (int rc = check_image_step("idg_image_to_grid_launch", grid_size,
                                nr_w_layers, image_size, grid, image))
    return rc;
  return from_hip(idg_mi355x::launch_image_to_grid(
                      grid_size, nr_w_layers, image_size, w_step_in_lambda,
                      correction, image, grid,
                      static_cast<hipStream_t>(stream)),
                  "idg_image_to_grid_launch");
}

int idg_taper_to_image(int subgrid_size, int grid_size,
                       const float *spheroidal, double *out) {
  if (subgrid_size < 1 || grid_size < 1 || spheroidal == nullptr ||
      out == nullptr)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_taper_to_image: subgrid_size >= 1, grid_size >= 1 and "
                "non-null buffers required");
  idg_mi355x::host::taper_to_image(subgrid_size, grid_size, spheroidal, out);
  return IDG_OK;
}

int idg_c_run_gridder(int nr_subgrids, int grid_size, int subgrid_size,
                      float image_size, float w_step_in_lambda,
                      int nr_channels, int nr_stations, const idg_uvw_t *uvw,
                      size_t uvw_rows, const float *wavenumbers,
                      const idg_cfloat_t *visibilities,
                      const float *spheroidal, const idg_cfloat_t *aterms,
                      size_t aterm_slots, const idg_metadata_t *metadata,
                      idg_cfloat_t *subgrids) {
  return idg_c_run_gridder_opts(nr_subgrids, grid_size, subgrid_size,
                                image_size, w_step_in_lambda, nr_channels,
                                nr_stations, uvw, uvw_rows, wavenumbers,
                                visibilities, spheroidal, aterms, aterm_slots,
                                metadata, subgrids, nullptr);
}

int idg_c_run_gridder_opts(int nr_subgrids, int grid_size, int subgrid_size,
                           float image_size, float w_step_in_lambda,
                           int nr_channels, int nr_stations,
                           const idg_uvw_t *uvw, size_t uvw_rows,
                           const float *wavenumbers,
                           const idg_cfloat_t *visibilities,
                           const float *spheroidal, const idg_cfloat_t *aterms,
                           size_t aterm_slots, const idg_metadata_t *metadata,
                           idg_cfloat_t *subgrids,
                           const idg_options_t *options) {
  const auto p = make_problem(nr_subgrids, grid_size, subgrid_size,
                              image_size, w_step_in_lambda, nr_channels,
                              nr_stations);
  return run_host(idg_mi355x::Direction::kGridder, p, uvw_rows, aterm_slots,
                  uvw, wavenumbers, const_cast<idg_cfloat_t *>(visibilities),
                  spheroidal, aterms, metadata, subgrids, options);
}

int idg_c_run_degridder(int nr_subgrids, int grid_size, int subgrid_size,
                        float image_size, float w_step_in_lambda,
                        int nr_channels, int nr_stations,
                        const idg_uvw_t *uvw, size_t uvw_rows,
                        const float *wavenumbers, idg_cfloat_t *visibilities,
                        const float *spheroidal, const idg_cfloat_t *aterms,
                        size_t aterm_slots, const idg_metadata_t *metadata,
                        const idg_cfloat_t *subgrids) {
  return idg_c_run_degridder_opts(nr_subgrids, grid_size, subgrid_size,
                                  image_size, w_step_in_lambda, nr_channels,
                                  nr_stations, uvw, uvw_rows, wavenumbers,
                                  visibilities, spheroidal, aterms,
                                  aterm_slots, metadata, subgrids, nullptr);
}

int idg_c_run_degridder_opts(int nr_subgrids, int grid_size, int subgrid_size,
                             float image_size, float w_step_in_lambda,
                             int nr_channels, int nr_stations,
                             const idg_uvw_t *uvw, size_t uvw_rows,
                             const float *wavenumbers,
                             idg_cfloat_t *visibilities,
                             const float *spheroidal,
                             const idg_cfloat_t *aterms, size_t aterm_slots,
                             const idg_metadata_t *metadata,
                             const idg_cfloat_t *subgrids,
                             const idg_options_t *options) {
  const auto p = make_problem(nr_subgrids, grid_size, subgrid_size,
                              image_size, w_step_in_lambda, nr_channels,
                              nr_stations);
  return run_host(idg_mi355x::Direction::kDegridder, p, uvw_rows,
                  aterm_slots, uvw, wavenumbers, visibilities, spheroidal,
                  aterms, metadata, const_cast<idg_cfloat_t *>(subgrids),
                  options);
}

int idg_gridder_launch(int nr_subgrids, int grid_size, int subgrid_size,
                       float image_size, float w_step_in_lambda,
                       int nr_channels, int nr_stations, const idg_uvw_t *uvw,
                       const float *wavenumbers,
                       const idg_cfloat_t *visibilities,
                       const float *spheroidal, const idg_cfloat_t *aterms,
                       const idg_metadata_t *metadata, idg_cfloat_t *subgrids,
                       void *stream) {
  return idg_gridder_launch_opts(nr_subgrids, grid_size, subgrid_size,
                                 image_size, w_step_in_lambda, nr_channels,
                                 nr_stations, uvw, wavenumbers, visibilities,
                                 spheroidal, aterms, metadata, subgrids,
                                 stream, nullptr);
}

int idg_gridder_launch_opts(int nr_subgrids, int grid_size, int subgrid_size,
                            float image_size, float w_step_in_lambda,
                            int nr_channels, int nr_stations,
                            const idg_uvw_t *uvw, const float *wavenumbers,
                            const idg_cfloat_t *visibilities,
                            const float *spheroidal,
                            const idg_cfloat_t *aterms,
                            const idg_metadata_t *metadata,
                            idg_cfloat_t *subgrids, void *stream,
                            const idg_options_t *options) {
  const auto p = make_problem(nr_subgrids, grid_size, subgrid_size,
                              image_size, w_step_in_lambda, nr_channels,
                              nr_stations);
  return launch(idg_mi355x::Direction::kGridder, p, uvw, wavenumbers,
                const_cast<idg_cfloat_t *>(visibilities), spheroidal, aterms,
                metadata, subgrids, stream, options);
}

int idg_gridder_fft_launch(int nr_subgrids, int grid_size, int subgrid_size,
                           float image_size, float w_step_in_lambda,
                           int nr_channels, int nr_stations,
                           const idg_uvw_t *uvw, const float *wavenumbers,
                           const idg_cfloat_t *visibilities,
                           const float *spheroidal, const idg_cfloat_t *aterms,
                           const idg_metadata_t *metadata,
                           idg_cfloat_t *subgrids, void *stream) {
  return idg_gridder_fft_launch_opts(nr_subgrids, grid_size, subgrid_size,
                                     image_size, w_step_in_lambda, nr_channels,
                                     nr_stations, uvw, wavenumbers,
                                     visibilities, spheroidal, aterms,
                                     metadata, subgrids, stream, nullptr);
}

int idg_gridder_fft_launch_opts(int nr_subgrids, int grid_size,
                                int subgrid_size, float image_size,
                                float w_step_in_lambda, int nr_channels,
                                int nr_stations, const idg_uvw_t *uvw,
                                const float *wavenumbers,
                                const idg_cfloat_t *visibilities,
                                const float *spheroidal,
                                const idg_cfloat_t *aterms,
                                const idg_metadata_t *metadata,
                                idg_cfloat_t *subgrids, void *stream,
                                const idg_options_t *options) {
  if (subgrid_size > 64)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_gridder_fft_launch: subgrid_size <= 64 (the FFT's)");
  auto p = make_problem(nr_subgrids, grid_size, subgrid_size, image_size,
                        w_step_in_lambda, nr_channels, nr_stations);
  p.fft_out = true;
  return launch(idg_mi355x::Direction::kGridder, p, uvw, wavenumbers,
                const_cast<idg_cfloat_t *>(visibilities), spheroidal, aterms,
                metadata, subgrids, stream, options);
}

int idg_degridder_launch(int nr_subgrids, int grid_size, int subgrid_size,
                         float image_size, float w_step_in_lambda,
                         int nr_channels, int nr_stations,
                         const idg_uvw_t *uvw, const float *wavenumbers,
                         idg_cfloat_t *visibilities, const float *spheroidal,
                         const idg_cfloat_t *aterms,
                         const idg_metadata_t *metadata,
                         const idg_cfloat_t *subgrids, void *stream) {
  return idg_degridder_launch_opts(nr_subgrids, grid_size, subgrid_size,
                                   image_size, w_step_in_lambda, nr_channels,
                                   nr_stations, uvw, wavenumbers, visibilities,
                                   spheroidal, aterms, metadata, subgrids,
                                   stream, nullptr);
}

int idg_degridder_launch_opts(int nr_subgrids, int grid_size, int subgrid_size,
                              float image_size, float w_step_in_lambda,
                              int nr_channels, int nr_stations,
                              const idg_uvw_t *uvw, const float *wavenumbers,
                              idg_cfloat_t *visibilities,
                              const float *spheroidal,
                              const idg_cfloat_t *aterms,
                              const idg_metadata_t *metadata,
                              const idg_cfloat_t *subgrids, void *stream,
                              const idg_options_t *options) {
  const auto p = make_problem(nr_subgrids, grid_size, subgrid_size,
                              image_size, w_step_in_lambda, nr_channels,
                              nr_stations);
  return launch(idg_mi355x::Direction::kDegridder, p, uvw, wavenumbers,
                visibilities, spheroidal, aterms, metadata,
                const_cast<idg_cfloat_t *>(subgrids), stream, options);
}

int idg_validate_metadata(int nr_subgrids, int subgrid_size, int nr_channels,
                          int nr_stations, size_t uvw_rows, size_t aterm_slots,
                          const idg_metadata_t *metadata) {
  idg_mi355x::Problem p;
  p.nr_subgrids = nr_subgrids;
  p.subgrid_size = subgrid_size;
  p.nr_channels = nr_channels;
  p.nr_stations = nr_stations;
  if (int rc = check_geometry(p)) return rc;
  idg_mi355x::Extents e;
  e.uvw_rows = uvw_rows;
  e.aterm_slots = aterm_slots;
  const std::string msg = idg_mi355x::validate(
      p, e, reinterpret_cast<const idg::Metadata *>(metadata));
  if (!msg.empty()) return fail(IDG_E_OUT_OF_BOUNDS, msg);
  return IDG_OK;
}

int idg_host_chunk_plan(int nr_subgrids, const idg_metadata_t *metadata,
                        size_t bytes_moved, int *bounds, int max_bounds) {
  if (nr_subgrids <= 0 || metadata == nullptr)
    return fail(IDG_E_INVALID_ARGUMENT, "nr_subgrids <= 0 or null metadata");
  std::vector<int> sb;
  const int n = idg_mi355x::plan_host_chunks(
      reinterpret_cast<const idg::Metadata *>(metadata), nr_subgrids,
      bytes_moved, &sb, nullptr);
  if (bounds)
    for (int i = 0; i < static_cast<int>(sb.size()) && i < max_bounds; ++i)
      bounds[i] = sb[i];
  return n;
}

const char *idg_kernel_name(int direction, int subgrid_size, int nr_channels) {
  return idg_kernel_name_opts(direction, subgrid_size, nr_channels, nullptr);
}

const char *idg_kernel_name_opts(int direction, int subgrid_size,
                                 int nr_channels,
                                 const idg_options_t *options) {
  idg_mi355x::Options opt;
  if (parse_options(options, &opt)) return nullptr;
  idg_mi355x::Problem p;
  p.subgrid_size = subgrid_size;
  p.nr_channels = nr_channels;
  return direction == 0 ? idg_mi355x::select_gridder(p, opt).name
                        : idg_mi355x::select_degridder(p, opt).name;
}

int idg_precision_options(int direction, int subgrid_size, int nr_channels) {
  return idg_precision_options_opts(direction, subgrid_size, nr_channels,
                                    nullptr);
}

int idg_precision_options_opts(int direction, int subgrid_size,
                               int nr_channels, const idg_options_t *options) {
  idg_mi355x::Options opt;
  if (int rc = parse_options(options, &opt)) return rc;
  idg_mi355x::Problem p;
  p.subgrid_size = subgrid_size;
  p.nr_channels = nr_channels;
  return direction == 0 ? idg_mi355x::select_gridder(p, opt).prec
                        : idg_mi355x::select_degridder(p, opt).prec;
}

int idg_auto_selected(int nr_subgrids, int nr_channels,
                      const idg_options_t *options,
                      const idg_metadata_t *metadata, uint8_t *selected) {
  idg_mi355x::Options opt;
  if (int rc = parse_options(options, &opt)) return rc;
  if (nr_subgrids < 0 || nr_channels <= 0 ||
      (nr_subgrids > 0 && metadata == nullptr))
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_auto_selected: nr_subgrids >= 0, nr_channels > 0 and "
                "metadata required");
  const unsigned threshold =
      idg_mi355x::resolve_options(opt).auto_threshold;
  int count = 0;
  for (int s = 0; s < nr_subgrids; ++s) {
    const bool sel = idg_mi355x::auto_selects(metadata[s].nr_timesteps,
                                              nr_channels, threshold);
    if (selected) selected[s] = sel ? 1 : 0;
    count += sel ? 1 : 0;
  }
  return count;
}

int idg_plan(const idg_plan_params_t *params, int nr_baselines,
             int nr_timesteps, const uint32_t *baselines, const idg_uvw_t *uvw,
             int nr_channels, const float *wavenumbers,
             idg_metadata_t *metadata, int capacity, int32_t counts[2],
             int nthreads) {
  idg_mi355x::plan::Geometry g;
  float image_size = 0.0f, inv_w_step = 0.0f;
  if (int rc = parse_plan(params, nr_baselines, nr_timesteps, nr_channels,
                          capacity, &g, &image_size, &inv_w_step))
    return rc;
  if (int rc = plan_buffers("idg_plan", baselines, uvw, wavenumbers, metadata,
                            capacity, counts))
    return rc;
  idg_mi355x::host::plan(g, image_size, inv_w_step, nr_baselines,
                         nr_timesteps, nr_channels, baselines,
                         reinterpret_cast<const idg_mi355x::host::UVW *>(uvw),
                         wavenumbers,
                         reinterpret_cast<idg::Metadata *>(metadata), capacity,
                         counts, nthreads);
  return IDG_OK;
}

int idg_plan_launch(const idg_plan_params_t *params, int nr_baselines,
                    int nr_timesteps, const uint32_t *baselines,
                    const idg_uvw_t *uvw, int nr_channels,
                    const float *wavenumbers, idg_metadata_t *metadata,
                    int capacity, int32_t counts[2], void *stream) {
  idg_mi355x::plan::Geometry g;
  float image_size = 0.0f, inv_w_step = 0.0f;
  if (int rc = parse_plan(params, nr_baselines, nr_timesteps, nr_channels,
                          capacity, &g, &image_size, &inv_w_step))
    return rc;
  if (int rc = plan_buffers("idg_plan_launch", baselines, uvw, wavenumbers,
                            metadata, capacity, counts))
    return rc;
  return from_hip(idg_mi355x::launch_plan(
                      g, image_size, inv_w_step, nr_baselines, nr_timesteps,
                      nr_channels, baselines, uvw, wavenumbers, metadata,
                      capacity, counts, static_cast<hipStream_t>(stream)),
                  "idg_plan_launch");
}

int idg_weight_density(const idg_weight_params_t *params, int nr_subgrids,
                       int subgrid_size, int nr_channels,
                       const idg_metadata_t *metadata, const idg_uvw_t *uvw,
                       size_t uvw_rows, const float *wavenumbers,
                       const float *weights, uint64_t *density) {
  WeightCall call;
  if (int rc = parse_weight(params, nr_subgrids, subgrid_size, nr_channels,
                            &call))
    return rc;
  if (nr_subgrids == 0) return IDG_OK;
  if (int rc = density_buffers("idg_weight_density", metadata, uvw,
                               wavenumbers, weights, density))
    return rc;
  return from_host(idg_mi355x::host::weight_density(
      call.g, nr_subgrids, nr_channels,
      reinterpret_cast<const idg::Metadata *>(metadata),
      reinterpret_cast<const idg_mi355x::host::UVW *>(uvw), uvw_rows,
      wavenumbers, weights, density));
}

int idg_weight_density_launch(const idg_weight_params_t *params,
                              int nr_subgrids, int subgrid_size,
                              int nr_channels, const idg_metadata_t *metadata,
                              const idg_uvw_t *uvw, const float *wavenumbers,
                              const float *weights, uint64_t *density,
                              void *stream) {
  WeightCall call;
  if (int rc = parse_weight(params, nr_subgrids, subgrid_size, nr_channels,
                            &call))
    return rc;
  if (nr_subgrids == 0) return IDG_OK;
  if (int rc = density_buffers("idg_weight_density_launch", metadata, uvw,
                               wavenumbers, weights, density))
    return rc;
  return from_hip(idg_mi355x::launch_weight_density(
                      call.g, nr_subgrids, subgrid_size, nr_channels, metadata,
                      uvw, wavenumbers, weights, density,
                      static_cast<hipStream_t>(stream)),
                  "idg_weight_density_launch");
}

int idg_weight_scheme(const idg_weight_params_t *params,
                      const uint64_t *density, float ab[2]) {
  WeightCall call;
  if (int rc = parse_weight(params, 0, 1, 1, &call)) return rc;
  if (int rc = scheme_buffers("idg_weight_scheme", density, ab)) return rc;
  return from_host(idg_mi355x::host::weight_scheme(
      call.g, call.scheme, call.briggs_scale, density, ab));
}

int idg_weight_scheme_launch(const idg_weight_params_t *params,
                             const uint64_t *density, float ab[2],
                             void *stream) {
  WeightCall call;
  if (int rc = parse_weight(params, 0, 1, 1, &call)) return rc;
  if (int rc = scheme_buffers("idg_weight_scheme_launch", density, ab))
    return rc;
  return from_hip(idg_mi355x::launch_weight_scheme(
                      call.g, call.scheme, call.briggs_scale, density, ab,
                      static_cast<hipStream_t>(stream)),
                  "idg_weight_scheme_launch");
}

int idg_weight_apply(const idg_weight_params_t *params, int nr_subgrids,
                     int nr_channels, const idg_metadata_t *metadata,
                     const idg_uvw_t *uvw, size_t uvw_rows,
                     const float *wavenumbers, const float *weights,
                     const uint64_t *density, const float ab[2],
                     const idg_cfloat_t *visibilities, float *imaging_weights,
                     idg_cfloat_t *out, double *sum_weights) {
  WeightCall call;
  if (int rc = parse_weight(params, nr_subgrids, 1, nr_channels, &call))
    return rc;
  if (!sum_weights)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_weight_apply: null buffer");
  if (nr_subgrids == 0) {
    *sum_weights = 0.0;
    return IDG_OK;
  }
  if (!metadata || !uvw || !wavenumbers || !weights || !density || !ab ||
      !imaging_weights || !out)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_weight_apply: null buffer");
  return from_host(idg_mi355x::host::weight_apply(
      call.g, nr_subgrids, nr_channels,
      reinterpret_cast<const idg::Metadata *>(metadata),
      reinterpret_cast<const idg_mi355x::host::UVW *>(uvw), uvw_rows,
      wavenumbers, weights, density, ab,
      reinterpret_cast<const std::complex<float> *>(visibilities),
      imaging_weights, reinterpret_cast<std::complex<float> *>(out),
      sum_weights));
}

int idg_weight_apply_launch(const idg_weight_params_t *params, int nr_subgrids,
                            int nr_channels, const idg_metadata_t *metadata,
                            const idg_uvw_t *uvw, const float *wavenumbers,
                            const float *weights, const uint64_t *density,
                            const float ab[2],
                            const idg_cfloat_t *visibilities,
                            float *imaging_weights, idg_cfloat_t *out,
                            double *sum_weights, void *stream) {
  WeightCall call;
  if (int rc = parse_weight(params, nr_subgrids, 1, nr_channels, &call))
    return rc;
  if (!sum_weights ||
      (nr_subgrids > 0 && (!metadata || !uvw || !wavenumbers || !weights ||
                           !density || !ab || !imaging_weights || !out)))
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_weight_apply_launch: null buffer");
  if ((reinterpret_cast<uintptr_t>(visibilities) |
       reinterpret_cast<uintptr_t>(out)) % 16 != 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_weight_apply_launch: visibilities and out must be "
                "16-byte aligned");
  return from_hip(idg_mi355x::launch_weight_apply(
                      call.g, nr_subgrids, nr_channels, metadata, uvw,
                      wavenumbers, weights, density, ab, visibilities,
                      imaging_weights, out, sum_weights,
                      static_cast<hipStream_t>(stream)),
                  "idg_weight_apply_launch");
}

int idg_clean(const idg_clean_params_t *params, float *residual,
              const float *psf, const uint8_t *mask, float *model,
              idg_clean_component_t *components, idg_clean_state_t *state) {
  namespace cl = idg_mi355x::clean;
  cl::Params p;
  if (int rc = parse_clean(params, &p)) return rc;
  if (int rc = clean_buffers("idg_clean", residual, psf, model, components,
                             state))
    return rc;
  const std::string msg = idg_mi355x::host::clean(
      p, residual, psf, mask, model,
      reinterpret_cast<cl::Component *>(components),
      reinterpret_cast<cl::State *>(state));
  if (!msg.empty()) return fail(IDG_E_INVALID_ARGUMENT, msg);
  return IDG_OK;
}

int idg_clean_launch(const idg_clean_params_t *params, float *residual,
                     const float *psf, const uint8_t *mask, float *model,
                     idg_clean_component_t *components,
                     idg_clean_state_t *state, void *stream) {
  idg_mi355x::clean::Params p;
  if (int rc = parse_clean(params, &p)) return rc;
  if (int rc = clean_buffers("idg_clean_launch", residual, psf, model,
                             components, state))
    return rc;
  return from_hip(idg_mi355x::launch_clean(p, residual, psf, mask, model,
                                           components, state,
                                           static_cast<hipStream_t>(stream)),
                  "idg_clean_launch");
}

int idg_clark(const idg_clark_params_t *params, float *residual,
              const float *psf, const uint8_t *mask, float *model,
              idg_clean_component_t *components, idg_clark_state_t *state) {
  idg_mi355x::clark::Params p;
  if (int rc = parse_clark(params, &p)) return rc;
  if (int rc = clean_buffers("idg_clark", residual, psf, model, components,
                             state))
    return rc;
  const std::string msg = idg_mi355x::host::clark(
      p, residual, psf, mask, model,
      reinterpret_cast<idg_mi355x::clean::Component *>(components),
      reinterpret_cast<idg_mi355x::clark::State *>(state));
  if (!msg.empty()) return fail(IDG_E_INVALID_ARGUMENT, msg);
  return IDG_OK;
}

int idg_clark_launch(const idg_clark_params_t *params, float *residual,
                     const float *psf, const uint8_t *mask, float *model,
                     idg_clean_component_t *components,
                     idg_clark_state_t *state, void *stream) {
  idg_mi355x::clark::Params p;
  if (int rc = parse_clark(params, &p)) return rc;
  if (int rc = clean_buffers("idg_clark_launch", residual, psf, model,
                             components, state))
    return rc;
  return from_hip(idg_mi355x::launch_clark(p, residual, psf, mask, model,
                                           components, state,
                                           static_cast<hipStream_t>(stream)),
                  "idg_clark_launch");
}

int idg_beam_from_axes(double major, double minor, double pa,
                       idg_beam_t *beam) {
  idg_beam_t size_only;
  if (int rc = read_struct(beam, "idg_beam_t", &size_only)) return rc;
  idg_mi355x::host::Beam b;
  const std::string msg = idg_mi355x::host::beam_from_axes(major, minor, pa, &b);
  if (!msg.empty()) return fail(IDG_E_INVALID_ARGUMENT, msg);
  store_beam(b, beam);
  return IDG_OK;
}

int idg_beam_fit(int psf_size, const float *psf, float level,
                 idg_beam_t *beam) {
  idg_beam_t size_only;
  if (int rc = read_struct(beam, "idg_beam_t", &size_only)) return rc;
  if (psf == nullptr)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_beam_fit: null buffer");
  if (psf_size < 1 || !(level > 0.0f) || !(level < 1.0f))
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_beam_fit: psf_size >= 1 and 0 < level < 1 required");
  idg_mi355x::host::Beam b;
  const std::string msg = idg_mi355x::host::beam_fit(psf_size, psf, level, &b);
  if (!msg.empty()) return fail(IDG_E_INVALID_ARGUMENT, msg);
  store_beam(b, beam);
  return IDG_OK;
}

int idg_beam_radius(const idg_beam_t *beam, double cutoff) {
  idg_mi355x::host::Beam b;
  if (int rc = parse_beam(beam, "idg_beam_radius", &b)) return rc;
  if (!(cutoff > 0.0) || !(cutoff < 1.0))
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_beam_radius: 0 < cutoff < 1 required");
  const double reach = idg_mi355x::host::beam_reach(b, cutoff);
  if (!(reach <= idg_mi355x::restore::kMaxRadius))
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_beam_radius: the beam is above the cutoff beyond 32 "
                "pixels");
  return static_cast<int>(reach);
}

int idg_beam_taps(const idg_beam_t *beam, int radius, float *taps) {
  idg_mi355x::host::Beam b;
  if (int rc = parse_beam(beam, "idg_beam_taps", &b)) return rc;
  if (radius < 0 || radius > idg_mi355x::restore::kMaxRadius)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_beam_taps: 0 <= radius <= 32 required");
  if (taps == nullptr)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_beam_taps: null buffer");
  idg_mi355x::host::beam_taps(b, radius, taps);
  return IDG_OK;
}

int idg_restore(const idg_restore_params_t *params, const float *model,
                const float *residual, const float *taps, float *restored) {
  idg_mi355x::restore::Params p;
  if (int rc = parse_restore("idg_restore", params, model, residual, taps,
                             restored, &p))
    return rc;
  const int side = 2 * p.radius + 1;
  for (int i = 0; i < side * side; ++i)
    if (!std::isfinite(taps[i]))
      return fail(IDG_E_INVALID_ARGUMENT,
                  "idg_restore: tap " + std::to_string(i) + " is not finite");
  const std::string msg =
      idg_mi355x::host::restore(p, model, residual, taps, restored);
  if (!msg.empty()) return fail(static_cast<int>(hipErrorOutOfMemory), msg);
  return IDG_OK;
}

int idg_restore_launch(const idg_restore_params_t *params, const float *model,
                       const float *residual, const float *taps,
                       float *restored, void *stream) {
  idg_mi355x::restore::Params p;
  if (int rc = parse_restore("idg_restore_launch", params, model, residual,
                             taps, restored, &p))
    return rc;
  return from_hip(idg_mi355x::launch_restore(p, model, residual, taps,
                                             restored,
                                             static_cast<hipStream_t>(stream)),
                  "idg_restore_launch");
}

int idg_ms_scale_radius(double scale) {
  const int r = idg_mi355x::host::ms_scale_radius(scale);
  if (r < 0)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_ms_scale_radius: scale >= 0 with ceil(9 scale / 16) <= "
                "48 required");
  return r;
}

int idg_ms_scale_taps(double scale, int radius, float *taps) {
  const int r = idg_mi355x::host::ms_scale_radius(scale);
  if (r < 0 || r != radius)
    return fail(IDG_E_INVALID_ARGUMENT,
                "idg_ms_scale_taps: radius must be idg_ms_scale_radius(scale)");
  if (taps == nullptr)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_ms_scale_taps: null buffer");
  idg_mi355x::host::ms_scale_taps(scale, radius, taps);
  return IDG_OK;
}

int idg_convolve_separable(int grid_size, int radius, const float *in,
                           const float *taps, float *tmp, float *out) {
  if (int rc = parse_convolve("idg_convolve_separable", grid_size, radius, in,
                              taps, tmp, out))
    return rc;
  idg_mi355x::host::convolve_separable(grid_size, radius, in, taps, tmp, out);
  return IDG_OK;
}

int idg_convolve_separable_launch(int grid_size, int radius, const float *in,
                                  const float *taps, float *tmp, float *out,
                                  void *stream) {
  if (int rc = parse_convolve("idg_convolve_separable_launch", grid_size,
                              radius, in, taps, tmp, out))
    return rc;
  return from_hip(idg_mi355x::launch_convolve_separable(
                      grid_size, radius, in, taps, tmp, out,
                      static_cast<hipStream_t>(stream)),
                  "idg_convolve_separable_launch");
}

int idg_ms_prepare(const idg_ms_params_t *params, const float *residual,
                   const float *psf, const float *taps, float *planes,
                   float *cross_psf, float *tmp) {
  idg_mi355x::ms::Params p;
  if (int rc = parse_ms(params, false, &p)) return rc;
  if (int rc = ms_prepare_buffers("idg_ms_prepare", p, residual, psf, taps,
                                  planes, cross_psf, tmp))
    return rc;
  idg_mi355x::host::ms_prepare(p, residual, psf, taps, planes, cross_psf, tmp);
  return IDG_OK;
}

int idg_ms_prepare_launch(const idg_ms_params_t *params, const float *residual,
                          const float *psf, const float *taps, float *planes,
                          float *cross_psf, float *tmp, void *stream) {
  idg_mi355x::ms::Params p;
  if (int rc = parse_ms(params, false, &p)) return rc;
  if (int rc = ms_prepare_buffers("idg_ms_prepare_launch", p, residual, psf,
                                  taps, planes, cross_psf, tmp))
    return rc;
  return from_hip(idg_mi355x::launch_ms_prepare(
                      p, residual, psf, taps, planes, cross_psf, tmp,
                      static_cast<hipStream_t>(stream)),
                  "idg_ms_prepare_launch");
}

int idg_ms_clean(const idg_ms_params_t *params, float *planes,
                 const float *cross_psf, const float *taps,
                 const uint8_t *mask, float *model,
                 idg_ms_component_t *components, idg_ms_state_t *state) {
  namespace ms = idg_mi355x::ms;
  ms::Params p;
  if (int rc = parse_ms(params, true, &p)) return rc;
  if (int rc = ms_clean_buffers("idg_ms_clean", p, planes, cross_psf, taps,
                                mask, model, components, state))
    return rc;
  const std::string msg = idg_mi355x::host::ms_clean(
      p, planes, cross_psf, taps, mask, model,
      reinterpret_cast<ms::Component *>(components),
      reinterpret_cast<ms::State *>(state));
  if (!msg.empty()) return fail(IDG_E_INVALID_ARGUMENT, msg);
  return IDG_OK;
}

int idg_ms_clean_launch(const idg_ms_params_t *params, float *planes,
                        const float *cross_psf, const float *taps,
                        const uint8_t *mask, float *model,
                        idg_ms_component_t *components, idg_ms_state_t *state,
                        void *stream) {
  idg_mi355x::ms::Params p;
  if (int rc = parse_ms(params, true, &p)) return rc;
  if (int rc = ms_clean_buffers("idg_ms_clean_launch", p, planes, cross_psf,
                                taps, mask, model, components, state))
    return rc;
  return from_hip(idg_mi355x::launch_ms_clean(
                      p, planes, cross_psf, taps, mask, model, components,
                      state, static_cast<hipStream_t>(stream)),
                  "idg_ms_clean_launch");
}

double idg_p_run_gridder(void) {
  idg_mi355x::Problem p;
  p.subgrid_size = static_cast<int>(get_env_var("SUBGRID_SIZE", 32));
  p.nr_channels = static_cast<int>(get_env_var("NR_CHANNELS", 16));
  const auto k = idg_mi355x::select_gridder(p);
  return 1e3 * idg_mi355x::run_performance(idg_mi355x::Direction::kGridder,
                                           k.func, "gridder_mi355x", k.block);
}

double idg_p_run_degridder(void) {
  idg_mi355x::Problem p;
  p.subgrid_size = static_cast<int>(get_env_var("SUBGRID_SIZE", 32));
  p.nr_channels = static_cast<int>(get_env_var("NR_CHANNELS", 16));
  // the batch run_performance builds (the kernel choice depends on its size)
  const int nr_stations = static_cast<int>(get_env_var("NR_STATIONS", 50));
  p.nr_subgrids = nr_stations * (nr_stations - 1) / 2 *
                  static_cast<int>(get_env_var("NR_TIMESLOTS", 20));
  const auto k = idg_mi355x::select_degridder(p);
  return 1e3 * idg_mi355x::run_performance(idg_mi355x::Direction::kDegridder,
                                           k.func, "degridder_mi355x",
                                           k.block);
}

void idg_print_device_info(void) { hip::print_device_info(); }
void idg_print_benchmark(void) { hip::print_benchmark(); }

int idg_get_device_name(char *buf, size_t len) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(IDG_E_NO_DEVICE, "no HIP device");
  const std::string name = hip::extern_get_device_name();
  if (buf && len) {
    std::strncpy(buf, name.c_str(), len - 1);
    buf[len - 1] = '\0';
  }
  return static_cast<int>(name.size());
}

uint64_t idg_flops_gridder(uint64_t nr_channels, uint64_t nr_timesteps,
                           uint64_t nr_subgrids, uint64_t subgrid_size,
                           uint64_t nr_correlations) {
  return flops_gridder(nr_channels, nr_timesteps, nr_subgrids, subgrid_size,
                       nr_correlations);
}

uint64_t idg_bytes_gridder(uint64_t nr_channels, uint64_t nr_timesteps,
                           uint64_t nr_subgrids, uint64_t subgrid_size,
                           uint64_t nr_correlations) {
  return bytes_gridder(nr_channels, nr_timesteps, nr_subgrids, subgrid_size,
                       nr_correlations);
}

int idg_generate(int nr_stations, int nr_timeslots, int nr_timesteps,
                 int nr_channels, int grid_size, int subgrid_size,
                 idg_uvw_t *uvw, float *frequencies, float *wavenumbers,
                 idg_cfloat_t *visibilities, float *spheroidal,
                 idg_cfloat_t *aterms, idg_metadata_t *metadata,
                 idg_cfloat_t *subgrids, int nthreads) {
  if (nr_stations < 2 || nr_timeslots < 1 || nr_timesteps < 1 ||
      nr_channels < 1 || grid_size < 1 || subgrid_size < 1)
    return fail(IDG_E_INVALID_ARGUMENT, "idg_generate: bad parameters");
  using UVW = idg::UVWCoordinate<float>;
  using Vis = idg::Visibility<std::complex<float>>;
  using Jones = idg::Matrix2x2<std::complex<float>>;
  const int nbl = nr_stations * (nr_stations - 1) / 2;
  const int ns = nbl * nr_timeslots;
  const size_t S = static_cast<size_t>(subgrid_size);
  // Caller buffers where given, owned temporaries otherwise (every generator
  // still runs, so the rand() stream is consumed exactly as the harness does).
  std::vector<UVW> t_uvw(uvw ? 0 : static_cast<size_t>(ns) * nr_timesteps);
  std::vector<float> t_f(frequencies ? 0 : nr_channels),
      t_wn(wavenumbers ? 0 : nr_channels), t_sph(spheroidal ? 0 : S * S);
  std::vector<Jones> t_at(aterms ? 0 : nr_timeslots * nr_stations * S * S);
  std::vector<idg::Metadata> t_md(metadata ? 0 : ns);
  UVW *p_uvw = uvw ? reinterpret_cast<UVW *>(uvw) : t_uvw.data();
  float *p_f = frequencies ? frequencies : t_f.data();
  float *p_wn = wavenumbers ? wavenumbers : t_wn.data();
  float *p_sph = spheroidal ? spheroidal : t_sph.data();
  Jones *p_at = aterms ? reinterpret_cast<Jones *>(aterms) : t_at.data();
  idg::Metadata *p_md =
      metadata ? reinterpret_cast<idg::Metadata *>(metadata) : t_md.data();

  idg::Array2D<UVW> a_uvw(p_uvw, ns, nr_timesteps);
  idg::Array1D<float> a_f(p_f, nr_channels), a_wn(p_wn, nr_channels);
  idg::Array1D<idg::Baseline> a_bl(nbl);
  idg::Array2D<float> a_sph(p_sph, subgrid_size, subgrid_size);
  idg::Array4D<Jones> a_at(p_at, nr_timeslots, nr_stations, subgrid_size,
                           subgrid_size);
  idg::Array1D<idg::Metadata> a_md(p_md, ns);

  srand(0);
  initialize_uvw(grid_size, a_uvw);
  initialize_frequencies(a_f);
  initialize_wavenumbers(a_f, a_wn);
  if (visibilities) {
    // Row-parallel: this generator draws no random numbers.
    const int nt = std::max(1, std::min(nthreads, ns));
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; ++w) {
      const int r0 = static_cast<int>(static_cast<long long>(ns) * w / nt);
      const int r1 = static_cast<int>(static_cast<long long>(ns) * (w + 1) / nt);
      if (r1 <= r0) continue;
      pool.emplace_back([&a_f, p_uvw, visibilities, grid_size, nr_timesteps,
                         nr_channels, r0, r1]() {
        idg::Array2D<UVW> u(p_uvw + static_cast<size_t>(r0) * nr_timesteps,
                            r1 - r0, nr_timesteps);
        idg::Array3D<Vis> v(
            reinterpret_cast<Vis *>(visibilities) +
                static_cast<size_t>(r0) * nr_timesteps * nr_channels,
            r1 - r0, nr_timesteps, nr_channels);
        initialize_visibilities(grid_size, IMAGE_SIZE, a_f, u, v);
      });
    }
    for (auto &th : pool) th.join();
  }
  initialize_baselines(nr_stations, a_bl);
  initialize_spheroidal(a_sph);
  initialize_aterms(a_sph, a_at);
  if (subgrids) {
    idg::Array4D<std::complex<float>> a_sg(
        reinterpret_cast<std::complex<float> *>(subgrids), ns, 4,
        subgrid_size, subgrid_size);
    initialize_subgrids(a_sg);
  }
  initialize_metadata(grid_size, nr_timeslots, nr_timesteps, a_bl, a_md);
  return ns;
}

}  // extern "C"
