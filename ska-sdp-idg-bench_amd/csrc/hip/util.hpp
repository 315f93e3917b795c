// util.hpp -- the HIP launch-and-buffer layer.
//
// Keeps the reference's app/HIP/util.hpp:13-63 API (p_run_kernel,
// c_run_kernel, p_run_gridder_ / c_run_gridder_, p_run_degridder_ /
// c_run_degridder_, device queries) so a kernel TU written against the
// reference drops in here and vice versa.  Differences, all deliberate:
//   * sizes are size_t end to end (the reference's int products overflow at
//     nr_channels = 256, util.cpp:220-231);
//   * every HIP call is checked; metadata is validated against the buffer
//     sizes on the host before any launch (a bad index would fault the GPU);
//   * the perf entry uploads real synthetic inputs (the reference times
//     kernels on uninitialised memory, util.cpp:234-235);
//   * launches go to an explicit stream (nullptr = legacy default stream).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "lib-common.hpp"

namespace hip {

// Aborts the process on error, as the reference's hipCheck does
// (util.cpp:5-15).
#define hipCheck(ans) ::hip::hip_assert((ans), __FILE__, __LINE__)
void hip_assert(hipError_t code, const char *file, int line, bool abort = true);

std::string get_device_name();
void print_device_info();
std::vector<int> get_launch_kernel_dimensions();
int get_cu_nr();
int get_max_threads();
size_t get_gmem_size();
int get_cu_freq();
void print_dimensions(dim3 gridDim, dim3 blockDim);

// Warm-up + event-timed loop of NR_ITERATIONS launches, then report() and
// report_csv() (reference util.cpp:81-165).  Returns seconds per launch.
double p_run_kernel(const void *func, dim3 gridDim, dim3 blockDim,
                    void **args, std::string func_name = "",
                    double gflops = 0, double gbytes = 0, double mvis = 0);

// One launch (reference util.cpp:167-174).
void c_run_kernel(const void *func, dim3 gridDim, dim3 blockDim, void **args);

void p_run_gridder_(const void *func, std::string func_name, int num_threads);

void c_run_gridder_(
    int nr_subgrids, int grid_size, int subgrid_size, float image_size,
    float w_step_in_lambda, int nr_channels, int nr_stations,
    idg::Array2D<idg::UVWCoordinate<float>> &uvw,
    idg::Array1D<float> &wavenumbers,
    idg::Array3D<idg::Visibility<std::complex<float>>> &visibilities,
    idg::Array2D<float> &spheroidal,
    idg::Array4D<idg::Matrix2x2<std::complex<float>>> &aterms,
    idg::Array1D<idg::Metadata> &metadata,
    idg::Array4D<std::complex<float>> &subgrids, const void *func,
    int num_threads);

void p_run_degridder_(const void *func, std::string func_name,
                      int num_threads);

void c_run_degridder_(
    int nr_subgrids, int grid_size, int subgrid_size, float image_size,
    float w_step_in_lambda, int nr_channels, int nr_stations,
    idg::Array2D<idg::UVWCoordinate<float>> &uvw,
    idg::Array1D<float> &wavenumbers,
    idg::Array3D<idg::Visibility<std::complex<float>>> &visibilities,
    idg::Array2D<float> &spheroidal,
    idg::Array4D<idg::Matrix2x2<std::complex<float>>> &aterms,
    idg::Array1D<idg::Metadata> &metadata,
    idg::Array4D<std::complex<float>> &subgrids, const void *func,
    int num_threads);

void print_benchmark();

}  // namespace hip

// ---------------------------------------------------------------------------
// MI355X runtime: kernel selection, validation and raw-pointer pipelines.
// Used by the kernel TUs, by util.cpp and by the C ABI (capi/idg_capi.cpp);
// the host twins of launch_plan, _weight_*, _clean, _clark and _restore are in
// host/host.hpp.
// ---------------------------------------------------------------------------
namespace idg_mi355x {

enum class Direction { kGridder = 0, kDegridder = 1 };

// Geometry of one gridder/degridder call; the 13-argument kernel ABI of the
// reference carries the same values.
struct Problem {
  int nr_subgrids = 0;
  int grid_size = 0;
  int subgrid_size = 0;
  float image_size = IMAGE_SIZE;
  float w_step_in_lambda = W_STEP;
  int nr_channels = 0;
  int nr_stations = 0;
  // gridder only: the output subgrids are their 2-D FFT (sign +1, scale 1),
  // as launch_subgrid_fft(+1, 1) after the plain gridder would make them
  // (in the kernel's epilogue where KernelChoice::fft_in_kernel, else a
  // launch_subgrid_fft after it)
  bool fft_out = false;
};

// Which kernels one call runs (include/idg_mi355x.h idg_options_t, the same
// numbers).  As a request every field may be 0 = unset; resolve_options()
// fills the unset ones from the environment -- the only place IDG_GRIDDER_IMPL,
// IDG_DEGRIDDER_IMPL, IDG_PREC, IDG_KERNEL_FORM and IDG_GRID_FFT are read --
// and marks the value resolved.  A default-constructed Options is therefore
// the environment route, which is what every entry without options takes.
constexpr int kImplDefault = 1, kImplValu = 2, kImplSequential = 3,
              kImplOrdered = 4, kImplAuto = 5;
constexpr int kPrecSet = 8;  // precision = kPrecSet | bits
constexpr int kFormCombined = 1, kFormSplit = 2,
              kFormBySize = 3;  // resolved only: split from kTwoKernelMinLaunch
constexpr int kFftFusionOff = 1, kFftFusionOn = 2;
constexpr unsigned kAutoThreshold = 16384;
struct Options {
  int gridder_impl = 0;    // kImpl*
  int degridder_impl = 0;  // kImplDefault / kImplValu (by environment only) /
                           // kImplSequential
  int precision = 0;       // kPrecSet | bits; resolved and still 0: the
                           // library's choice for the problem (precision_for)
  int kernel_form = 0;     // kForm*
  int fft_fusion = 0;      // kFftFusion*
  unsigned auto_threshold = 0;  // kImplAuto: ordered above this T x C
  bool resolved = false;
};
Options resolve_options(const Options &request);

// Buffer extents used for host-side validation (element counts).
struct Extents {
  size_t uvw_rows = 0;      // UVW triplets (= visibility rows)
  size_t aterm_slots = 0;   // leading dimension of aterms (timeslots)
};

struct KernelChoice {
  // one kernel that handles every subgrid (__global__, 13-argument ABI,
  // grid = nr_subgrids): the reference's launch shape, used by the perf
  // entries and for caller-supplied kernels
  const void *func = nullptr;
  const char *name = "";
  int block = 256;
  int grid = 0;  // = nr_subgrids
  bool fft_in_kernel = false;  // Problem::fft_out done by these kernels
  int prec = 0;  // precision options of the MFMA kernels (device.hpp kPrec*)
  // kImplAuto: the kernels above are the default (MFMA) pass, run on a shadow
  // metadata in which the subgrids above auto_threshold are empty; the
  // queue-fed ordered kernel then writes those (launch_auto_gridder)
  bool auto_ordered = false;
  unsigned auto_threshold = 0;
  // The launch the device entries make instead, when parts[1] is set: one
  // kernel per subgrid class, each with the register allocation of its own
  // path.  parts[0] (kMirror; absent for odd S): grid =
  // nr_subgrids, the 13-argument ABI plus `int *queue`; it takes the
  // mirror-eligible subgrids and queues the others.  parts[1] (kGeneral): a
  // resident grid (occupancy x CUs, at most nr_subgrids), the 13 arguments
  // plus (int *queue, int nr_subgrids, int all); it takes the queued
  // subgrids (all of them with `all` set and no mirror launch).  queue:
  // device.hpp queue_ints(nr_subgrids) ints of stream-ordered workspace.
  // When no subgrid can be mirror-eligible (odd S, or w_step_in_lambda !=
  // 0), all_general is launched instead, once: grid = nr_subgrids, the
  // 13-argument ABI, one workgroup per subgrid on the general path.
  enum Kind { kPlain = 0, kMirror = 1, kGeneral = 2 };
  struct Part {
    const void *func = nullptr;
    int block = 0;
    int kind = kPlain;
    int per_subgrid = 1;  // workgroups per subgrid (mirror part: grid x)
  } parts[2], all_general;
};

// The two-kernel launch of `k` (k.parts[1].func set) on `stream`; args13 is
// the 13-argument kernel ABI.  all_general: no subgrid can be
// mirror-eligible (w_step_in_lambda != 0), so the mirror launch is skipped.
hipError_t launch_parts(const KernelChoice &k, int nr_subgrids, void **args13,
                        bool all_general, hipStream_t stream);

// A device workspace cached per (device, stream, slot) (util.cpp), leased
// for the enqueueing of one launch sequence on `stream`: ptr holds at least
// the bytes asked for; `clean` = the last lease of this slot ended with
// leave_clean set (its contents are what that sequence left).  While another
// host thread holds the slot, ptr is a private stream-ordered allocation
// (never clean) freed after the sequence.
constexpr int kWorkspaceQueue = 0, kWorkspaceHomeSort = 1,
              kWorkspaceAdderSeg = 2, kWorkspaceAuto = 3, kWorkspacePlan = 4,
              kWorkspaceWeight = 5, kWorkspaceClean = 6,
              kWorkspaceMultiscale = 7, kWorkspaceClark = 8;
// Not copyable: a copy would release the slot twice.
struct WorkspaceLease {
  void *ptr = nullptr;
  hipStream_t stream = nullptr;
  bool clean = false;
  bool leave_clean = false;
  WorkspaceLease() = default;
  WorkspaceLease(const WorkspaceLease &) = delete;
  WorkspaceLease &operator=(const WorkspaceLease &) = delete;
  hipError_t acquire(hipStream_t s, int slot, size_t bytes);
  ~WorkspaceLease();

 private:
  int dev_ = 0, slot_ = 0;
  bool private_ = false;
};

// Frees the cached workspaces of `stream` on the current device (all = true:
// of every stream of the current device).  The stream(s) must be idle: call
// it before destroying a stream the entries have used (a new stream may get
// the same handle) and before hipDeviceReset.  A slot leased at the moment
// (another host thread enqueueing on it) is left alone and reported as
// hipErrorNotReady.  idg_release_workspaces in the C ABI.
hipError_t release_workspaces(hipStream_t stream, bool all);

// Whether the device entries launch the two-kernel form (mirror kernel +
// queue-fed general kernel) or the one combined kernel: the two-kernel form
// from kTwoKernelMinLaunch subgrids up.  Below that (the N >= 4 shards of
// the batch) its fixed cost -- the queue's allocation and clear and a second
// launch, ~15 us per direction -- outweighs what the mirror kernel's own
// register allocation saves (one-GPU shard rehearsal at N = 8: 0.953 with
// it, 0.969 without).  Options::kernel_form (IDG_KERNEL_FORM=combined /
// split) forces either.
constexpr int kTwoKernelMinLaunch = 8192;
bool two_kernel_form(int nr_subgrids, const Options &opt = Options());

// Precision options (device.hpp kPrecTail | kPrecFlush | kPrecTailAlt) of
// the MFMA kernels for a launch: the gridder takes
// the reduction tail on every phasor (kPrecTail; round 6, was kPrecTailAlt,
// one channel per quad, until channel-incoherent data showed it losing to the
// reference's own f32 sum) and, above
// kTailMinChannels channels, blocked summation (kPrecFlush: C = 256 gridder
// 8.4e-6 -> 2.0e-6 from exact accumulation); the degridder no tail.
// Options::precision (IDG_PREC=<0..7>) forces the bits for both directions.
constexpr int kTailMinChannels = 16;
int precision_for(Direction dir, const Problem &p,
                  const Options &opt = Options());

// The kernels are built for S = 32, S = 64 and a runtime S (template argument
// 0).  kernel_for_size: pick(std::integral_constant<int, 32 | 64 | 0>) for a
// subgrid size, pick returning the address of that instantiation.
template <typename Pick>
const void *kernel_for_size(int subgrid_size, Pick pick) {
  switch (subgrid_size) {
    case 32: return pick(std::integral_constant<int, 32>{});
    case 64: return pick(std::integral_constant<int, 64>{});
    default: return pick(std::integral_constant<int, 0>{});
  }
}
// The matching kernel name, prefix "_s32" / "_s64" / "_generic": string
// literals, because idg_kernel_name hands the pointer out.
#define IDG_SIZE_NAME(prefix, subgrid_size)   \
  ((subgrid_size) == 32   ? prefix "_s32"     \
   : (subgrid_size) == 64 ? prefix "_s64"     \
                          : prefix "_generic")

// Defined in the kernel TUs.
KernelChoice select_gridder(const Problem &p, const Options &opt = Options());
KernelChoice select_degridder(const Problem &p,
                              const Options &opt = Options());

// The order-preserving kernels (kernels/sequential_mi355x.hip.cpp): the
// reference CPU path's rounding sequence, bit for bit; 13-argument ABI, grid
// = nr_subgrids, block = sequential_block().  Selected per call by
// Options kImplSequential (IDG_GRIDDER_IMPL / IDG_DEGRIDDER_IMPL=sequential).
const void *sequential_gridder(int subgrid_size);
const void *sequential_degridder(int subgrid_size);
int sequential_block();

// The ordered gridder (kernels/ordered_mi355x.hip.cpp): the reference's
// summation order and product forms with the hardware sin / cos of the MFMA
// kernels -- within the reference's 1e-5 bar at any T x C, not bit-exact;
// same ABI and launch shape.  Options kImplOrdered (IDG_GRIDDER_IMPL=ordered).
const void *ordered_gridder(int subgrid_size);
int ordered_block();

// The auto gridder (Options::gridder_impl = kImplAuto), three
// stream-ordered steps with no device-to-host copy and no cross-workgroup
// wait; kernel boundaries order them.  `ws` is auto_workspace_bytes() of
// workspace: a count, a queue of subgrid indices and a shadow metadata.
//   launch_auto_classify: one thread per subgrid; subgrids with nr_timesteps
//     x nr_channels > threshold (64-bit product) are pushed to the queue and
//     get nr_timesteps = 0 in the shadow copy, the others are copied as is.
//   (the caller runs the default gridder on auto_shadow(ws))
//   launch_ordered_queue: the ordered kernel over the queue, true metadata;
//     `slices` workgroups per queued subgrid, each taking a contiguous range
//     of whole pixels (a pixel's (t, c) sum is never split, so the bits are
//     the ordered kernel's).  Grid = nr_subgrids x slices: the host does not
//     know the count; workgroups past it return at once.
// kAutoSlices: the slicing the launch layer uses (IDG_AUTO_SLICES, a
// measurement knob, overrides it).
size_t auto_workspace_bytes(int nr_subgrids);
const void *auto_shadow(void *ws, int nr_subgrids);
hipError_t launch_auto_classify(int nr_subgrids, int nr_channels,
                                unsigned threshold, const void *d_metadata,
                                void *ws, hipStream_t stream);
hipError_t launch_ordered_queue(const Problem &p, void **args13, void *ws,
                                int slices, hipStream_t stream);
constexpr int kAutoSlices = 2;
// Host twin of the classification.
bool auto_selects(long long nr_timesteps, long long nr_channels,
                  unsigned threshold);

// The plan step on the device (kernels/plan_mi355x.hip.cpp):
// uvw rows of nr_baselines x nr_timesteps -> metadata records, bit for bit
// the host walk of common/plan.hpp.  Three stream-ordered launches (count per
// baseline, scan, fill) on a kWorkspacePlan lease of plan_workspace_bytes();
// nothing is read back.  `geometry` carries the integer parameters (its
// scales are set on the device from d_wavenumbers); d_counts receives
// {subgrids needed, dropped timesteps}; records past `capacity` are not
// written.
namespace plan {
struct Geometry;
}
size_t plan_workspace_bytes(int nr_baselines);
hipError_t launch_plan(const plan::Geometry &geometry, float image_size,
                       float inv_w_step, int nr_baselines, int nr_timesteps,
                       int nr_channels, const void *d_baselines,
                       const void *d_uvw, const float *d_wavenumbers,
                       void *d_metadata, int capacity, void *d_counts,
                       hipStream_t stream);

// Imaging weights on the device (kernels/weight_mi355x.hip.cpp; DESIGN.md
// §14), bit for bit the host entries of common/weight.hpp's arithmetic.
// launch_weight_density adds the covered samples' quantised weights onto
// d_density ([G][G] uint64; integer atomics, so the bits do not depend on any
// order); launch_weight_scheme writes (a, b) of a scheme (weight::kNatural /
// kUniform / kBriggs; briggs_scale = (5 * 10^-robust)^2) to d_ab from fixed-
// order sums over the cells; launch_weight_apply writes the imaging weights,
// the weighted visibilities (d_visibilities null: (f, 0, 0, f); d_out may be
// d_visibilities; both 16-byte aligned) and *d_sum_weights for every covered
// sample.  The partials of the two sums live on a kWorkspaceWeight lease;
// nothing is read back.
namespace weight {
struct Geometry;
}
hipError_t launch_weight_density(const weight::Geometry &geometry,
                                 int nr_subgrids, int subgrid_size,
                                 int nr_channels, const void *d_metadata,
                                 const void *d_uvw, const float *d_wavenumbers,
                                 const float *d_weights, void *d_density,
                                 hipStream_t stream);
hipError_t launch_weight_scheme(const weight::Geometry &geometry, int scheme,
                                double briggs_scale, const void *d_density,
                                float *d_ab, hipStream_t stream);
hipError_t launch_weight_apply(const weight::Geometry &geometry,
                               int nr_subgrids, int nr_channels,
                               const void *d_metadata, const void *d_uvw,
                               const float *d_wavenumbers,
                               const float *d_weights, const void *d_density,
                               const float *d_ab, const void *d_visibilities,
                               float *d_imaging_weights, void *d_out,
                               double *d_sum_weights, hipStream_t stream);

// The Hogbom minor cycle on the device (kernels/clean_mi355x.hip.cpp over the
// shared body of kernels/minor_cycle.hpp), bit for bit the
// host entry of common/clean.hpp's arithmetic: one
// search launch, params.nr_iterations iteration launches (each subtracts one
// component and searches for the next in the same pass) and one finish launch,
// continuing from *d_state (clean::State) and leaving it there.  The tiles'
// partials and the double-buffered state live on a kWorkspaceClean lease;
// nothing is read back.  d_mask may be null; d_components: clean::Component
// [params.max_components].
namespace clean {
struct Params;
}
hipError_t launch_clean(const clean::Params &params, float *d_residual,
                        const float *d_psf, const uint8_t *d_mask,
                        float *d_model, void *d_components, void *d_state,
                        hipStream_t stream);

// Multi-scale CLEAN on the device (kernels/multiscale_mi355x.hip.cpp; DESIGN.md
// §17), bit for bit the host entries of common/multiscale.hpp's arithmetic.
// launch_convolve_separable: the row pass into d_tmp and the column pass into
// d_out (which may be d_in), two launches, no workspace.  launch_ms_prepare:
// the scale planes and the cross-PSFs, launches of those two passes and one
// device-to-device copy.  launch_ms_clean (the shared body of
// kernels/minor_cycle.hpp under ms::Cycle): one search launch,
// params.base.nr_iterations iteration launches and one finish launch,
// continuing from *d_state (ms::State) and leaving it there; the tiles'
// partials and the double-buffered state live on a kWorkspaceMultiscale
// lease.  Nothing is read back.  d_taps: every scale's taps, one after the
// other; d_mask may be null; d_components: ms::Component
// [params.base.max_components].
namespace ms {
struct Params;
}
hipError_t launch_convolve_separable(int grid_size, int radius,
                                     const float *d_in, const float *d_taps,
                                     float *d_tmp, float *d_out,
                                     hipStream_t stream);
hipError_t launch_ms_prepare(const ms::Params &params, const float *d_residual,
                             const float *d_psf, const float *d_taps,
                             float *d_planes, float *d_cross_psf, float *d_tmp,
                             hipStream_t stream);
hipError_t launch_ms_clean(const ms::Params &params, float *d_planes,
                           const float *d_cross_psf, const float *d_taps,
                           const uint8_t *d_mask, float *d_model,
                           void *d_components, void *d_state,
                           hipStream_t stream);

// Clark CLEAN on the device (kernels/clark_mi355x.hip.cpp), bit
// for bit the host entry of common/clark.hpp's arithmetic: params.nr_rounds
// rounds of five launches each (histogram and peak, limit, compaction, the
// one-workgroup minor cycle on the candidate list, apply) between a begin
// launch and a search and a finish launch, continuing from *d_state
// (clark::State) and leaving it there.  The partials, the histogram, the
// candidate list and the state live on a kWorkspaceClark lease; nothing is
// read back.  d_mask may be null; d_components: clean::Component
// [params.base.max_components].
namespace clark {
struct Params;
}
hipError_t launch_clark(const clark::Params &params, float *d_residual,
                        const float *d_psf, const uint8_t *d_mask,
                        float *d_model, void *d_components, void *d_state,
                        hipStream_t stream);

// The restore step on the device (kernels/restore_mi355x.hip.cpp; DESIGN.md
// §16), bit for bit the host entry of common/restore.hpp's arithmetic: one
// launch, one workgroup per tile, no workspace; nothing is read back.
// d_residual may be null, and d_restored may be d_residual.
namespace restore {
struct Params;
}
hipError_t launch_restore(const restore::Params &params, const float *d_model,
                          const float *d_residual, const float *d_taps,
                          float *d_restored, hipStream_t stream);

// Returns an empty string if every subgrid's time range, stations and A-term
// slot lie inside the buffers, else a description of the first violation.
std::string validate(const Problem &p, const Extents &e,
                     const idg::Metadata *metadata);

// Asynchronous launch on device buffers (the C-ABI idg_*_launch path).
// `force` launches a caller-supplied 13-argument kernel instead of the
// selected one (the func/num_threads arguments of c_run_gridder_).
hipError_t launch(Direction dir, const Problem &p, const void *d_uvw,
                  const float *d_wavenumbers, void *d_visibilities,
                  const float *d_spheroidal, const void *d_aterms,
                  const void *d_metadata, void *d_subgrids,
                  hipStream_t stream, const KernelChoice *force = nullptr,
                  const Options &opt = Options());

// Synchronous host-buffer pipeline: validate, allocate, H2D, launch, D2H,
// free.  Returns hipSuccess or the first error; *msg explains validation
// failures.
hipError_t run_host(Direction dir, const Problem &p, const Extents &e,
                    const void *uvw, const float *wavenumbers,
                    void *visibilities, const float *spheroidal,
                    const void *aterms, const idg::Metadata *metadata,
                    void *subgrids, std::string *msg,
                    const KernelChoice *force = nullptr,
                    const Options &opt = Options());

// Chunk plan of run_host: subgrid bounds (nchunk + 1 entries) of
// consecutive chunks whose visibility rows are disjoint and ascending, and
// each chunk's merged row runs; one chunk when they are not.  `moved` =
// bytes of visibilities + subgrids.  Returns the chunk count.
int plan_host_chunks(const idg::Metadata *metadata, int nr_subgrids,
                     size_t moved, std::vector<int> *bounds,
                     std::vector<std::vector<std::pair<long long, long long>>>
                         *row_runs);

// Workgroups of `func` (block threads) resident on the current device at
// once: occupancy x CUs, cached per (device, kernel); 0 if the query fails.
int resident_workgroups(const void *func, int block);

// Pipeline steps (kernels/pipeline_mi355x.hip.cpp; include/idg_mi355x.h).
hipError_t launch_subgrid_fft(int nr_subgrids, int subgrid_size, int sign,
                              float scale, void *d_subgrids,
                              hipStream_t stream);
hipError_t launch_adder(int nr_subgrids, int grid_size, int subgrid_size,
                        int nr_w_layers, const void *d_metadata,
                        const void *d_subgrids, void *d_grid,
                        hipStream_t stream);
hipError_t launch_splitter(int nr_subgrids, int grid_size, int subgrid_size,
                           int nr_w_layers, const void *d_metadata,
                           const void *d_grid, void *d_subgrids,
                           hipStream_t stream);
// launch_splitter then launch_subgrid_fft(-1, 1/S^2), fused for S = 32/64
hipError_t launch_splitter_fft(int nr_subgrids, int grid_size,
                               int subgrid_size, int nr_w_layers,
                               const void *d_metadata, const void *d_grid,
                               void *d_subgrids, hipStream_t stream);

// Grid <-> image (kernels/image_mi355x.hip.cpp).  grid_size:
// a power of two in [64, 4096] (grid_fft_supported), else
// hipErrorInvalidValue.  launch_grid_fft: in-place 2-D DFT of nr_planes
// planes, the definition of launch_subgrid_fft.  launch_grid_to_image
// destroys the grid (the transform runs in place); launch_image_to_grid
// overwrites every layer.  d_correction: [G][G] floats or null (1).  None of
// them needs scratch beyond the grid.
bool grid_fft_supported(int grid_size);
hipError_t launch_grid_fft(int grid_size, int nr_planes, int sign, float scale,
                           void *d_planes, hipStream_t stream);
hipError_t launch_grid_to_image(int grid_size, int nr_w_layers,
                                float image_size, float w_step_in_lambda,
                                const float *d_correction, void *d_grid,
                                void *d_image, hipStream_t stream);
hipError_t launch_image_to_grid(int grid_size, int nr_w_layers,
                                float image_size, float w_step_in_lambda,
                                const float *d_correction, const void *d_image,
                                void *d_grid, hipStream_t stream);

// Perf entry shared by p_run_gridder_/p_run_degridder_: env-configured
// problem, synthetic inputs, timed launches.  Returns seconds per launch.
double run_performance(Direction dir, const void *func, std::string name,
                       int num_threads);

}  // namespace idg_mi355x
