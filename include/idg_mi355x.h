/*
 * idg_mi355x.h -- C ABI of the MI355X IDG gridder/degridder
 *                 (libidg_mi355x.so, built from ska-sdp-idg-bench_amd/csrc).
 *
 * Plain C: pointers, sizes, int status codes; no C++ or torch types.  Each
 * entry point names the reference interface of ska-telescope/ska-sdp-idg-bench
 * it replaces.  The reference's own binding for this path is C++
 * (hip::c_run_gridder et al. with idg::ArrayND& arguments, mangled names);
 * libidg_mi355x.so exports those C++ symbols too (ska-sdp-idg-bench_amd/csrc/
 * lib-hip.hpp), and this header is the flat C twin an FFI (ctypes, cgo, JNI,
 * N-API) binds.  See INTEGRATION.md.
 *
 * Layouts (row-major, complex = interleaved {re, im} float32):
 *   uvw           [rows]                 idg_uvw_t     (rows = visibility rows)
 *   wavenumbers   [nr_channels]          float
 *   visibilities  [rows][nr_channels][4] idg_cfloat_t  (xx, xy, yx, yy)
 *   spheroidal    [S][S]                 float
 *   aterms        [slots][nr_stations][S][S][4] idg_cfloat_t
 *   metadata      [nr_subgrids]          idg_metadata_t
 *   subgrids      [nr_subgrids][4][S][S] idg_cfloat_t  (correlation-planar)
 * Row index of timestep t of subgrid s:
 *   (md[s].baseline_offset - md[0].baseline_offset) + md[s].time_offset + t
 *
 * Status: 0 = success, > 0 = hipError_t of the failing HIP call, < 0 = the
 * IDG_E_* codes below; idg_last_error() describes the last failure of the
 * calling thread.  (The reference's C++ entries abort the process on error,
 * app/HIP/util.cpp:5-15; the C++ symbols of this library keep that.)
 */
#ifndef IDG_MI355X_H_
#define IDG_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDG_MI355X_ABI_VERSION 1

#define IDG_OK 0
#define IDG_E_INVALID_ARGUMENT (-1) /* bad sizes / null pointers          */
#define IDG_E_OUT_OF_BOUNDS (-2)    /* metadata indexes outside a buffer  */
#define IDG_E_NO_DEVICE (-3)        /* no HIP device visible              */

/* idg::Metadata (reference app/common/types.hpp:11-26), 36 bytes. */
typedef struct idg_metadata_t {
  int32_t baseline_offset;
  int32_t time_offset;
  int32_t nr_timesteps;
  int32_t aterm_index;
  uint32_t station1;
  uint32_t station2;
  int32_t coord_x;
  int32_t coord_y;
  int32_t coord_z;
} idg_metadata_t;

/* idg::UVWCoordinate<float> (types.hpp:49-54). */
typedef struct idg_uvw_t {
  float u, v, w;
} idg_uvw_t;

/* std::complex<float> */
typedef struct idg_cfloat_t {
  float re, im;
} idg_cfloat_t;

int idg_abi_version(void);

/* ---- host-buffer entries (synchronous, allocate + copy + launch + copy) ---
 * Replace hip::c_run_gridder / hip::c_run_degridder, the kernel-TU contract
 * of the reference (app/HIP/kernels/gridder_v1.hip.cpp:118-137 and
 * degridder_v1.hip.cpp; declared by the harness at
 * tests/gridder_common.cpp:21-30, tests/degridder_common.cpp:21-30), which
 * run app/HIP/util.cpp:255-311 / :392-448.  The ArrayND arguments become
 * (pointer, element count): uvw_rows UVW triplets (visibilities then hold
 * uvw_rows * nr_channels * 4 complex values) and aterm_slots timeslots.
 * Metadata is validated against these extents before anything is launched.
 * The gridder fully overwrites subgrids; the degridder writes every
 * visibility row referenced by the metadata. */
int idg_c_run_gridder(int nr_subgrids, int grid_size, int subgrid_size,
                      float image_size, float w_step_in_lambda,
                      int nr_channels, int nr_stations, const idg_uvw_t *uvw,
                      size_t uvw_rows, const float *wavenumbers,
                      const idg_cfloat_t *visibilities,
                      const float *spheroidal, const idg_cfloat_t *aterms,
                      size_t aterm_slots, const idg_metadata_t *metadata,
                      idg_cfloat_t *subgrids);

int idg_c_run_degridder(int nr_subgrids, int grid_size, int subgrid_size,
                        float image_size, float w_step_in_lambda,
                        int nr_channels, int nr_stations,
                        const idg_uvw_t *uvw, size_t uvw_rows,
                        const float *wavenumbers, idg_cfloat_t *visibilities,
                        const float *spheroidal, const idg_cfloat_t *aterms,
                        size_t aterm_slots, const idg_metadata_t *metadata,
                        const idg_cfloat_t *subgrids);

/* ---- device-buffer entries (asynchronous on `stream`) ---------------------
 * The launch half of the same pipeline: hipLaunchKernel with the 13-argument
 * kernel ABI, grid = nr_subgrids, block = 256 (reference
 * app/HIP/util.cpp:167-174 c_run_kernel and :237-244).  All pointers are
 * device pointers, resident in HBM; `stream` is a hipStream_t (NULL = the
 * legacy default stream).  The caller guarantees metadata validity (use
 * idg_validate_metadata on a host copy). */
int idg_gridder_launch(int nr_subgrids, int grid_size, int subgrid_size,
                       float image_size, float w_step_in_lambda,
                       int nr_channels, int nr_stations, const idg_uvw_t *uvw,
                       const float *wavenumbers,
                       const idg_cfloat_t *visibilities,
                       const float *spheroidal, const idg_cfloat_t *aterms,
                       const idg_metadata_t *metadata, idg_cfloat_t *subgrids,
                       void *stream);

int idg_degridder_launch(int nr_subgrids, int grid_size, int subgrid_size,
                         float image_size, float w_step_in_lambda,
                         int nr_channels, int nr_stations,
                         const idg_uvw_t *uvw, const float *wavenumbers,
                         idg_cfloat_t *visibilities, const float *spheroidal,
                         const idg_cfloat_t *aterms,
                         const idg_metadata_t *metadata,
                         const idg_cfloat_t *subgrids, void *stream);

/* Host-side bounds check of metadata against the buffer extents (what the
 * host-buffer entries run before launching).  Returns IDG_OK or
 * IDG_E_OUT_OF_BOUNDS / IDG_E_INVALID_ARGUMENT. */
int idg_validate_metadata(int nr_subgrids, int subgrid_size, int nr_channels,
                          int nr_stations, size_t uvw_rows, size_t aterm_slots,
                          const idg_metadata_t *metadata);

/* The chunk plan the host-buffer entries use for a batch whose copies move
 * bytes_moved bytes (visibilities + subgrids): consecutive subgrid ranges
 * [bounds[i], bounds[i+1]) whose visibility rows are disjoint and ascending,
 * so chunk i's copies overlap chunk i-1's kernel; one chunk when the rows are
 * not.  Writes at most max_bounds entries of bounds (nchunk + 1 in all) and
 * returns nchunk (< 0 on bad arguments).  No reference counterpart: the
 * reference's c_run_* copies everything, launches once, copies back
 * (app/HIP/util.cpp:255-311). */
int idg_host_chunk_plan(int nr_subgrids, const idg_metadata_t *metadata,
                        size_t bytes_moved, int *bounds, int max_bounds);

/* Name of the kernel the launch entries select for this geometry
 * (direction 0 = gridder, 1 = degridder); for profiles and reports. */
const char *idg_kernel_name(int direction, int subgrid_size, int nr_channels);

/* Precision options of the kernels the launch entries select for this
 * geometry (bit 0: the phase-reduction tail on every phasor, bit 1: blocked
 * summation, bit 2: the tail on one channel per quad); the
 * IDG_PREC environment variable overrides them.  No reference counterpart:
 * the reference's kernels have a single precision path. */
int idg_precision_options(int direction, int subgrid_size, int nr_channels);

/* ---- perf entries ---------------------------------------------------------
 * Replace hip::p_run_gridder / hip::p_run_degridder (kernel TUs, e.g.
 * gridder_v1.hip.cpp:114-116 -> app/HIP/util.cpp:176-253 / :313-390): the
 * problem comes from the environment (NR_STATIONS=50, NR_TIMESLOTS=20,
 * NR_TIMESTEPS_SUBGRID=128, NR_CHANNELS=16, SUBGRID_SIZE=32, GRID_SIZE=1024,
 * NR_WARM_UP_RUNS=2, NR_ITERATIONS=5), prints the reference report line and
 * CSV; returns milliseconds per launch (< 0 on error). */
double idg_p_run_gridder(void);
double idg_p_run_degridder(void);

/* ---- device info (app/lib-hip.hpp:5-9) ----------------------------------- */
void idg_print_device_info(void);
void idg_print_benchmark(void);
/* extern_get_device_name (declared, never defined, in the reference).
 * Writes at most len bytes incl. NUL; returns the full name length. */
int idg_get_device_name(char *buf, size_t len);

/* ---- work model (app/common/common.cpp:100-159) -------------------------- */
uint64_t idg_flops_gridder(uint64_t nr_channels, uint64_t nr_timesteps,
                           uint64_t nr_subgrids, uint64_t subgrid_size,
                           uint64_t nr_correlations);
uint64_t idg_bytes_gridder(uint64_t nr_channels, uint64_t nr_timesteps,
                           uint64_t nr_subgrids, uint64_t subgrid_size,
                           uint64_t nr_correlations);

/* ---- pipeline steps either side of the path ----
 * Not in the reference (its Grid type is unused, app/common/types.hpp:358-370):
 * these complete gridding into, and degridding from, a uv grid.  Conventions
 * (DESIGN.md §8f):
 *   gridding:   idg_gridder_launch -> idg_subgrid_fft_launch(+1, 1.0f)
 *               -> idg_adder_launch
 *   degridding: idg_splitter_launch -> idg_subgrid_fft_launch(-1, 1/S^2)
 *               -> idg_degridder_launch
 * grid: [nr_w_layers][4][grid_size][grid_size] complex64; a subgrid goes to
 * layer metadata.coordinate.z.  Device pointers, asynchronous on `stream`.
 */

/* In-place 2-D DFT of each [S][S] correlation plane of subgrids
 * [nr_subgrids][4][S][S]: out[k][l] = scale * sum in[y][x] *
 * exp(sign * 2 pi i (k y + l x) / S); sign = +1 or -1. */
int idg_subgrid_fft_launch(int nr_subgrids, int subgrid_size, int sign,
                           float scale, idg_cfloat_t *subgrids, void *stream);

/* grid[z][pol][y0 + y][x0 + x] += exp(i pi ((x + y)(S + 1)/S - 1)) *
 * subgrid[s][pol][(y + S/2) % S][(x + S/2) % S]; subgrids not wholly inside
 * the grid are skipped.  Deterministic: a per-tile gather in subgrid order,
 * no atomics. */
int idg_adder_launch(int nr_subgrids, int grid_size, int subgrid_size,
                     int nr_w_layers, const idg_metadata_t *metadata,
                     const idg_cfloat_t *subgrids, idg_cfloat_t *grid,
                     void *stream);

/* The adjoint placement: subgrid[s][pol][(y + S/2) % S][(x + S/2) % S] =
 * exp(-i pi ((x + y)(S + 1)/S - 1)) * grid[z][pol][y0 + y][x0 + x]; zero for
 * subgrids not wholly inside the grid. */
int idg_splitter_launch(int nr_subgrids, int grid_size, int subgrid_size,
                        int nr_w_layers, const idg_metadata_t *metadata,
                        const idg_cfloat_t *grid, idg_cfloat_t *subgrids,
                        void *stream);

/* idg_gridder_launch followed by idg_subgrid_fft_launch(+1, 1.0f): the
 * adder's input subgrids straight from the visibilities.  For S = 32 the FFT
 * runs in the gridder's epilogue (the image-domain subgrids never reach
 * HBM), bit for bit the two launches' result; other S <= 64 run the two
 * launches.  Arguments as idg_gridder_launch. */
int idg_gridder_fft_launch(int nr_subgrids, int grid_size, int subgrid_size,
                           float image_size, float w_step_in_lambda,
                           int nr_channels, int nr_stations,
                           const idg_uvw_t *uvw, const float *wavenumbers,
                           const idg_cfloat_t *visibilities,
                           const float *spheroidal, const idg_cfloat_t *aterms,
                           const idg_metadata_t *metadata,
                           idg_cfloat_t *subgrids, void *stream);

/* idg_splitter_launch followed by idg_subgrid_fft_launch(-1, 1/S^2): the
 * degridder's input subgrids straight from the grid.  For S = 32 and 64 one
 * fused kernel (the uv-domain subgrids never reach HBM), bit for bit the
 * two launches' result; other even S <= 64 run the two launches. */
int idg_splitter_fft_launch(int nr_subgrids, int grid_size, int subgrid_size,
                            int nr_w_layers, const idg_metadata_t *metadata,
                            const idg_cfloat_t *grid, idg_cfloat_t *subgrids,
                            void *stream);

/* ---- grid <-> image ----------------------------------------
 * The steps between the uv grid and the image, in this library's sign
 * convention (the degridder's phase +i (k (u l + v m + w n) - offset), the
 * gridder its adjoint).  Image: [4][grid_size][grid_size] complex64,
 * correlation-planar like the grid; pixel (y, x) stands for
 *   l = (x - grid_size/2) * image_size / grid_size,
 *   m = (y - grid_size/2) * image_size / grid_size,  n = 1 - sqrt(1 - l^2 - m^2).
 * grid_size: a power of two in [64, 4096]; 1 <= nr_w_layers <= 16383 (the
 * 4 nr_w_layers planes are one launch's grid); else IDG_E_INVALID_ARGUMENT.
 * Device pointers, asynchronous on `stream`; no scratch is needed beyond the
 * grid itself, so a launch allocates nothing.  None of the four entries has
 * a reference counterpart (the reference stops at subgrids).
 */

/* In-place 2-D DFT of nr_planes planes of [grid_size][grid_size] complex64,
 * the definition of idg_subgrid_fft_launch: out[k][l] = scale * sum in[y][x] *
 * exp(sign * 2 pi i (k y + l x) / grid_size); sign = +1 or -1; no shift.
 * No reference counterpart. */
int idg_grid_fft_launch(int grid_size, int nr_planes, int sign, float scale,
                        idg_cfloat_t *planes, void *stream);

/* image[pol][y][x] = correction[y][x] * sum_z exp(-2 pi i w_step_in_lambda
 * (z + 0.5) n) * sum_{Y,X} grid[z][pol][Y][X] * exp(-2 pi i ((X - G/2)(x - G/2)
 * + (Y - G/2)(y - G/2)) / G): the centred grid FFT, the w-stacking phasor,
 * the sum over the layers and the correction (real [G][G]; NULL = 1).  With
 * the grid that idg_adder_launch fills from
 * idg_gridder_fft_launch this is S^2 taper(l, m) times the direct sum
 * sum_{row,c} A1^H V A2 exp(-i k_c (u l + v m + w n)) (S = the subgrid size,
 * taper = idg_taper_to_image): pass correction = 1 / (S^2 taper) for the
 * image itself.  DESTROYS the grid (the transform's passes run in place).
 * No reference counterpart. */
int idg_grid_to_image_launch(int grid_size, int nr_w_layers, float image_size,
                             float w_step_in_lambda, const float *correction,
                             idg_cfloat_t *grid, idg_cfloat_t *image,
                             void *stream);

/* The exact adjoint of idg_grid_to_image_launch: grid[z][pol][Y][X] =
 * sum_{y,x} exp(+2 pi i ((X - G/2)(x - G/2) + (Y - G/2)(y - G/2)) / G) *
 * exp(+2 pi i w_step_in_lambda (z + 0.5) n) * correction[y][x] *
 * image[pol][y][x]; every one of the nr_w_layers layers is overwritten.
 * With correction = 1 / taper, idg_splitter_fft_launch and
 * idg_degridder_launch then predict V = sum_{y,x} A1 image A2^H
 * exp(+i k_c (u l + v m + w n)).  No reference counterpart. */
int idg_image_to_grid_launch(int grid_size, int nr_w_layers, float image_size,
                             float w_step_in_lambda, const float *correction,
                             const idg_cfloat_t *image, idg_cfloat_t *grid,
                             void *stream);

/* The taper as the image sees it (host pointers, no device needed):
 * out[grid_size][grid_size] (double) = the separable trigonometric interpolant of
 * spheroidal[S][S], whose samples sit at the subgrid's half-pixel-centred
 * positions (p + 0.5 - S/2) / S of the field of view, evaluated at the image
 * pixels' (x - grid_size/2) / grid_size; the Nyquist term is split
 * symmetrically, so the result is real.  S/2 and grid_size/2 are integer
 * divisions, as in the gridder's own pixel coordinates (reference
 * app/common/math.hpp:9-13): for an odd S the samples sit at p + 0.5 -
 * floor(S/2), half a pixel off the field centre, where the gridder puts
 * them, and there is no Nyquist term.  Summed directly in double,
 * O(G S (S + G)).  The caller inverts it (and decides where it is too close
 * to 0 to invert).  subgrid_size, grid_size >= 1, else
 * IDG_E_INVALID_ARGUMENT.  No reference counterpart. */
int idg_taper_to_image(int subgrid_size, int grid_size,
                       const float *spheroidal, double *out);

/* ---- synthetic observation (app/common/init.cpp:4-180) -------------------
 * Exactly the reference harness' inputs: srand(0), then the initialize_*
 * generators in harness order.  nr_subgrids = nr_stations*(nr_stations-1)/2
 * * nr_timeslots is returned.  Any output pointer may be NULL to skip it
 * (the random stream is consumed identically either way).  Sizes:
 *   uvw [nr_subgrids*nr_timesteps], frequencies/wavenumbers [nr_channels],
 *   visibilities [nr_subgrids*nr_timesteps*nr_channels*4],
 *   spheroidal [S*S], aterms [nr_timeslots*nr_stations*S*S*4],
 *   metadata [nr_subgrids], subgrids [nr_subgrids*4*S*S].
 * nthreads > 1 parallelises the (random-free) visibility generator. */
int idg_generate(int nr_stations, int nr_timeslots, int nr_timesteps,
                 int nr_channels, int grid_size, int subgrid_size,
                 idg_uvw_t *uvw, float *frequencies, float *wavenumbers,
                 idg_cfloat_t *visibilities, float *spheroidal,
                 idg_cfloat_t *aterms, idg_metadata_t *metadata,
                 idg_cfloat_t *subgrids, int nthreads);

/* ---- workspaces -----------------------------------------------------------
 * The device entries keep their scratch (the two-kernel form's subgrid queue,
 * the adder's home sort and segment lists, the plan's counts, the weight
 * steps' partial sums) cached per (device, stream), so a
 * launch makes no allocation.  idg_release_workspaces frees the cache of
 * `stream` on the current device (all != 0: of every stream of the current
 * device).  The stream(s) must be idle (their work complete): call it before
 * destroying a stream the entries used -- a new stream may be given the same
 * handle -- and before hipDeviceReset.  Returns IDG_OK or a HIP error code
 * (hipErrorNotReady: a slot was being enqueued on by another host thread and
 * was left).  No reference counterpart (the reference allocates per call,
 * app/HIP/util.cpp:220-232). */
int idg_release_workspaces(void *stream, int all);

const char *idg_last_error(void);

/* ---- per-call launch options ----------------------------------------------
 * Which kernels a call runs, chosen by the caller for that call instead of by
 * the process environment.  Every field uses 0 for "unset": the environment
 * variable of the same meaning if it is set (IDG_GRIDDER_IMPL,
 * IDG_DEGRIDDER_IMPL, IDG_PREC, IDG_KERNEL_FORM, IDG_GRID_FFT), else the
 * library's default -- what the entries without options do.  An explicit
 * field wins over its variable.  A NULL pointer and a zero-filled struct with
 * struct_size set are the same thing.
 *
 * struct_size = sizeof(idg_options_t) of the caller's header.  Fields beyond
 * a smaller struct_size count as unset; a larger one is accepted while every
 * byte past the fields known here is zero.  IDG_E_INVALID_ARGUMENT: a
 * struct_size below the first field's end or not a multiple of 4, a non-zero
 * byte past the known fields, an unknown enum value, a degridder_impl other
 * than ENV / DEFAULT / SEQUENTIAL.  No reference counterpart: the reference
 * has one kernel per direction. */
#define IDG_IMPL_ENV 0        /* unset                                       */
#define IDG_IMPL_DEFAULT 1    /* the MFMA kernels, whatever the environment  */
#define IDG_IMPL_VALU 2       /* gridder: the VALU mirror path               */
#define IDG_IMPL_SEQUENTIAL 3 /* the reference CPU path's rounding sequence  */
#define IDG_IMPL_ORDERED 4    /* gridder: reference summation order          */
#define IDG_IMPL_AUTO 5       /* gridder: ORDERED for the subgrids with
                                 nr_timesteps * nr_channels > auto_threshold,
                                 DEFAULT for the others, chosen on the device
                                 per subgrid                 */

#define IDG_PREC_SET 8u /* precision = IDG_PREC_SET | bits (bits 0..7 as
                           idg_precision_options), so bits = 0 can be forced */

#define IDG_FORM_ENV 0
#define IDG_FORM_COMBINED 1 /* one kernel for every subgrid                  */
#define IDG_FORM_SPLIT 2    /* mirror kernel + queue-fed general kernel      */

#define IDG_FFT_FUSION_ENV 0
#define IDG_FFT_FUSION_OFF 1 /* idg_gridder_fft_launch: two launches         */
#define IDG_FFT_FUSION_ON 2  /* the FFT in the gridder's epilogue (S = 32)   */

#define IDG_AUTO_THRESHOLD_DEFAULT 16384u

typedef struct idg_options_t {
  uint32_t struct_size;    /* sizeof(idg_options_t)                          */
  uint32_t gridder_impl;   /* IDG_IMPL_*                                     */
  uint32_t degridder_impl; /* IDG_IMPL_ENV / _DEFAULT / _SEQUENTIAL          */
  uint32_t precision;      /* 0, or IDG_PREC_SET | bits                      */
  uint32_t kernel_form;    /* IDG_FORM_*                                     */
  uint32_t fft_fusion;     /* IDG_FFT_FUSION_*                               */
  uint32_t auto_threshold; /* IDG_IMPL_AUTO; 0 = IDG_AUTO_THRESHOLD_DEFAULT  */
} idg_options_t;

/* The entries above with options; the entries above are these with NULL.
 * Under IDG_IMPL_AUTO the launch stays asynchronous (the classification runs
 * on the device), each selected subgrid is bit for bit the IDG_IMPL_ORDERED
 * launch's and each other one the IDG_IMPL_DEFAULT launch's of the same
 * kernel form; precision and kernel_form apply to the default pass and the
 * FFT of idg_gridder_fft_launch_opts is a launch of its own. */
int idg_c_run_gridder_opts(int nr_subgrids, int grid_size, int subgrid_size,
                           float image_size, float w_step_in_lambda,
                           int nr_channels, int nr_stations,
                           const idg_uvw_t *uvw, size_t uvw_rows,
                           const float *wavenumbers,
                           const idg_cfloat_t *visibilities,
                           const float *spheroidal, const idg_cfloat_t *aterms,
                           size_t aterm_slots, const idg_metadata_t *metadata,
                           idg_cfloat_t *subgrids,
                           const idg_options_t *options);

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
                             const idg_options_t *options);

int idg_gridder_launch_opts(int nr_subgrids, int grid_size, int subgrid_size,
                            float image_size, float w_step_in_lambda,
                            int nr_channels, int nr_stations,
                            const idg_uvw_t *uvw, const float *wavenumbers,
                            const idg_cfloat_t *visibilities,
                            const float *spheroidal,
                            const idg_cfloat_t *aterms,
                            const idg_metadata_t *metadata,
                            idg_cfloat_t *subgrids, void *stream,
                            const idg_options_t *options);

int idg_degridder_launch_opts(int nr_subgrids, int grid_size, int subgrid_size,
                              float image_size, float w_step_in_lambda,
                              int nr_channels, int nr_stations,
                              const idg_uvw_t *uvw, const float *wavenumbers,
                              idg_cfloat_t *visibilities,
                              const float *spheroidal,
                              const idg_cfloat_t *aterms,
                              const idg_metadata_t *metadata,
                              const idg_cfloat_t *subgrids, void *stream,
                              const idg_options_t *options);

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
                                const idg_options_t *options);

/* NULL (and idg_last_error) on invalid options.  Under IDG_IMPL_AUTO the
 * gridder's name is gridder_auto_mi355x_{s32,s64,generic}. */
const char *idg_kernel_name_opts(int direction, int subgrid_size,
                                 int nr_channels,
                                 const idg_options_t *options);

/* < 0 on invalid options.  Under IDG_IMPL_AUTO: the default pass's bits. */
int idg_precision_options_opts(int direction, int subgrid_size,
                               int nr_channels, const idg_options_t *options);

/* The host twin of IDG_IMPL_AUTO's device classification: selected[s] = 1 for
 * every subgrid an auto launch with these options sends to the ordered
 * kernel (nr_timesteps * nr_channels > the threshold, the product in 64
 * bits; nr_timesteps <= 0 never), else 0; returns their count, < 0 on bad
 * arguments.  metadata and selected are host pointers (selected may be NULL
 * to count only). */
int idg_auto_selected(int nr_subgrids, int nr_channels,
                      const idg_options_t *options,
                      const idg_metadata_t *metadata, uint8_t *selected);

/* ---- plan: uvw tracks -> subgrid metadata --------------------
 * The step between "I have uvw" and the entries above.  No reference
 * counterpart: the reference's initialize_metadata (app/common/init.cpp)
 * draws subgrid coordinates at random.  Each baseline's nr_timesteps rows
 * (row bl * nr_timesteps + t of uvw, metres) are walked in time order and cut
 * greedily into subgrids: a timestep joins the open subgrid while that has
 * fewer than max_nr_timesteps_per_subgrid timesteps, the A-term slot
 * (t / nr_timesteps_per_aterm) and the w layer stay the same, and a subgrid
 * centred on the uv cells of all its timesteps at the first and the last
 * channel still has kernel_size cells to spare and lies wholly inside the
 * grid.  Timesteps with a non-finite coordinate, or whose own cells fit no
 * subgrid, are dropped (in no subgrid) and counted.  Records are written
 * baseline-major, in time order, with baseline_offset = 0 and time_offset =
 * the first row; the w layer (coord_z) is floor(w * mean wavenumber / (2 pi
 * w_step_in_lambda)) clamped into [0, nr_w_layers - 1], 0 when
 * w_step_in_lambda is 0.  All arithmetic is float32 and the two entries
 * produce the same bytes.
 *
 * struct_size = sizeof(idg_plan_params_t), with the rules of idg_options_t:
 * fields beyond a smaller struct_size are zero, bytes past the fields known
 * here must be zero.  IDG_E_INVALID_ARGUMENT: that, sizes < 1,
 * kernel_size < 0 or >= subgrid_size, subgrid_size > grid_size,
 * max_nr_timesteps_per_subgrid < 1, nr_timesteps_per_aterm < 0,
 * nr_w_layers < 1 or > 2^24, capacity < 0, nr_baselines * nr_timesteps >=
 * 2^31. */
typedef struct idg_plan_params_t {
  uint32_t struct_size; /* sizeof(idg_plan_params_t)                        */
  int32_t grid_size;
  int32_t subgrid_size;
  float image_size;
  float w_step_in_lambda;
  int32_t nr_w_layers;
  int32_t kernel_size; /* uv cells kept free at the subgrid's edge          */
  int32_t max_nr_timesteps_per_subgrid;
  int32_t nr_timesteps_per_aterm; /* 0 = one A-term slot                    */
} idg_plan_params_t;

/* Host pointers, no device needed.  baselines: [nr_baselines][2] station
 * indices; wavenumbers: monotone, only the first and the last are read.
 * Writes the first min(needed, capacity) records (metadata may be NULL with
 * capacity 0), counts[0] = subgrids needed, counts[1] = dropped timesteps.
 * nthreads > 1 splits the baselines over threads (same bytes). */
int idg_plan(const idg_plan_params_t *params, int nr_baselines,
             int nr_timesteps, const uint32_t *baselines, const idg_uvw_t *uvw,
             int nr_channels, const float *wavenumbers,
             idg_metadata_t *metadata, int capacity, int32_t counts[2],
             int nthreads);

/* The same on device pointers (baselines, uvw, wavenumbers, metadata and
 * counts all in device memory), asynchronous on `stream`; nothing is read
 * back: the caller reads counts[0] to size the gridder launch.  Its scratch
 * comes from the workspace cache (idg_release_workspaces). */
int idg_plan_launch(const idg_plan_params_t *params, int nr_baselines,
                    int nr_timesteps, const uint32_t *baselines,
                    const idg_uvw_t *uvw, int nr_channels,
                    const float *wavenumbers, idg_metadata_t *metadata,
                    int capacity, int32_t counts[2], void *stream);

/* ---- imaging weights -------------------------------------------
 * The step between "uvw, visibilities and weights" and a normalised dirty
 * image and its PSF: the uv sampling density of the samples the gridder will
 * grid, the (a, b) of a weighting scheme, and the imaging weights
 * f = w / (a + b D).  No reference counterpart (the reference stops at
 * subgrids); each entry has a host form (host pointers, no device needed)
 * and a _launch form (device pointers, asynchronous on `stream`, nothing read
 * back) that produce the same bytes, except the two double sums noted below.
 *
 * weights: float32 [rows][nr_channels], one weight per row and channel,
 * shared by the four correlations; a flag is a weight of 0.  Only the samples
 * a subgrid covers count (rows time_offset .. time_offset + nr_timesteps - 1
 * of each record, indexed as for the gridder); other rows are neither read
 * nor written.
 *
 * Cell of a sample: X = floorf(u * s_c + 0.5f) + grid_size / 2 (Y from v),
 * s_c = wavenumbers[c] * (image_size / 2 pi): the nearest cell of the grid
 * idg_grid_to_image_launch transforms; w and the w layer play no part.
 * Quantised weight: q = (uint64) rintf(w * 2^-quantum_log2) for a finite
 * w > 0 whose scaled value is below 2^40, else 0.  A sample with q = 0, or
 * whose cell is not finite or outside the grid, is flagged: nothing in the
 * density, imaging weight 0, weighted visibility literal zeros.
 * density: uint64 [grid_size][grid_size]; density[Y][X] = the sum of q over
 * the covered samples in that cell -- exact, whatever the order.  THE CALLER
 * KEEPS EVERY CELL'S SUM BELOW 2^62 (with q < 2^40 that is 2^22 samples of
 * the largest weight in one cell); the host entries check it.
 * D at a cell = (float) n * 2^quantum_log2 with n = density[Y][X], plus
 * density[G - Y][G - X] when `hermitian` is set and that cell is inside the
 * grid (X, Y >= 1): the centre cell counts twice, row 0 and column 0 have no
 * mirror.
 *
 * struct_size = sizeof(idg_weight_params_t), with the rules of idg_options_t.
 * The fields are taken as they are (0 is quantum 1, hermitian off, natural):
 * set quantum_log2 = IDG_WEIGHT_QUANTUM_LOG2_DEFAULT and hermitian = 1 for
 * the usual case.  IDG_E_INVALID_ARGUMENT: a bad struct_size, grid_size < 1
 * or > 16384, quantum_log2 outside [-64, 64], an unknown scheme, a non-finite
 * image_size or robust, nr_subgrids < 0, nr_channels < 1, subgrid_size < 1,
 * a null buffer, a density cell at or above 2^62 (host forms).
 * IDG_E_OUT_OF_BOUNDS: a record's rows outside [0, uvw_rows) (host forms; the
 * _launch forms trust the metadata, use idg_validate_metadata). */
#define IDG_WEIGHT_NATURAL 0 /* a = 1, b = 0: f = w                           */
#define IDG_WEIGHT_UNIFORM 1 /* a = 0, b = 1: f = w / D                       */
#define IDG_WEIGHT_BRIGGS 2  /* a = 1, b = (float)((5 * 10^-robust)^2 *
                                sum D / sum D^2), the sums over all cells in
                                double; b = 0 for an empty density            */
#define IDG_WEIGHT_QUANTUM_LOG2_DEFAULT (-20)

typedef struct idg_weight_params_t {
  uint32_t struct_size; /* sizeof(idg_weight_params_t)                       */
  int32_t grid_size;
  float image_size;
  int32_t quantum_log2; /* weights are counted in units of 2^quantum_log2    */
  int32_t hermitian;    /* != 0: D counts the mirror cell too                */
  int32_t scheme;       /* IDG_WEIGHT_* (idg_weight_scheme*)                 */
  float robust;         /* IDG_WEIGHT_BRIGGS                                 */
} idg_weight_params_t;

/* density[Y][X] += the sum of q over the covered samples of that cell: the
 * entry accumulates, the caller zeroes the buffer, several batches may add to
 * one density.  nr_subgrids = 0: a no-op.  The host form leaves the density
 * untouched when it fails.  Device: one workgroup per subgrid sums in an
 * S x S LDS tile at the subgrid's corner and adds its non-zero cells, and
 * every sample outside the tile, with 64-bit integer atomics; correct for any
 * metadata, fastest for a plan's. */
int idg_weight_density(const idg_weight_params_t *params, int nr_subgrids,
                       int subgrid_size, int nr_channels,
                       const idg_metadata_t *metadata, const idg_uvw_t *uvw,
                       size_t uvw_rows, const float *wavenumbers,
                       const float *weights, uint64_t *density);
int idg_weight_density_launch(const idg_weight_params_t *params,
                              int nr_subgrids, int subgrid_size,
                              int nr_channels, const idg_metadata_t *metadata,
                              const idg_uvw_t *uvw, const float *wavenumbers,
                              const float *weights, uint64_t *density,
                              void *stream);

/* ab[0] = a, ab[1] = b of params->scheme at this density.  The Briggs sums
 * run in double: the host form in row-major order, the device form in a
 * fixed tree (bitwise reproducible run to run; b may differ from the host's
 * in the last place). */
int idg_weight_scheme(const idg_weight_params_t *params,
                      const uint64_t *density, float ab[2]);
int idg_weight_scheme_launch(const idg_weight_params_t *params,
                             const uint64_t *density, float ab[2],
                             void *stream);

/* For every covered sample: imaging_weights[row][c] = f = w / (a + b D) (one
 * multiply, one add, one correctly rounded divide; 0 for a flagged sample),
 * out[row][c][pol] = f * visibilities[row][c][pol] (one multiply per
 * component; literal zeros for a flagged sample; out may be visibilities;
 * visibilities NULL: (f, 0, 0, f), the PSF's input), and *sum_weights = the
 * sum of f over the covered samples, in double (host: sequentially; device:
 * per-subgrid partials and a final sum in fixed orders, reproducible run to
 * run; nr_subgrids = 0 writes 0).  ab: the two floats idg_weight_scheme*
 * wrote.  Rows no subgrid covers are left as they were in all three outputs.
 * The _launch form needs visibilities and out 16-byte aligned. */
int idg_weight_apply(const idg_weight_params_t *params, int nr_subgrids,
                     int nr_channels, const idg_metadata_t *metadata,
                     const idg_uvw_t *uvw, size_t uvw_rows,
                     const float *wavenumbers, const float *weights,
                     const uint64_t *density, const float ab[2],
                     const idg_cfloat_t *visibilities, float *imaging_weights,
                     idg_cfloat_t *out, double *sum_weights);
int idg_weight_apply_launch(const idg_weight_params_t *params, int nr_subgrids,
                            int nr_channels, const idg_metadata_t *metadata,
                            const idg_uvw_t *uvw, const float *wavenumbers,
                            const float *weights, const uint64_t *density,
                            const float ab[2],
                            const idg_cfloat_t *visibilities,
                            float *imaging_weights, idg_cfloat_t *out,
                            double *sum_weights, void *stream);

/* ---- Hogbom CLEAN minor cycle ----------------------------------
 * Dirty image -> model, on one real plane: find the peak, take gain * peak as
 * a component, subtract component * psf around it, again.  No reference
 * counterpart; idg_clean (host pointers, no device needed) and
 * idg_clean_launch (device pointers, asynchronous on `stream`, nothing read
 * back, no synchronisation, scratch from the workspace cache) produce the
 * same bytes in every output.
 *
 * residual: float32 [G][G], updated in place.  psf: float32 [Gp][Gp], centre
 * at (Gp / 2, Gp / 2) (integer division), 1 <= Gp <= G <= 16384; it is used as
 * it is, not divided by its centre.  mask: uint8 [G][G] or NULL; a pixel is
 * searchable iff its byte is non-zero (NULL: all are); the mask limits the
 * search only, never the subtraction.  model: float32 [G][G], accumulated
 * onto (the caller zeroes it).  components: [max_components] records.  state:
 * input and output; the caller zeroes it before the first call, and any later
 * call with the same buffers continues from it: k calls of n iterations give
 * exactly the bytes of one call of k * n.
 *
 * Peak: among the searchable pixels whose value is not NaN the largest |s|,
 * ties (+v against -v too) to the lowest linear index y * G + x; v is the
 * signed value there.  One iteration, in this order:
 *   1. reason != 0: nothing.
 *   2. no peak: reason = IDG_CLEAN_NO_PEAK, stop.
 *   3. started == 0: level = fmaxf(threshold, cycle_fraction * |v|) (one
 *      rounded multiply), started = 1.
 *   4. !(|v| > level): reason = IDG_CLEAN_BELOW_LEVEL, stop.
 *   5. n_components == max_components: reason = IDG_CLEAN_COMPONENTS_FULL, stop.
 *   6. c = gain * v (one rounded multiply); components[n_components++] =
 *      {py, px, c}; model[py][px] += c (one add).
 *   7. every (y, x) with dy = y - py + Gp / 2 and dx = x - px + Gp / 2 inside
 *      [0, Gp): residual[y][x] = fmaf(-c, psf[dy][dx], residual[y][x]).
 * After the last iteration state.peak = |s| at the peak of the residual as it
 * stands (0 if none) and state.peak_index its linear index (-1 if none);
 * reason stays 0 when the call only ran out of iterations.  nr_iterations = 0
 * refreshes those two fields and nothing else.
 *
 * IDG_E_INVALID_ARGUMENT (every buffer left as it was): a bad struct_size
 * (the rules of idg_options_t), sizes out of range, gain / threshold /
 * cycle_fraction not finite, threshold or cycle_fraction negative,
 * nr_iterations < 0 or max_components < 0, a NULL buffer other than mask,
 * and (host form, which can read it) a state with n_components outside
 * [0, max_components]; on such a state the _launch form runs no iteration. */
#define IDG_CLEAN_RUNNING 0
#define IDG_CLEAN_BELOW_LEVEL 1
#define IDG_CLEAN_NO_PEAK 2
#define IDG_CLEAN_COMPONENTS_FULL 3

typedef struct idg_clean_params_t {
  uint32_t struct_size; /* sizeof(idg_clean_params_t)                        */
  int32_t grid_size;    /* G                                                 */
  int32_t psf_size;     /* Gp                                                */
  int32_t max_components;
  int32_t nr_iterations;
  float gain;
  float threshold;
  float cycle_fraction;
} idg_clean_params_t;

typedef struct idg_clean_component_t {
  int32_t y, x;
  float value;
} idg_clean_component_t;

typedef struct idg_clean_state_t {
  int32_t n_components;
  int32_t reason;     /* IDG_CLEAN_*                                         */
  int32_t started;    /* != 0: level is set                                  */
  int32_t peak_index; /* y * G + x of the residual's peak, -1: none          */
  float level;
  float peak;
} idg_clean_state_t;

int idg_clean(const idg_clean_params_t *params, float *residual,
              const float *psf, const uint8_t *mask, float *model,
              idg_clean_component_t *components, idg_clean_state_t *state);
/* One launch per iteration plus two: a caller who wants to stop early reads
 * state->reason between calls of a few iterations each. */
int idg_clean_launch(const idg_clean_params_t *params, float *residual,
                     const float *psf, const uint8_t *mask, float *model,
                     idg_clean_component_t *components,
                     idg_clean_state_t *state, void *stream);

/* ---- Clark CLEAN: many components per launch on a candidate list
 * The minor cycle of idg_clean on the few thousand brightest pixels alone
 * (Clark 1980): a round selects them, runs the cycle on that list, and then
 * subtracts the components it found from the whole residual.  On the device
 * the list lives in the registers of one workgroup, so a round of thousands
 * of components is a fixed handful of launches.  No reference counterpart;
 * idg_clark (host pointers, no device needed) and idg_clark_launch (device
 * pointers, asynchronous on `stream`, nothing read back, scratch from the
 * workspace cache) produce the same bytes in every output.
 *
 * residual, psf, mask, model and components are idg_clean's, with the same
 * meaning: the mask limits which pixels may become candidates, never what is
 * subtracted.  state: idg_clark_state_t, zeroed by the caller before the first
 * call; every later call continues from it: k calls of n rounds give exactly
 * the bytes of one call of k * n.  All arithmetic is float32, every operation
 * rounded once, the one fused operation idg_clean's step 7.
 *
 * One round, run while reason == 0 (rounds counts the rounds begun):
 *   1. Peak.  P: the signed value at the residual's peak, as idg_clean defines
 *      it.  No peak: reason = IDG_CLEAN_NO_PEAK, the round ends.  started ==
 *      0: level = fmaxf(threshold, cycle_fraction * |P|), started = 1.
 *      !(|P| > level): reason = IDG_CLEAN_BELOW_LEVEL, the round ends.
 *   2. Limit.  f = fmaxf(level, select_fraction * |P|) (one rounded multiply).
 *      A pixel's bin is (bits(|s|) >> 19), 4096 bins: the exponent and four
 *      mantissa bits.  hist[b]: the searchable, non-NaN pixels of bin b.  b*:
 *      the least bin with sum_{b >= b*} hist[b] <= max_candidates (4096 when
 *      even the top occupied bin overflows).  tbits = max(bits(f) + 1,
 *      b* << 19) as unsigned 32-bit integers; round_limit = the float with
 *      those bits.
 *   3. Candidates: the searchable, non-NaN pixels with bits(|s|) >= tbits, at
 *      most max_candidates by construction; n_candidates = their number.
 *      None: reason = IDG_CLARK_NO_CANDIDATE, the round ends.  The list is a
 *      set: no output depends on its order.
 *   4. Cycle, at most iterations_per_round times: the list's peak (largest
 *      |value|, ties to the lowest linear index).  None, or its bits(|value|)
 *      < tbits: the round goes to step 5 with reason still 0.  Otherwise
 *      steps 3 to 6 of idg_clean's iteration on it (a stop there -- only
 *      IDG_CLEAN_COMPONENTS_FULL can occur -- sends the round to step 5 with
 *      that reason), and for every list entry (y, x) inside the component's
 *      patch: value = fmaf(-c, psf[dy][dx], value).
 *   5. Apply: the components this round recorded are subtracted from the
 *      whole residual, each over its patch as idg_clean's step 7, at every
 *      pixel in record order.  A round that took no component leaves the
 *      residual untouched.
 * After the call state.peak and state.peak_index describe the residual as it
 * stands, as for idg_clean; nr_rounds = 0 refreshes those two and nothing
 * else.
 *
 * What follows: (A) the residual is, bit for bit, the one from which the same
 * components were subtracted one at a time by idg_clean's step 7; (B) after a
 * round's apply the residual at every candidate equals that candidate's final
 * list value; (C) whenever the whole residual's peak is a list member at every
 * iteration, components, model, residual and n_components are idg_clean's.
 *
 * IDG_E_INVALID_ARGUMENT (every buffer left as it was): idg_clean's list with
 * nr_rounds and iterations_per_round in place of nr_iterations (both >= 0),
 * select_fraction not finite or outside [0, 1], max_candidates outside
 * [1, 16384]; on a state with n_components outside [0, max_components] the
 * _launch form, which reads nothing back, runs no round. */
#define IDG_CLARK_NO_CANDIDATE 4 /* state.reason, beside IDG_CLEAN_*          */

typedef struct idg_clark_params_t {
  uint32_t struct_size; /* sizeof(idg_clark_params_t)                        */
  int32_t grid_size;    /* G                                                 */
  int32_t psf_size;     /* Gp                                                */
  int32_t max_components;
  int32_t nr_rounds;    /* rounds of this call                               */
  int32_t iterations_per_round;
  int32_t max_candidates; /* 1 .. 16384                                      */
  float gain;
  float threshold;
  float cycle_fraction;
  float select_fraction; /* in [0, 1]                                        */
} idg_clark_params_t;

typedef struct idg_clark_state_t {
  int32_t n_components; /* the six fields of idg_clean_state_t               */
  int32_t reason;       /* IDG_CLEAN_* or IDG_CLARK_NO_CANDIDATE             */
  int32_t started;
  int32_t peak_index;
  float level;
  float peak;
  int32_t n_candidates; /* of the last round that reached step 3             */
  float round_limit;    /* of the last round that reached step 2             */
  int32_t rounds;       /* rounds begun so far                               */
} idg_clark_state_t;

int idg_clark(const idg_clark_params_t *params, float *residual,
              const float *psf, const uint8_t *mask, float *model,
              idg_clean_component_t *components, idg_clark_state_t *state);
/* Five launches per round plus three: a caller who wants to stop early reads
 * state->reason between calls of a few rounds each. */
int idg_clark_launch(const idg_clark_params_t *params, float *residual,
                     const float *psf, const uint8_t *mask, float *model,
                     idg_clean_component_t *components,
                     idg_clark_state_t *state, void *stream);

/* ---- restore: clean beam and restored image --------------------
 * model and residual -> the image an imager hands over: the model convolved
 * with a Gaussian clean beam fitted to the PSF's main lobe, plus the residual.
 * No reference counterpart.  All planes are single float32 [G][G] planes (the
 * Stokes-I convention of the CLEAN entries).  Three parts: the beam fit and
 * the tap table are host only, tiny and in doubles; the restore itself has a
 * host form and a _launch form that produce the same bytes.
 *
 * Beam.  exp(-(a dx^2 + 2 b dx dy + c dy^2)), dx and dy in pixels, peak 1: a
 * component of flux f restores to a peak of f.  major >= minor: the FWHMs in
 * pixels along the eigen-directions of the form, 2 sqrt(ln 2 / lambda).  pa:
 * the angle of the major axis from +x towards +y, in (-pi/2, pi/2].
 * idg_beam_from_axes fills a, b, c from the three numbers (major >= minor >
 * 0, pa finite; pa is brought into the range); idg_beam_fit fills all six.
 * Both read beam->struct_size (the rules of idg_options_t) and write the
 * fields it has room for.  idg_beam_radius and idg_beam_taps read a, b, c only.
 *
 * Fit.  idg_beam_fit(psf_size = Gp, psf [Gp][Gp], level, beam): host
 * pointers, no device.  Centre (Gp / 2, Gp / 2); p0 = psf[centre] must be
 * finite and > 0; q = (double)psf / (double)p0.  Region: the pixels with
 * q >= level that are 4-connected to the centre through such pixels, inside
 * the psf and within |dy|, |dx| <= 32 (0 < level < 1; 0.5 is the usual
 * choice); a sidelobe above the level that is not connected to the centre is
 * left out.  Over the region in row-major order, in doubles, the 3 x 3 normal
 * equations of min sum w (a dx^2 + b2 dx dy + c dy^2 + ln q)^2 with w = q^2
 * and b2 = 2 b (the weights make the log-linear fit approximate the
 * least-squares fit of the Gaussian itself), solved by elimination.
 * IDG_E_INVALID_ARGUMENT, *beam untouched, idg_last_error() saying which: a
 * bad struct_size; a NULL pointer, psf_size < 1 or level outside (0, 1); a
 * centre not finite and positive; fewer than three region pixels besides the
 * centre; a region that touches the +-32 window's edge (lobe too wide); a
 * singular or non-finite system; a solution with a <= 0, c <= 0 or
 * a c - b^2 <= 0.
 *
 * Taps.  idg_beam_radius returns floor(sqrt(-ln(cutoff) / lambda_min)), the
 * largest integer distance along the major axis at which the beam is still
 * >= cutoff; IDG_E_INVALID_ARGUMENT if cutoff is not in (0, 1), the beam's
 * form is not positive definite or the result exceeds 32.  idg_beam_taps
 * writes taps[dy + R][dx + R] = (float)exp(-(a dx^2 + 2 b dx dy + c dy^2)),
 * 0 <= R <= 32: the exponent in doubles in exactly that association (dx^2,
 * dx dy and dy^2 are exact integers), libm exp.  The taps are an input of the
 * restore, as psf is an input of idg_clean: both forms read the same table.
 *
 * Restore.  model, residual (NULL: none), restored: float32 [G][G], 1 <= G <=
 * 16384; taps: float32 [2R + 1][2R + 1], 0 <= R <= 32.  For every (y, x):
 *   acc = +0.0f
 *   for (y', x') in row-major order, |y - y'| <= R, |x - x'| <= R, inside the
 *   image:
 *     m = model[y'][x'];  if (m == 0.0f) continue;     (+-0 skipped, NaN taken)
 *     acc = fmaf(m, taps[y - y' + R][x - x' + R], acc)
 *   restored[y][x] = (residual ? residual[y][x] : 0.0f) + acc   (one add)
 * The skip is part of the contract: with it the bytes do not depend on
 * whether an implementation visits the zero pixels, even for non-finite taps.
 * restored may be the same pointer as residual (a pixel reads only its own
 * residual).  IDG_E_INVALID_ARGUMENT, every buffer left as it was: a bad
 * struct_size, a size out of range, a NULL model, taps or restored, any other
 * overlap among the four buffers, and (host form) a tap that is not finite.
 * idg_restore takes host pointers and needs no device; its cost follows the
 * number of non-zero model pixels. */
typedef struct idg_beam_t {
  uint32_t struct_size; /* sizeof(idg_beam_t)                                */
  double a, b, c;
  double major, minor, pa;
} idg_beam_t;

typedef struct idg_restore_params_t {
  uint32_t struct_size; /* sizeof(idg_restore_params_t)                      */
  int32_t grid_size;    /* G                                                 */
  int32_t radius;       /* R                                                 */
} idg_restore_params_t;

int idg_beam_from_axes(double major, double minor, double pa,
                       idg_beam_t *beam);
int idg_beam_fit(int psf_size, const float *psf, float level,
                 idg_beam_t *beam);
/* >= 0: the radius. */
int idg_beam_radius(const idg_beam_t *beam, double cutoff);
int idg_beam_taps(const idg_beam_t *beam, int radius, float *taps);

int idg_restore(const idg_restore_params_t *params, const float *model,
                const float *residual, const float *taps, float *restored);
/* Device pointers; asynchronous on `stream`: one launch, nothing read back,
 * no synchronisation, nothing allocated.  It cannot read the taps, so a tap
 * that is not finite is not refused here: it goes into the sums as it is. */
int idg_restore_launch(const idg_restore_params_t *params, const float *model,
                       const float *residual, const float *taps,
                       float *restored, void *stream);

/* ---- multi-scale CLEAN -----------------------------------------
 * The minor cycle of idg_clean over Ns scale-convolved residual planes
 * (Cornwell 2008): a component is a Gaussian blob of one of Ns widths, found
 * as the peak over all planes and subtracted from every plane with the
 * cross-PSF of its scale and the plane's.  No reference counterpart.  Three
 * layers, each with a host form (host pointers, no device needed) and a
 * _launch form (device pointers, asynchronous on `stream`, nothing read back,
 * no synchronisation, scratch from the workspace cache only); both forms
 * produce the same bytes in every output.  Every float operation is one
 * rounded float32 operation; fmaf is fused.
 *
 * Scales.  A scale a >= 0 is a width in pixels.  a = 0 is the delta: radius
 * 0, taps {1.0f}.  a > 0: sigma = a * 3 / 16, r = ceil(3 sigma) <= 48, and
 *   h[k + r] = (float)(exp(-k^2 / (2 sigma^2)) / sum_j exp(-j^2 / (2 sigma^2)))
 * in doubles, the sum over j = -r ... r in ascending order; the 2-D kernel is
 * the outer product.  idg_ms_scale_radius returns r, or
 * IDG_E_INVALID_ARGUMENT for a negative or NaN scale or r > 48;
 * idg_ms_scale_taps writes the 2 r + 1 taps for radius = that r (host only).
 * Like the restore taps, the tables are inputs of everything below.
 *
 * Convolution.  in, tmp, out: float32 [G][G], 1 <= G <= 16384; taps: float32
 * [2 r + 1], 0 <= r <= 48.  The image is zero beyond its edge:
 *   row pass:    tmp[y][x] = acc, acc = +0.0f; for k = -r ... r ascending with
 *                0 <= x + k < G:  acc = fmaf(in[y][x + k], taps[k + r], acc)
 *   column pass: out[y][x] = acc, acc = +0.0f; for k = -r ... r ascending with
 *                0 <= y + k < G:  acc = fmaf(tmp[y + k][x], taps[k + r], acc)
 * No zero is skipped; NaN and +-inf go in as they are (with taps {1} the
 * output is the input except that -0 becomes +0).  out may be in; tmp must be
 * distinct from both; any other overlap is IDG_E_INVALID_ARGUMENT, as are a
 * NULL buffer and a size out of range.
 *
 * Prepare.  idg_ms_params_t: G, Gp (1 <= Gp <= G), 1 <= Ns <= 8 and
 * radius[s]; radius[0] must be 0 (scale 0 is the delta).  taps: every scale's
 * taps one after the other, scale s at offset sum_{j < s} (2 radius[j] + 1).
 * residual [G][G], psf [Gp][Gp] (centre (Gp / 2, Gp / 2)), tmp [G][G];
 * planes [Ns][G][G]; cross_psf [Ns (Ns + 1) / 2][Gp][Gp], the patch of
 * (s, q), s <= q, at index s Ns - s (s - 1) / 2 + (q - s).
 *   planes[0] = residual, a copy (planes may be residual itself);
 *   planes[s] = convolve(residual, h_s), s >= 1;
 *   cross(s, q) = convolve(convolve(psf, h_s), h_q) on the [Gp][Gp] window:
 *   the PSF is zero outside it and the result is truncated to it; each is a
 *   full row-then-column convolution as above.  cross(q, s) is cross(s, q).
 * The other fields of the struct are not read.
 *
 * Minor cycle.  planes, cross_psf and taps as prepare leaves them; mask uint8
 * [G][G] or NULL, limiting the search on every scale and never the
 * subtraction; model float32 [G][G], accumulated onto; components
 * [max_components]; state: input and output, zeroed by the caller before the
 * first call: k calls of n iterations give the bytes of one call of k * n.
 * weight[s] and inv_peak[s] are the caller's: the usual choice is inv_peak[s]
 * = 1 / cross(s, s)[centre] and weight[s] = (1 - bias a_s / a_max)
 * inv_peak[s].
 * Peak: over every scale s and every searchable pixel whose planes[s] value
 * v is not NaN, the largest u = |weight[s] * v| (one rounded multiply; a NaN
 * u is excluded too); ties go to the lowest scale, then the lowest linear
 * index.  One iteration: steps 1 to 5 of idg_clean with u in place of |v|,
 * then for the peak (py, px) of scale s, value v:
 *   6. c = (gain * v) * inv_peak[s] (two rounded multiplies);
 *      components[n_components++] = {py, px, s, c}.
 *   7. every (y, x) inside the image with |y - py| <= r and |x - px| <= r, r
 *      = radius[s], h = scale s's taps:
 *      model[y][x] += (c * h[y - py + r]) * h[x - px + r]   (one add)
 *   8. every scale q and every (y, x) of idg_clean's step 7:
 *      planes[q][y][x] = fmaf(-c, cross(s, q)[dy][dx], planes[q][y][x]).
 * After the call state.peak = u, peak_index and peak_scale describe the planes
 * as they stand (0, -1, -1 if there is no peak).  The residual to hand on is
 * planes[0].
 *
 * IDG_E_INVALID_ARGUMENT (every buffer left as it was): idg_clean's list, Ns
 * outside [1, 8], a radius outside [0, 48] or radius[0] != 0, a weight or
 * inv_peak of a used scale that is not finite, and (host form) a state with
 * n_components outside [0, max_components]; on such a state the _launch form
 * runs no iteration. */
#define IDG_MS_MAX_SCALES 8
#define IDG_MS_MAX_RADIUS 48

typedef struct idg_ms_params_t {
  uint32_t struct_size; /* sizeof(idg_ms_params_t)                           */
  int32_t grid_size;    /* G                                                 */
  int32_t psf_size;     /* Gp                                                */
  int32_t max_components;
  int32_t nr_iterations;
  float gain;
  float threshold;
  float cycle_fraction;
  int32_t nr_scales;    /* Ns                                                */
  int32_t radius[IDG_MS_MAX_SCALES];
  float weight[IDG_MS_MAX_SCALES];
  float inv_peak[IDG_MS_MAX_SCALES];
} idg_ms_params_t;

typedef struct idg_ms_component_t {
  int32_t y, x, scale;
  float value;
} idg_ms_component_t;

typedef struct idg_ms_state_t {
  int32_t n_components;
  int32_t reason;     /* IDG_CLEAN_*                                         */
  int32_t started;
  int32_t peak_index; /* y * G + x of the peak, -1: none                     */
  float level;
  float peak;         /* |weight[peak_scale] * v| there                      */
  int32_t peak_scale; /* -1: none                                            */
} idg_ms_state_t;

/* >= 0: the radius. */
int idg_ms_scale_radius(double scale);
int idg_ms_scale_taps(double scale, int radius, float *taps);

int idg_convolve_separable(int grid_size, int radius, const float *in,
                           const float *taps, float *tmp, float *out);
/* Two launches, nothing allocated. */
int idg_convolve_separable_launch(int grid_size, int radius, const float *in,
                                  const float *taps, float *tmp, float *out,
                                  void *stream);

int idg_ms_prepare(const idg_ms_params_t *params, const float *residual,
                   const float *psf, const float *taps, float *planes,
                   float *cross_psf, float *tmp);
int idg_ms_prepare_launch(const idg_ms_params_t *params, const float *residual,
                          const float *psf, const float *taps, float *planes,
                          float *cross_psf, float *tmp, void *stream);

int idg_ms_clean(const idg_ms_params_t *params, float *planes,
                 const float *cross_psf, const float *taps,
                 const uint8_t *mask, float *model,
                 idg_ms_component_t *components, idg_ms_state_t *state);
/* One launch per iteration plus two, as idg_clean_launch. */
int idg_ms_clean_launch(const idg_ms_params_t *params, float *planes,
                        const float *cross_psf, const float *taps,
                        const uint8_t *mask, float *model,
                        idg_ms_component_t *components, idg_ms_state_t *state,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif /* IDG_MI355X_H_ */
