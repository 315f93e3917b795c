// util.cpp -- HIP launch-and-buffer layer and MI355X runtime (see util.hpp).
#include "util.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <map>
#include <mutex>
#include <memory>
#include <sstream>
#include <thread>
#include <tuple>
#include <utility>

#include "lib-hip.hpp"
#include "hip/kernels/device.hpp"

namespace hip {

void hip_assert(hipError_t code, const char *file, int line, bool abort) {
  if (code == hipSuccess) return;
  std::fprintf(stderr, "GPUassert: %s %s %d\n", hipGetErrorString(code), file,
               line);
  if (abort) std::exit(static_cast<int>(code));
}

namespace {
hipDeviceProp_t current_props() {
  int dev = 0;
  hipCheck(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  hipCheck(hipGetDeviceProperties(&prop, dev));
  return prop;
}
}  // namespace

std::string get_device_name() {
  std::string name = current_props().name;
  std::replace(name.begin(), name.end(), ' ', '_');
  return name;
}

std::string extern_get_device_name() { return get_device_name(); }

void print_device_info() {
  const hipDeviceProp_t prop = current_props();
  std::cout << "\nDevice Name " << prop.name << " (" << prop.gcnArchName
            << ")\n"
            << "  Memory Clock Rate (KHz): " << prop.memoryClockRate << "\n"
            << "  Memory Bus Width (bits): " << prop.memoryBusWidth << "\n"
            << "  Peak Memory Bandwidth (GB/s): "
            << 2.0 * prop.memoryClockRate * (prop.memoryBusWidth / 8) / 1.0e6
            << "\n"
            << "  Memory size (GB): " << prop.totalGlobalMem / 1e9 << "\n"
            << "  Compute Units: " << prop.multiProcessorCount << "\n"
            << std::endl;
}

std::vector<int> get_launch_kernel_dimensions() {
  const hipDeviceProp_t prop = current_props();
  return {prop.multiProcessorCount, prop.maxThreadsPerBlock};
}

int get_cu_nr() { return current_props().multiProcessorCount; }
int get_max_threads() { return current_props().maxThreadsPerBlock; }
size_t get_gmem_size() { return current_props().totalGlobalMem; }
int get_cu_freq() { return current_props().clockRate; }

void print_dimensions(dim3 g, dim3 b) {
  std::cout << "Dimensions: (" << g.x << "," << g.y << "," << g.z << ") - ("
            << b.x << "," << b.y << "," << b.z << ")\n"
            << std::endl;
}

namespace {
// The timed loop of p_run_kernel: `once` enqueues one iteration on the
// legacy default stream.
double time_iterations(const std::function<void()> &once,
                       const std::string &func_name, double gflops,
                       double gbytes, double mvis) {
  const int warm = static_cast<int>(get_env_var("NR_WARM_UP_RUNS", 2));
  const int iters =
      std::max(1, static_cast<int>(get_env_var("NR_ITERATIONS", 5)));
  hipEvent_t start, stop;
  hipCheck(hipEventCreate(&start));
  hipCheck(hipEventCreate(&stop));
  for (int i = 0; i < warm; ++i) once();
  hipCheck(hipDeviceSynchronize());
  hipCheck(hipEventRecord(start, nullptr));
  for (int i = 0; i < iters; ++i) once();
  hipCheck(hipEventRecord(stop, nullptr));
  hipCheck(hipEventSynchronize(stop));
  float ms = 0.0f;
  hipCheck(hipEventElapsedTime(&ms, start, stop));
  hipCheck(hipEventDestroy(start));
  hipCheck(hipEventDestroy(stop));
  const double seconds = 1e-3 * ms / iters;
  report(func_name, seconds, gflops, gbytes, mvis);
  report_csv(func_name, get_device_name(), "-hip.csv", seconds, gflops, gbytes,
             mvis);
  return seconds;
}

// One kernel per iteration, or the two-kernel form of the MI355X kernels
// (util.hpp KernelChoice::parts).
double time_launches(const idg_mi355x::KernelChoice &k, dim3 gridDim,
                     void **args, const std::string &func_name, double gflops,
                     double gbytes, double mvis) {
  return time_iterations(
      [&] {
        if (k.parts[1].func)
          hipCheck(idg_mi355x::launch_parts(
              k, static_cast<int>(gridDim.x), args,
              *static_cast<float *>(args[3]) != 0.0f, nullptr));
        else
          hipCheck(hipLaunchKernel(k.func, gridDim, dim3(k.block), args, 0,
                                   nullptr));
      },
      func_name, gflops, gbytes, mvis);
}
}  // namespace

double p_run_kernel(const void *func, dim3 gridDim, dim3 blockDim,
                    void **args, std::string func_name, double gflops,
                    double gbytes, double mvis) {
  idg_mi355x::KernelChoice k;
  k.func = func;
  k.block = static_cast<int>(blockDim.x);
  return time_launches(k, gridDim, args, func_name, gflops, gbytes, mvis);
}

void c_run_kernel(const void *func, dim3 gridDim, dim3 blockDim, void **args) {
  hipCheck(hipLaunchKernel(func, gridDim, blockDim, args, 0, nullptr));
}

void p_run_gridder_(const void *func, std::string func_name, int num_threads) {
  idg_mi355x::run_performance(idg_mi355x::Direction::kGridder, func,
                              func_name, num_threads);
}

void p_run_degridder_(const void *func, std::string func_name,
                      int num_threads) {
  idg_mi355x::run_performance(idg_mi355x::Direction::kDegridder, func,
                              func_name, num_threads);
}

namespace {
// Shared body of c_run_gridder_ / c_run_degridder_: the reference semantics
// (allocate, copy in, one launch, copy out, free) with validation.
void c_run_common(idg_mi355x::Direction dir, int nr_subgrids, int grid_size,
                  int subgrid_size, float image_size, float w_step_in_lambda,
                  int nr_channels, int nr_stations,
                  idg::Array2D<idg::UVWCoordinate<float>> &uvw,
                  idg::Array1D<float> &wavenumbers,
                  idg::Array3D<idg::Visibility<std::complex<float>>> &vis,
                  idg::Array2D<float> &spheroidal,
                  idg::Array4D<idg::Matrix2x2<std::complex<float>>> &aterms,
                  idg::Array1D<idg::Metadata> &metadata,
                  idg::Array4D<std::complex<float>> &subgrids,
                  const void *func, int num_threads) {
  idg_mi355x::Problem p;
  p.nr_subgrids = nr_subgrids;
  p.grid_size = grid_size;
  p.subgrid_size = subgrid_size;
  p.image_size = image_size;
  p.w_step_in_lambda = w_step_in_lambda;
  p.nr_channels = nr_channels;
  p.nr_stations = nr_stations;
  idg_mi355x::Extents e;
  e.uvw_rows = uvw.size();
  e.aterm_slots = aterms.get_w_dim();
  std::string msg;
  idg_mi355x::KernelChoice force;
  force.func = func;
  force.name = "caller-supplied";
  force.block = num_threads;
  const hipError_t err = idg_mi355x::run_host(
      dir, p, e, uvw.data(), wavenumbers.data(), vis.data(),
      spheroidal.data(), aterms.data(), metadata.data(), subgrids.data(),
      &msg, func ? &force : nullptr);
  if (!msg.empty()) {
    std::fprintf(stderr, "idg-mi355x: %s\n", msg.c_str());
    std::exit(EXIT_FAILURE);
  }
  hipCheck(err);
}
}  // namespace

// The func/num_threads arguments of the reference signature are honoured:
// a kernel with the 13-argument ABI is launched with grid = nr_subgrids,
// block = num_threads; func == nullptr selects the MI355X kernel.
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
    int num_threads) {
  c_run_common(idg_mi355x::Direction::kGridder, nr_subgrids, grid_size,
               subgrid_size, image_size, w_step_in_lambda, nr_channels,
               nr_stations, uvw, wavenumbers, visibilities, spheroidal, aterms,
               metadata, subgrids, func, num_threads);
}

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
    int num_threads) {
  c_run_common(idg_mi355x::Direction::kDegridder, nr_subgrids, grid_size,
               subgrid_size, image_size, w_step_in_lambda, nr_channels,
               nr_stations, uvw, wavenumbers, visibilities, spheroidal, aterms,
               metadata, subgrids, func, num_threads);
}

void print_benchmark() {
  std::cout << ">>> hip IDG BENCHMARK (MI355X / gfx950)" << std::endl;
}

}  // namespace hip

namespace idg_mi355x {

// The one reader of the mode variables: a field the caller left unset takes
// its variable's value, else the library's default.
Options resolve_options(const Options &request) {
  if (request.resolved) return request;
  Options o = request;
  const auto env = [](const char *name) {
    const char *v = std::getenv(name);
    return std::string(v ? v : "");
  };
  if (o.gridder_impl == 0) {
    // valu: the VALU mirror path (A/B comparisons); sequential: the
    // order-preserving kernel, bit-exact to the reference's CPU output;
    // ordered: the reference's summation order with the hardware sin / cos;
    // auto: ordered per subgrid above auto_threshold, else the MFMA kernels
    const std::string v = env("IDG_GRIDDER_IMPL");
    o.gridder_impl = v == "sequential" ? kImplSequential
                     : v == "ordered"  ? kImplOrdered
                     : v == "auto"     ? kImplAuto
                     : v == "valu"     ? kImplValu
                                       : kImplDefault;
  }
  if (o.degridder_impl == 0) {
    const std::string v = env("IDG_DEGRIDDER_IMPL");
    o.degridder_impl = v == "sequential" ? kImplSequential
                       : v == "valu"     ? kImplValu
                                         : kImplDefault;
  }
  if (o.precision == 0)
    if (const char *v = std::getenv("IDG_PREC"))
      o.precision = kPrecSet | (std::atoi(v) & 7);
  if (o.kernel_form == 0) {
    const std::string v = env("IDG_KERNEL_FORM");
    o.kernel_form = v == "combined" ? kFormCombined
                    : v == "split"  ? kFormSplit
                                    : kFormBySize;
  }
  if (o.fft_fusion == 0)
    o.fft_fusion = env("IDG_GRID_FFT")[0] == '0' ? kFftFusionOff : kFftFusionOn;
  if (o.auto_threshold == 0) o.auto_threshold = kAutoThreshold;
  o.resolved = true;
  return o;
}

bool two_kernel_form(int nr_subgrids, const Options &opt) {
  const int form = resolve_options(opt).kernel_form;
  if (form == kFormCombined) return false;
  if (form == kFormSplit) return true;
  return nr_subgrids >= kTwoKernelMinLaunch;
}

bool auto_selects(long long nr_timesteps, long long nr_channels,
                  unsigned threshold) {
  return nr_timesteps > 0 &&
         nr_timesteps * nr_channels > static_cast<long long>(threshold);
}

int precision_for(Direction dir, const Problem &p, const Options &opt) {
  const int forced = resolve_options(opt).precision;
  if (forced & kPrecSet) return forced & 7;
  // degridder: no reduction tail (its visibilities are not coherent sums
  // over channels; measured 1.00e-6 vs 0.97e-6 from exact at the -c
  // defaults, 8.1e-7 vs 6.7e-7 at C = 256, for 5 % of its time)
  if (dir == Direction::kDegridder) return 0;
  // gridder: the reduction tail on every phasor.  The one-channel-per-quad
  // tail (kPrecTailAlt, IDG_PREC=4: a quarter of the adds) cancels only
  // where a quad's four terms are coherent; on channel-incoherent
  // visibilities it left the gridder farther from exact than the reference's
  // own f32 sum (round 5: 1.31e-6 against 0.79e-6 at C = 16,
  // tests/test_gpu_accuracy.py::test_tail_patterns_on_channel_incoherent_
  // visibilities), so it is no longer the default
  return kPrecTail | (p.nr_channels > kTailMinChannels ? kPrecFlush : 0);
}

std::string validate(const Problem &p, const Extents &e,
                     const idg::Metadata *md) {
  std::ostringstream err;
  if (p.nr_subgrids < 0) return "nr_subgrids < 0";
  if (p.nr_subgrids == 0) return "";
  if (p.subgrid_size <= 0) return "subgrid_size must be > 0";
  if (p.nr_channels <= 0) return "nr_channels must be > 0";
  if (p.nr_stations <= 0) return "nr_stations must be > 0";
  if (md == nullptr) return "metadata is null";
  const long long bo0 = md[0].baseline_offset;
  for (int s = 0; s < p.nr_subgrids; ++s) {
    const idg::Metadata &m = md[s];
    const long long t0 = (m.baseline_offset - bo0) + (long long)m.time_offset;
    if (m.nr_timesteps < 0 || t0 < 0 ||
        t0 + m.nr_timesteps > static_cast<long long>(e.uvw_rows)) {
      err << "subgrid " << s << ": timesteps [" << t0 << ", "
          << t0 + m.nr_timesteps << ") outside uvw/visibility rows [0, "
          << e.uvw_rows << ")";
      return err.str();
    }
    if (m.aterm_index < 0 ||
        static_cast<size_t>(m.aterm_index) >= e.aterm_slots) {
      err << "subgrid " << s << ": aterm_index " << m.aterm_index
          << " outside [0, " << e.aterm_slots << ")";
      return err.str();
    }
    if (m.baseline.station1 >= static_cast<unsigned>(p.nr_stations) ||
        m.baseline.station2 >= static_cast<unsigned>(p.nr_stations)) {
      err << "subgrid " << s << ": station (" << m.baseline.station1 << ","
          << m.baseline.station2 << ") outside [0, " << p.nr_stations << ")";
      return err.str();
    }
  }
  return "";
}

hipError_t launch(Direction dir, const Problem &p, const void *d_uvw,
                  const float *d_wavenumbers, void *d_visibilities,
                  const float *d_spheroidal, const void *d_aterms,
                  const void *d_metadata, void *d_subgrids,
                  hipStream_t stream, const KernelChoice *force,
                  const Options &opt) {
  if (p.nr_subgrids <= 0) return hipSuccess;
  const KernelChoice k =
      force ? *force
            : (dir == Direction::kGridder ? select_gridder(p, opt)
                                          : select_degridder(p, opt));
  if (k.func == nullptr) return hipErrorInvalidConfiguration;
  int grid_size = p.grid_size, subgrid_size = p.subgrid_size;
  float image_size = p.image_size, w_step = p.w_step_in_lambda;
  int nr_channels = p.nr_channels, nr_stations = p.nr_stations;
  void *args[] = {&grid_size,     &subgrid_size,    &image_size,
                  &w_step,        &nr_channels,     &nr_stations,
                  &d_uvw,         &d_wavenumbers,   &d_visibilities,
                  &d_spheroidal,  &d_aterms,        &d_metadata,
                  &d_subgrids};
  const auto default_pass = [&]() {
    return (force || k.parts[1].func == nullptr)
               ? hipLaunchKernel(k.func, dim3(p.nr_subgrids), dim3(k.block),
                                 args, 0, stream)
               : launch_parts(k, p.nr_subgrids, args,
                              p.w_step_in_lambda != 0.0f, stream);
  };
  hipError_t err = hipSuccess;
  if (k.auto_ordered) {
    // classify on the device; the default kernels on the shadow metadata
    // (selected subgrids empty: zeros); the ordered kernel over the queue on
    // the true metadata.  Stream order alone separates the three.
    WorkspaceLease lease;
    err = lease.acquire(stream, kWorkspaceAuto,
                        auto_workspace_bytes(p.nr_subgrids));
    if (err != hipSuccess) return err;
    err = launch_auto_classify(p.nr_subgrids, p.nr_channels, k.auto_threshold,
                               d_metadata, lease.ptr, stream);
    const void *true_metadata = d_metadata;
    d_metadata = auto_shadow(lease.ptr, p.nr_subgrids);
    if (err == hipSuccess) err = default_pass();
    d_metadata = true_metadata;
    int slices = kAutoSlices;
    // IDG_AUTO_SLICES: the slicing A/B of tools/debug/auto_rate.py
    if (const char *v = std::getenv("IDG_AUTO_SLICES"))
      slices = std::max(1, std::min(64, std::atoi(v)));
    if (err == hipSuccess)
      err = launch_ordered_queue(p, args, lease.ptr, slices, stream);
  } else {
    err = default_pass();
  }
  if (err != hipSuccess || dir != Direction::kGridder || !p.fft_out ||
      k.fft_in_kernel)
    return err;
  return launch_subgrid_fft(p.nr_subgrids, p.subgrid_size, +1, 1.0f,
                            d_subgrids, stream);
}

// Workgroups of `func` (block threads) resident on the current device at
// once: occupancy x CUs, cached per (device, kernel).
int resident_workgroups(const void *func, int block) {
  static std::mutex mu;
  static std::map<std::pair<int, const void *>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(dev, func);
  const auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, func, block, 0) !=
          hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess)
    return 0;
  // IDG_PERSISTENT_PER_CU overrides the occupancy query (A/B)
  if (const char *v = std::getenv("IDG_PERSISTENT_PER_CU")) per_cu = std::atoi(v);
  const int n = std::max(1, per_cu) * std::max(1, cus);
  if (std::getenv("IDG_DEBUG_LAUNCH"))
    std::fprintf(stderr, "idg-mi355x: persistent grid %d (%d per CU x %d CUs)\n",
                 n, per_cu, cus);
  cache[key] = n;
  return n;
}

// Device workspaces cached per (device, stream, slot): one stream-ordered
// allocation per stream and use (grown when a launch needs more), so the
// launches that need one (the two-kernel form's queue, the pipeline's home
// sort) make no allocation or free per call.  A slot is
// leased for the enqueueing of one launch sequence; while another host
// thread holds it, the caller gets a private allocation freed after its
// sequence.
namespace {
struct WorkspaceSlot {
  void *ptr = nullptr;
  size_t bytes = 0;
  bool clean = false;
  bool busy = false;
};
std::mutex g_ws_mu;
std::map<std::tuple<int, hipStream_t, int>, WorkspaceSlot> g_ws;
}  // namespace

hipError_t WorkspaceLease::acquire(hipStream_t s, int slot, size_t bytes) {
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  stream = s;
  std::lock_guard<std::mutex> lock(g_ws_mu);
  WorkspaceSlot &w = g_ws[std::make_tuple(dev, s, slot)];
  if (w.busy) {
    private_ = true;
    clean = false;
    return hipMallocAsync(&ptr, bytes, s);
  }
  if (w.bytes < bytes) {
    if (w.ptr) {
      err = hipFreeAsync(w.ptr, s);
      if (err != hipSuccess) return err;
      w.ptr = nullptr;
      w.bytes = 0;
    }
    err = hipMallocAsync(&w.ptr, bytes, s);
    if (err != hipSuccess) return err;
    w.bytes = bytes;
    w.clean = false;
  }
  w.busy = true;
  clean = w.clean;
  w.clean = false;
  ptr = w.ptr;
  dev_ = dev;
  slot_ = slot;
  return hipSuccess;
}

WorkspaceLease::~WorkspaceLease() {
  if (ptr == nullptr) return;
  if (private_) {
    (void)hipFreeAsync(ptr, stream);
    return;
  }
  std::lock_guard<std::mutex> lock(g_ws_mu);
  WorkspaceSlot &w = g_ws[std::make_tuple(dev_, stream, slot_)];
  w.busy = false;
  w.clean = leave_clean;
}

hipError_t release_workspaces(hipStream_t stream, bool all) {
  int dev = 0;
  hipError_t err = hipGetDevice(&dev);
  if (err != hipSuccess) return err;
  std::lock_guard<std::mutex> lock(g_ws_mu);
  bool busy = false;
  for (auto it = g_ws.begin(); it != g_ws.end();) {
    if (std::get<0>(it->first) != dev ||
        (!all && std::get<1>(it->first) != stream)) {
      ++it;
      continue;
    }
    if (it->second.busy) {
      busy = true;
      ++it;
      continue;
    }
    // freed on the owning stream, so the free is ordered after every kernel
    // still queued there that uses the slot (torch streams do not
    // synchronise with the null stream), then that stream is waited for, so
    // the memory is gone when this returns
    if (it->second.ptr) {
      const hipStream_t owner = std::get<1>(it->first);
      hipError_t e = hipFreeAsync(it->second.ptr, owner);
      if (e == hipSuccess) e = hipStreamSynchronize(owner);
      if (e != hipSuccess && err == hipSuccess) err = e;
    }
    it = g_ws.erase(it);
  }
  if (err == hipSuccess && busy) err = hipErrorNotReady;
  return err;
}

hipError_t launch_parts(const KernelChoice &k, int nr_subgrids, void **args13,
                        bool all_general, hipStream_t stream) {
  if (nr_subgrids <= 0) return hipSuccess;
  const KernelChoice::Part &mirror = k.parts[0], &general = k.parts[1];
  if ((all_general || mirror.func == nullptr) && k.all_general.func)
    return hipLaunchKernel(k.all_general.func, dim3(nr_subgrids),
                           dim3(k.all_general.block), args13, 0, stream);
  const int resident = resident_workgroups(general.func, general.block);
  if (resident <= 0) return hipErrorInvalidConfiguration;
  // the queue's counters are zero when the workspace is new or the last
  // pair did not complete, and left zero by the general kernel's last
  // workgroup otherwise (device.hpp queue_retire)
  WorkspaceLease lease;
  hipError_t err = lease.acquire(stream, kWorkspaceQueue,
                                 queue_ints(nr_subgrids) * sizeof(int));
  if (err != hipSuccess) return err;
  int *queue = static_cast<int *>(lease.ptr);
  if (!lease.clean) {
    err = hipMemsetAsync(queue, 0, kQueueHead * sizeof(int), stream);
    if (err != hipSuccess) return err;
  }
  const bool run_mirror = mirror.func != nullptr && !all_general;
  int ns = nr_subgrids, all = run_mirror ? 0 : 1;
  void *args[16];
  for (int i = 0; i < 13; ++i) args[i] = args13[i];
  args[13] = &queue;
  args[14] = &ns;  // (the general kernel's; the mirror kernel takes 14)
  const int mirror_grid = nr_subgrids * mirror.per_subgrid;
  if (err == hipSuccess && run_mirror)
    err = hipLaunchKernel(mirror.func, dim3(mirror_grid), dim3(mirror.block),
                          args, 0, stream);
  args[15] = &all;
  if (err == hipSuccess)
    err = hipLaunchKernel(general.func, dim3(std::min(nr_subgrids, resident)),
                          dim3(general.block), args, 0, stream);
  // the general kernel's last workgroup zeroes the counters (device.hpp
  // queue_retire); after a failed launch they are cleared on the next use
  lease.leave_clean = err == hipSuccess;
  return err;
}

namespace {
// RAII device buffer.
struct DevBuf {
  void *ptr = nullptr;
  hipError_t alloc(size_t bytes) {
    return bytes ? hipMalloc(&ptr, bytes) : hipSuccess;
  }
  ~DevBuf() {
    if (ptr) (void)hipFree(ptr);
  }
};
#define IDG_TRY(x)                   \
  do {                               \
    hipError_t e_ = (x);             \
    if (e_ != hipSuccess) return e_; \
  } while (0)
}  // namespace

namespace {
// Visibility row intervals [first, second) of subgrids [s0, s1) in the row
// space of metadata[0] (the kernels' rebasing, device.hpp:setup_subgrid),
// merged and sorted.
std::vector<std::pair<long long, long long>> row_runs(
    const idg::Metadata *md, int s0, int s1) {
  std::vector<std::pair<long long, long long>> r;
  const long long bo0 = md[0].baseline_offset;
  for (int s = s0; s < s1; ++s) {
    const long long a = (md[s].baseline_offset - bo0) + md[s].time_offset;
    if (md[s].nr_timesteps > 0) r.emplace_back(a, a + md[s].nr_timesteps);
  }
  std::sort(r.begin(), r.end());
  std::vector<std::pair<long long, long long>> m;
  for (const auto &x : r) {
    if (!m.empty() && x.first <= m.back().second)
      m.back().second = std::max(m.back().second, x.second);
    else
      m.push_back(x);
  }
  return m;
}

struct Stream {
  hipStream_t s = nullptr;
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};
struct Event {
  hipEvent_t e = nullptr;
  hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
};
}  // namespace

int plan_host_chunks(const idg::Metadata *metadata, int nr_subgrids,
                     size_t moved, std::vector<int> *bounds,
                     std::vector<std::vector<std::pair<long long, long long>>>
                         *row_runs_out) {
  std::vector<int> sb;
  std::vector<std::vector<std::pair<long long, long long>>> runs;
  int nchunk = static_cast<int>(std::min<size_t>(16, moved >> 27));
  nchunk = std::max(1, std::min(nchunk, nr_subgrids / 256));
  sb.resize(nchunk + 1);
  runs.resize(nchunk);
  for (int i = 0; i <= nchunk; ++i)
    sb[i] = static_cast<int>(static_cast<long long>(nr_subgrids) * i / nchunk);
  // Chunks must be disjoint AND ascending in rows: each chunk's first row
  // is compared with the largest row end of EVERY earlier chunk (a chunk
  // with no rows, e.g. only zero-timestep subgrids, must not hide an
  // overlap between its neighbours).
  bool disjoint = true;
  long long row_end = -1;  // max row end over the chunks so far
  for (int i = 0; i < nchunk; ++i) {
    runs[i] = row_runs(metadata, sb[i], sb[i + 1]);
    if (runs[i].empty()) continue;
    if (runs[i].front().first < row_end) disjoint = false;
    row_end = std::max(row_end, runs[i].back().second);
  }
  if (!disjoint) {  // one chunk: every row any subgrid reads or writes
    nchunk = 1;
    sb = {0, nr_subgrids};
    runs = {row_runs(metadata, 0, nr_subgrids)};
  }
  if (bounds) *bounds = std::move(sb);
  if (row_runs_out) *row_runs_out = std::move(runs);
  return nchunk;
}

// The reference's c_run_* contract (app/HIP/util.cpp:255-311: allocate, copy
// in, launch once, copy out, free) on host buffers.  Large batches are split
// into chunks of consecutive subgrids whose visibility rows do not overlap:
// chunk i's input is copied in while chunk i-1 computes, and a second host
// thread copies chunk i-2's output back meanwhile (pageable copies block the
// thread that issues them, so each direction gets its own), so the two PCIe
// directions and the kernel overlap.  The degridder copies back only the
// rows its subgrids reference, so it need not upload the caller's
// visibilities to preserve the others.
hipError_t run_host(Direction dir, const Problem &p, const Extents &e,
                    const void *uvw, const float *wavenumbers,
                    void *visibilities, const float *spheroidal,
                    const void *aterms, const idg::Metadata *metadata,
                    void *subgrids, std::string *msg,
                    const KernelChoice *force, const Options &request) {
  const Options opt = resolve_options(request);  // one read for every chunk
  const std::string bad = validate(p, e, metadata);
  if (!bad.empty()) {
    if (msg) *msg = bad;
    return hipErrorInvalidValue;
  }
  if (p.nr_subgrids == 0) return hipSuccess;
  const size_t S = static_cast<size_t>(p.subgrid_size);
  const size_t row_b = static_cast<size_t>(p.nr_channels) * 4 * 2 * sizeof(float);
  const size_t b_uvw = e.uvw_rows * 3 * sizeof(float);
  const size_t b_wn = static_cast<size_t>(p.nr_channels) * sizeof(float);
  const size_t b_vis = e.uvw_rows * row_b;
  const size_t b_sph = S * S * sizeof(float);
  const size_t b_at = e.aterm_slots * p.nr_stations * S * S * 4 * 2 *
                      sizeof(float);
  const size_t b_md = static_cast<size_t>(p.nr_subgrids) * sizeof(idg::Metadata);
  const size_t sg_b = 4 * S * S * 2 * sizeof(float);  // one subgrid
  const size_t b_sg = static_cast<size_t>(p.nr_subgrids) * sg_b;
  DevBuf d_uvw, d_wn, d_vis, d_sph, d_at, d_md, d_sg;
  IDG_TRY(d_uvw.alloc(b_uvw));
  IDG_TRY(d_wn.alloc(b_wn));
  IDG_TRY(d_vis.alloc(b_vis));
  IDG_TRY(d_sph.alloc(b_sph));
  IDG_TRY(d_at.alloc(b_at));
  IDG_TRY(d_md.alloc(b_md));
  IDG_TRY(d_sg.alloc(b_sg));
  const hipMemcpyKind h2d = hipMemcpyHostToDevice;
  const hipMemcpyKind d2h = hipMemcpyDeviceToHost;
  IDG_TRY(hipMemcpy(d_uvw.ptr, uvw, b_uvw, h2d));
  IDG_TRY(hipMemcpy(d_wn.ptr, wavenumbers, b_wn, h2d));
  IDG_TRY(hipMemcpy(d_sph.ptr, spheroidal, b_sph, h2d));
  IDG_TRY(hipMemcpy(d_at.ptr, aterms, b_at, h2d));
  IDG_TRY(hipMemcpy(d_md.ptr, metadata, b_md, h2d));

  // Chunks: ~128 MB of copies each, at most 16, at least 256 subgrids.
  const bool grid = dir == Direction::kGridder;
  std::vector<int> sb;
  std::vector<std::vector<std::pair<long long, long long>>> runs;
  const int nchunk =
      plan_host_chunks(metadata, p.nr_subgrids, b_vis + b_sg, &sb, &runs);

  int dev = 0;
  IDG_TRY(hipGetDevice(&dev));
  Stream s_in, s_k, s_out;
  IDG_TRY(s_in.create());
  IDG_TRY(s_k.create());
  IDG_TRY(s_out.create());
  std::vector<Event> e_in(nchunk), e_k(nchunk);
  for (int i = 0; i < nchunk; ++i) {
    IDG_TRY(e_in[i].create());
    IDG_TRY(e_k[i].create());
  }
  char *vis_h = static_cast<char *>(visibilities);
  char *sg_h = static_cast<char *>(subgrids);
  char *vis_d = static_cast<char *>(d_vis.ptr);
  char *sg_d = static_cast<char *>(d_sg.ptr);

  // Output copies on their own thread: chunk i's once its kernel is done.
  std::atomic<int> launched{0};
  std::atomic<bool> abort_out{false};
  hipError_t out_err = hipSuccess;
  std::thread out([&] {
    hipError_t err = hipSetDevice(dev);
    for (int i = 0; i < nchunk && err == hipSuccess; ++i) {
      while (launched.load(std::memory_order_acquire) <= i) {
        if (abort_out.load(std::memory_order_acquire)) return;
        std::this_thread::yield();
      }
      err = hipEventSynchronize(e_k[i].e);
      if (err != hipSuccess) break;
      if (grid) {
        const size_t off = static_cast<size_t>(sb[i]) * sg_b;
        err = hipMemcpyAsync(sg_h + off, sg_d + off,
                             static_cast<size_t>(sb[i + 1] - sb[i]) * sg_b, d2h,
                             s_out.s);
      } else {
        for (const auto &r : runs[i]) {
          err = hipMemcpyAsync(vis_h + r.first * row_b, vis_d + r.first * row_b,
                               static_cast<size_t>(r.second - r.first) * row_b,
                               d2h, s_out.s);
          if (err != hipSuccess) break;
        }
      }
      if (err == hipSuccess) err = hipStreamSynchronize(s_out.s);
    }
    out_err = err;
  });

  hipError_t err = hipSuccess;
  for (int i = 0; i < nchunk && err == hipSuccess; ++i) {
    // input of chunk i (overlaps chunk i-1's kernel and output copy)
    if (grid) {
      for (const auto &r : runs[i]) {
        err = hipMemcpyAsync(vis_d + r.first * row_b, vis_h + r.first * row_b,
                             static_cast<size_t>(r.second - r.first) * row_b,
                             h2d, s_in.s);
        if (err != hipSuccess) break;
      }
    } else {
      const size_t off = static_cast<size_t>(sb[i]) * sg_b;
      err = hipMemcpyAsync(sg_d + off, sg_h + off,
                           static_cast<size_t>(sb[i + 1] - sb[i]) * sg_b, h2d,
                           s_in.s);
    }
    if (err == hipSuccess) err = hipEventRecord(e_in[i].e, s_in.s);
    if (err == hipSuccess) err = hipStreamWaitEvent(s_k.s, e_in[i].e, 0);
    if (err == hipSuccess) {
      // the chunk's metadata starts at sb[i]: the kernels rebase rows on its
      // first entry, so the row pointers move by that entry's rebase delta
      Problem pc = p;
      pc.nr_subgrids = sb[i + 1] - sb[i];
      const long long delta = static_cast<long long>(metadata[sb[i]].baseline_offset) -
                              metadata[0].baseline_offset;
      err = launch(dir, pc,
                   static_cast<char *>(d_uvw.ptr) + delta * 3 * sizeof(float),
                   static_cast<const float *>(d_wn.ptr), vis_d + delta * row_b,
                   static_cast<const float *>(d_sph.ptr), d_at.ptr,
                   static_cast<const idg::Metadata *>(d_md.ptr) + sb[i],
                   sg_d + static_cast<size_t>(sb[i]) * sg_b, s_k.s, force,
                   opt);
    }
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipEventRecord(e_k[i].e, s_k.s);
    if (err == hipSuccess) launched.store(i + 1, std::memory_order_release);
  }
  if (err != hipSuccess) abort_out.store(true, std::memory_order_release);
  out.join();
  if (err == hipSuccess) err = out_err;
  const hipError_t sync = hipDeviceSynchronize();
  return err != hipSuccess ? err : sync;
}

double run_performance(Direction dir, const void *func, std::string name,
                       int num_threads) {
  const int nr_correlations =
      static_cast<int>(get_env_var("NR_CORRELATIONS", 4));
  const int grid_size = static_cast<int>(get_env_var("GRID_SIZE", 1024));
  const int subgrid_size = static_cast<int>(get_env_var("SUBGRID_SIZE", 32));
  const int nr_stations = static_cast<int>(get_env_var("NR_STATIONS", 50));
  const int nr_timeslots = static_cast<int>(get_env_var("NR_TIMESLOTS", 20));
  const int nr_timesteps =
      static_cast<int>(get_env_var("NR_TIMESTEPS_SUBGRID", 128));
  const int nr_channels = static_cast<int>(get_env_var("NR_CHANNELS", 16));
  const int nr_baselines = nr_stations * (nr_stations - 1) / 2;
  const int nr_subgrids = nr_baselines * nr_timeslots;
  const size_t rows = static_cast<size_t>(nr_subgrids) * nr_timesteps;
  if (nr_correlations != 4)
    std::cerr << "idg-mi355x: kernels compute 4 correlations; "
                 "NR_CORRELATIONS only affects the work model\n";
  print_parameters(nr_stations, nr_channels, nr_timesteps, nr_correlations,
                   nr_timeslots, IMAGE_SIZE, grid_size, subgrid_size, W_STEP,
                   nr_baselines, nr_subgrids, static_cast<int>(rows));
  const double gflops =
      1e-9 * flops_gridder(nr_channels, rows, nr_subgrids, subgrid_size,
                           nr_correlations);
  const double gbytes =
      1e-9 * bytes_gridder(nr_channels, rows, nr_subgrids, subgrid_size,
                           nr_correlations);
  const double mvis = 1e-6 * rows * nr_channels;

  // Real synthetic inputs (documented deviation from the reference, which
  // uploads only the metadata).
  srand(0);
  idg::Array2D<idg::UVWCoordinate<float>> uvw(nr_subgrids, nr_timesteps);
  idg::Array1D<float> freq(nr_channels), wn(nr_channels);
  idg::Array1D<idg::Baseline> baselines(nr_baselines);
  idg::Array2D<float> sph(subgrid_size, subgrid_size);
  idg::Array4D<idg::Matrix2x2<std::complex<float>>> aterms(
      nr_timeslots, nr_stations, subgrid_size, subgrid_size);
  idg::Array1D<idg::Metadata> md(nr_subgrids);
  initialize_uvw(grid_size, uvw);
  initialize_frequencies(freq);
  initialize_wavenumbers(freq, wn);
  initialize_baselines(nr_stations, baselines);
  initialize_spheroidal(sph);
  initialize_aterms(sph, aterms);
  initialize_metadata(grid_size, nr_timeslots, nr_timesteps, baselines, md);
  idg::Array3D<idg::Visibility<std::complex<float>>> vis(nr_subgrids,
                                                         nr_timesteps,
                                                         nr_channels);
  idg::Array4D<std::complex<float>> subgrids(nr_subgrids, 4, subgrid_size,
                                             subgrid_size);
  if (dir == Direction::kGridder)
    initialize_visibilities(grid_size, IMAGE_SIZE, freq, uvw, vis);
  else
    initialize_subgrids(subgrids);

  Problem p{nr_subgrids, grid_size, subgrid_size, IMAGE_SIZE,
            static_cast<float>(W_STEP), nr_channels, nr_stations};
  Extents e{rows, static_cast<size_t>(nr_timeslots)};
  const std::string bad = validate(p, e, md.data());
  if (!bad.empty()) {
    std::cerr << "idg-mi355x: " << bad << std::endl;
    std::exit(EXIT_FAILURE);
  }
  void *d_uvw, *d_wn, *d_vis, *d_sph, *d_at, *d_md, *d_sg;
  hipCheck(hipMalloc(&d_uvw, uvw.bytes()));
  hipCheck(hipMalloc(&d_wn, wn.bytes()));
  hipCheck(hipMalloc(&d_vis, vis.bytes()));
  hipCheck(hipMalloc(&d_sph, sph.bytes()));
  hipCheck(hipMalloc(&d_at, aterms.bytes()));
  hipCheck(hipMalloc(&d_md, md.bytes()));
  hipCheck(hipMalloc(&d_sg, subgrids.bytes()));
  hipCheck(hipMemcpy(d_uvw, uvw.data(), uvw.bytes(), hipMemcpyHostToDevice));
  hipCheck(hipMemcpy(d_wn, wn.data(), wn.bytes(), hipMemcpyHostToDevice));
  hipCheck(hipMemcpy(d_vis, vis.data(), vis.bytes(), hipMemcpyHostToDevice));
  hipCheck(hipMemcpy(d_sph, sph.data(), sph.bytes(), hipMemcpyHostToDevice));
  hipCheck(hipMemcpy(d_at, aterms.data(), aterms.bytes(),
                     hipMemcpyHostToDevice));
  hipCheck(hipMemcpy(d_md, md.data(), md.bytes(), hipMemcpyHostToDevice));
  hipCheck(hipMemcpy(d_sg, subgrids.data(), subgrids.bytes(),
                     hipMemcpyHostToDevice));
  int a_grid = grid_size, a_sub = subgrid_size, a_nc = nr_channels,
      a_ns = nr_stations;
  float a_img = IMAGE_SIZE, a_w = W_STEP;
  void *args[] = {&a_grid, &a_sub, &a_img, &a_w,   &a_nc,  &a_ns, &d_uvw,
                  &d_wn,   &d_vis, &d_sph, &d_at,  &d_md,  &d_sg};
  // The selected MI355X kernel is timed as the device entries launch it
  // (its two-launch form, when it has one); a caller-supplied kernel as
  // itself.
  const KernelChoice k = dir == Direction::kGridder ? select_gridder(p)
                                                    : select_degridder(p);
  double seconds;
  if (func == k.func && k.auto_ordered) {
    // the auto gridder (IDG_GRIDDER_IMPL=auto) is its launch sequence
    seconds = hip::time_iterations(
        [&] {
          hipCheck(launch(dir, p, d_uvw, static_cast<const float *>(d_wn),
                          d_vis, static_cast<const float *>(d_sph), d_at, d_md,
                          d_sg, nullptr));
        },
        name, gflops, gbytes, mvis);
  } else if (func == k.func && k.parts[1].func) {
    seconds = hip::time_launches(k, dim3(nr_subgrids), args, name, gflops,
                                 gbytes, mvis);
  } else {
    seconds = hip::p_run_kernel(func, dim3(nr_subgrids), dim3(num_threads),
                                args, name, gflops, gbytes, mvis);
  }
  for (void *ptr : {d_uvw, d_wn, d_vis, d_sph, d_at, d_md, d_sg})
    hipCheck(hipFree(ptr));
  return seconds;
}

}  // namespace idg_mi355x
