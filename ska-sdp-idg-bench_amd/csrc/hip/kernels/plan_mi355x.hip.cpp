// plan_mi355x.hip.cpp -- the plan step on the device: uvw rows
// in HBM -> subgrid metadata in HBM, bit for bit what idg_plan computes on
// the host (common/plan.hpp holds the arithmetic of both).  Three launches
// ordered by their kernel boundaries, no cross-workgroup wait, no atomics:
//   walk<count>  one wave64 per baseline: subgrids and dropped rows of it
//   scan         one workgroup: exclusive scan of the counts -> offsets,
//                counts[0] = subgrids needed, counts[1] = dropped timesteps
//   walk<fill>   the same walk, writing record i of baseline bl at
//                offsets[bl] + i while that is below `capacity`
// Workspace (util.hpp kWorkspacePlan), in ints: [0, B) counts, [B, 2B)
// dropped, [2B, 3B) offsets.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common/plan.hpp"
#include "hip/util.hpp"

namespace idg_mi355x {

namespace {

constexpr int kWave = 64;
constexpr int kWalkBlock = 256;  // 4 baselines per workgroup
constexpr int kScanBlock = 1024;

__device__ inline int prefix_min(int v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d *= 2) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v = o < v ? o : v;
  }
  return v;
}

__device__ inline int prefix_max(int v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d *= 2) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v = o > v ? o : v;
  }
  return v;
}

__device__ inline plan::Box box_of_lane(const plan::Box &b, int lane) {
  return plan::Box{__shfl(b.x0, lane), __shfl(b.x1, lane), __shfl(b.y0, lane),
                   __shfl(b.y1, lane)};
}

// One wave per baseline.  The lanes hold the next 64 candidate timesteps
// from `pos` on; an inclusive prefix min / max of their boxes, merged with
// the box carried from the blocks before, is the box the open subgrid would
// have if it ran through each lane; the first failing lane closes it.
// Everything but the per-lane evaluation is wave-uniform.
template <bool FILL>
__global__ void __launch_bounds__(kWalkBlock)
    kernel_plan_walk_mi355x(plan::Geometry g, float image_size,
                            float inv_w_step, int nr_baselines,
                            int nr_timesteps, int nr_channels,
                            const uint32_t *__restrict__ baselines,
                            const float *__restrict__ uvw,
                            const float *__restrict__ wavenumbers,
                            int *__restrict__ ws, int32_t *__restrict__ metadata,
                            int capacity) {
  const int lane = threadIdx.x & (kWave - 1);
  const int bl = blockIdx.x * (kWalkBlock / kWave) + (threadIdx.x / kWave);
  if (bl >= nr_baselines) return;
  plan::set_scales(&g, image_size, wavenumbers[0],
                   wavenumbers[nr_channels - 1], inv_w_step);
  const int T = nr_timesteps;
  const int row0 = bl * T;  // < 2^31 (checked by the entry)
  const float *rows = uvw + static_cast<size_t>(row0) * 3;
  const uint32_t station1 = baselines[2 * bl], station2 = baselines[2 * bl + 1];
  const int first_record = FILL ? ws[2 * nr_baselines + bl] : 0;

  int pos = 0, n = 0, t0 = 0, slot0 = 0, layer0 = 0, count = 0, dropped = 0;
  bool open = false;
  plan::Box carry = plan::empty_box();

  const auto close = [&]() {
    if (FILL) {
      const long long at = static_cast<long long>(first_record) + count;
      if (at < capacity) {
        int32_t words[9];
        plan::record_words(g, row0 + t0, n, slot0, layer0, station1, station2,
                           carry, words);
        int32_t mine = words[0];
#pragma unroll
        for (int i = 1; i < 9; ++i) mine = lane == i ? words[i] : mine;
        if (lane < 9) metadata[at * 9 + lane] = mine;
      }
    }
    ++count;
    open = false;
  };

  while (pos < T) {
    const int t = pos + lane;
    const bool in = t < T;
    plan::Step s;
    s.box = plan::empty_box();
    s.layer = 0;
    s.valid = false;
    if (in) {
      const float *r = rows + static_cast<size_t>(t) * 3;
      s = plan::eval_step(g, r[0], r[1], r[2]);
    }
    const int slot = plan::slot_of(g, in ? t : 0);
    if (!open) {
      // a run of leading invalid rows is dropped in one step
      const unsigned long long bad = __ballot(in && !s.valid);
      if (bad & 1ull) {
        const int run = ~bad ? __builtin_ctzll(~bad) : kWave;
        dropped += run;
        pos += run;
        continue;
      }
      open = true;
      t0 = pos;
      slot0 = __shfl(slot, 0);
      layer0 = __shfl(s.layer, 0);
      n = 0;
      carry = plan::empty_box();
    }
    // (an invalid lane's box is empty; it fails below, and nothing after the
    // first failing lane is used)
    plan::Box m;
    m.x0 = prefix_min(s.box.x0, lane);
    m.x1 = prefix_max(s.box.x1, lane);
    m.y0 = prefix_min(s.box.y0, lane);
    m.y1 = prefix_max(s.box.y1, lane);
    m = plan::merge(carry, m);
    int x, y;
    const bool ok = in && s.valid && slot == slot0 && s.layer == layer0 &&
                    lane < g.max_timesteps - n && plan::place(g, m, &x, &y);
    const unsigned long long fail = __ballot(!ok);
    if (fail == 0) {  // all 64 join: the box is carried into the next block
      carry = box_of_lane(m, kWave - 1);
      n += kWave;
      pos += kWave;
      continue;
    }
    const int first = __builtin_ctzll(fail);
    if (first > 0) carry = box_of_lane(m, first - 1);
    n += first;
    pos += first;  // the failing lane is lane 0 of the next block
    close();
  }
  if (open) close();
  if (!FILL && lane == 0) {
    ws[bl] = count;
    ws[nr_baselines + bl] = dropped;
  }
}

// One workgroup: exclusive scan of the B counts in chunks of kScanBlock
// (wave scans joined through LDS, a running carry between chunks), the sum
// of the dropped rows, and the two totals.  Integer sums: any order gives
// the same bits.
__global__ void __launch_bounds__(kScanBlock)
    kernel_plan_scan_mi355x(int nr_baselines, int *__restrict__ ws,
                            int32_t *__restrict__ counts) {
  constexpr int kWaves = kScanBlock / kWave;
  __shared__ int wave_sum[kWaves];
  __shared__ int drop_sum[kWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int *cnt = ws, *drop = ws + nr_baselines;
  int *off = ws + 2 * static_cast<size_t>(nr_baselines);
  int carry = 0, dropped = 0;
  for (int base = 0; base < nr_baselines; base += kScanBlock) {
    const int i = base + tid;
    const int c = i < nr_baselines ? cnt[i] : 0;
    dropped += i < nr_baselines ? drop[i] : 0;
    int incl = c;
#pragma unroll
    for (int d = 1; d < kWave; d *= 2) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int v = wave_sum[w];
      before += w < wave ? v : 0;
      total += v;
    }
    if (i < nr_baselines) off[i] = carry + before + incl - c;
    carry += total;
    __syncthreads();
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d /= 2) dropped += __shfl_down(dropped, d);
  if (lane == 0) drop_sum[wave] = dropped;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < kWaves; ++w) total += drop_sum[w];
    counts[0] = carry;
    counts[1] = total;
  }
}

}  // namespace

size_t plan_workspace_bytes(int nr_baselines) {
  return 3 * static_cast<size_t>(nr_baselines) * sizeof(int);
}

hipError_t launch_plan(const plan::Geometry &geometry, float image_size,
                       float inv_w_step, int nr_baselines, int nr_timesteps,
                       int nr_channels, const void *d_baselines,
                       const void *d_uvw, const float *d_wavenumbers,
                       void *d_metadata, int capacity, void *d_counts,
                       hipStream_t stream) {
  WorkspaceLease lease;
  hipError_t err = lease.acquire(stream, kWorkspacePlan,
                                 plan_workspace_bytes(nr_baselines));
  if (err != hipSuccess) return err;
  plan::Geometry g = geometry;
  void *ws = lease.ptr;
  void *args[] = {&g,           &image_size,   &inv_w_step, &nr_baselines,
                  &nr_timesteps, &nr_channels, &d_baselines, &d_uvw,
                  &d_wavenumbers, &ws,         &d_metadata, &capacity};
  const int per_block = kWalkBlock / kWave;
  const dim3 grid((nr_baselines + per_block - 1) / per_block);
  err = hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_plan_walk_mi355x<false>), grid,
      dim3(kWalkBlock), args, 0, stream);
  if (err != hipSuccess) return err;
  void *scan_args[] = {&nr_baselines, &ws, &d_counts};
  err = hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_plan_scan_mi355x), dim3(1),
      dim3(kScanBlock), scan_args, 0, stream);
  if (err != hipSuccess || capacity <= 0) return err;
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_plan_walk_mi355x<true>), grid,
      dim3(kWalkBlock), args, 0, stream);
}

}  // namespace idg_mi355x
