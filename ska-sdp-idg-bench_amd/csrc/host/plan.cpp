// plan.cpp -- the host twin of the plan step (host.hpp).
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

#include "host/host.hpp"

namespace idg_mi355x {
namespace host {

void plan(plan::Geometry g, float image_size, float inv_w_step,
          int nr_baselines, int nr_timesteps, int nr_channels,
          const uint32_t *baselines, const UVW *uvw, const float *wavenumbers,
          idg::Metadata *metadata, int capacity, int32_t counts[2],
          int nthreads) {
  plan::set_scales(&g, image_size, wavenumbers[0],
                   wavenumbers[nr_channels - 1], inv_w_step);
  const int B = nr_baselines, T = nr_timesteps;
  const float *rows = reinterpret_cast<const float *>(uvw);
  int32_t *out = reinterpret_cast<int32_t *>(metadata);
  // count, prefix, fill: each pass splits the baselines over the threads
  std::vector<int> count(B), dropped(B);
  std::vector<long long> offset(B + 1, 0);
  const auto pass = [&](bool fill) {
    const int nt = std::max(1, std::min(nthreads, B));
    const auto range = [&](int b0, int b1) {
      for (int bl = b0; bl < b1; ++bl) {
        const int row0 = bl * T;
        int n = 0;
        const long long first = offset[bl];
        const int d = plan::walk_baseline(
            g, rows + static_cast<size_t>(row0) * 3, row0, T,
            baselines[2 * bl], baselines[2 * bl + 1],
            [&](const int32_t words[9]) {
              if (fill && first + n < capacity)
                std::memcpy(out + (first + n) * 9, words, 9 * sizeof(int32_t));
              ++n;
            });
        if (!fill) {
          count[bl] = n;
          dropped[bl] = d;
        }
      }
    };
    if (nt == 1) return range(0, B);
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; ++w) {
      const int b0 = static_cast<int>(static_cast<long long>(B) * w / nt);
      const int b1 = static_cast<int>(static_cast<long long>(B) * (w + 1) / nt);
      if (b1 > b0) pool.emplace_back(range, b0, b1);
    }
    for (auto &th : pool) th.join();
  };
  pass(false);
  long long lost = 0;
  for (int bl = 0; bl < B; ++bl) {
    offset[bl + 1] = offset[bl] + count[bl];
    lost += dropped[bl];
  }
  counts[0] = static_cast<int32_t>(offset[B]);
  counts[1] = static_cast<int32_t>(lost);
  if (capacity > 0 && offset[B] > 0) pass(true);
}

}  // namespace host
}  // namespace idg_mi355x
