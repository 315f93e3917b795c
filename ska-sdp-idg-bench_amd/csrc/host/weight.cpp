// weight.cpp -- the host twins of the imaging-weight steps (host.hpp).
#include <cstring>
#include <vector>

#include "host/host.hpp"
#include "idg_mi355x.h"

namespace idg_mi355x {
namespace host {

namespace {

namespace wt = idg_mi355x::weight;

// Row of timestep 0 of subgrid s (include/idg_mi355x.h).
long long weight_row0(const idg::Metadata *md, int s) {
  return (static_cast<long long>(md[s].baseline_offset) -
          md[0].baseline_offset) +
         md[s].time_offset;
}

// Every record's rows inside [0, uvw_rows).
Status check_weight_rows(int nr_subgrids, size_t uvw_rows,
                         const idg::Metadata *md) {
  for (int s = 0; s < nr_subgrids; ++s) {
    const long long t0 = weight_row0(md, s);
    if (md[s].nr_timesteps < 0 || t0 < 0 ||
        t0 + md[s].nr_timesteps > static_cast<long long>(uvw_rows))
      return {IDG_E_OUT_OF_BOUNDS,
              "subgrid " + std::to_string(s) + ": timesteps [" +
                  std::to_string(t0) + ", " +
                  std::to_string(t0 + md[s].nr_timesteps) +
                  ") outside uvw/weight rows [0, " +
                  std::to_string(uvw_rows) + ")"};
  }
  return {};
}

Status check_density_cells(const wt::Geometry &g, const uint64_t *density) {
  const size_t cells = static_cast<size_t>(g.grid_size) * g.grid_size;
  for (size_t i = 0; i < cells; ++i)
    if (density[i] >= wt::kCellLimit)
      return {IDG_E_INVALID_ARGUMENT, "weight: density cell " +
                                          std::to_string(i) +
                                          " is at or above 2^62"};
  return {};
}

}  // namespace

Status weight_density(const wt::Geometry &g, int nr_subgrids, int nr_channels,
                      const idg::Metadata *metadata, const UVW *uvw,
                      size_t uvw_rows, const float *wavenumbers,
                      const float *weights, uint64_t *density) {
  if (Status st = check_weight_rows(nr_subgrids, uvw_rows, metadata); st.code)
    return st;
  if (Status st = check_density_cells(g, density); st.code) return st;
  const size_t G = static_cast<size_t>(g.grid_size), C = nr_channels;
  // summed on a copy, so that a failure leaves the caller's density alone
  std::vector<uint64_t> sum(density, density + G * G);
  for (int s = 0; s < nr_subgrids; ++s) {
    const size_t row0 = static_cast<size_t>(weight_row0(metadata, s));
    for (int t = 0; t < metadata[s].nr_timesteps; ++t) {
      const size_t row = row0 + t;
      for (size_t c = 0; c < C; ++c) {
        int x, y;
        const uint64_t q = wt::sample(g, uvw[row].u, uvw[row].v,
                                      wavenumbers[c], weights[row * C + c],
                                      &x, &y);
        if (q == 0) continue;
        uint64_t &cell = sum[static_cast<size_t>(y) * G + x];
        cell += q;
        if (cell >= wt::kCellLimit)
          return {IDG_E_INVALID_ARGUMENT,
                  "idg_weight_density: the sum of cell (" +
                      std::to_string(x) + ", " + std::to_string(y) +
                      ") reaches 2^62"};
      }
    }
  }
  std::memcpy(density, sum.data(), G * G * sizeof(uint64_t));
  return {};
}

Status weight_scheme(const wt::Geometry &g, int scheme, double briggs_scale,
                     const uint64_t *density, float ab[2]) {
  if (Status st = check_density_cells(g, density); st.code) return st;
  double sum_d = 0.0, sum_d2 = 0.0;
  if (scheme == wt::kBriggs) {
    const int G = g.grid_size;
    for (int y = 0; y < G; ++y)
      for (int x = 0; x < G; ++x) {
        const double D =
            wt::density_of(wt::count_at(g, density, x, y), g.quantum_log2);
        sum_d += D;
        sum_d2 += D * D;
      }
  }
  wt::scheme_ab(scheme, briggs_scale, sum_d, sum_d2, &ab[0], &ab[1]);
  return {};
}

Status weight_apply(const wt::Geometry &g, int nr_subgrids, int nr_channels,
                    const idg::Metadata *metadata, const UVW *uvw,
                    size_t uvw_rows, const float *wavenumbers,
                    const float *weights, const uint64_t *density,
                    const float ab[2],
                    const std::complex<float> *visibilities,
                    float *imaging_weights, std::complex<float> *out,
                    double *sum_weights) {
  using cfloat = std::complex<float>;
  if (Status st = check_weight_rows(nr_subgrids, uvw_rows, metadata); st.code)
    return st;
  if (Status st = check_density_cells(g, density); st.code) return st;
  const size_t C = nr_channels;
  const float a = ab[0], b = ab[1];
  double sum = 0.0;
  for (int s = 0; s < nr_subgrids; ++s) {
    const size_t row0 = static_cast<size_t>(weight_row0(metadata, s));
    for (int t = 0; t < metadata[s].nr_timesteps; ++t) {
      const size_t row = row0 + t;
      for (size_t c = 0; c < C; ++c) {
        const size_t at = row * C + c;
        const float w = weights[at];
        int x, y;
        const bool live = wt::sample(g, uvw[row].u, uvw[row].v,
                                     wavenumbers[c], w, &x, &y) != 0;
        const float f =
            live ? wt::imaging_weight(
                       w, a, b,
                       wt::density_of(wt::count_at(g, density, x, y),
                                      g.quantum_log2))
                 : 0.0f;
        cfloat *o = out + at * 4;
        if (visibilities == nullptr) {
          o[0] = o[3] = cfloat(f, 0.0f);
          o[1] = o[2] = cfloat(0.0f, 0.0f);
        } else if (live) {
          const cfloat *v = visibilities + at * 4;
          for (int p = 0; p < 4; ++p)
            o[p] = cfloat(f * v[p].real(), f * v[p].imag());
        } else {
          for (int p = 0; p < 4; ++p) o[p] = cfloat(0.0f, 0.0f);
        }
        imaging_weights[at] = f;
        sum += f;
      }
    }
  }
  *sum_weights = sum;
  return {};
}

}  // namespace host
}  // namespace idg_mi355x
