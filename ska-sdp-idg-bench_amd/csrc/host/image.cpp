// image.cpp -- the taper on the image's pixels (host.hpp).
#include <cmath>
#include <vector>

#include "host/host.hpp"

namespace idg_mi355x {
namespace host {

void taper_to_image(int subgrid_size, int grid_size, const float *spheroidal,
                    double *out) {
  const int S = subgrid_size, G = grid_size;
  // d[j][p]: the periodic interpolation kernel from sample p, at (p + 0.5 -
  // S/2) subgrid pixels, to image pixel j, at (j - G/2) S / G of them;
  // frequencies |k| < S/2 whole, the Nyquist pair (even S) as one cosine
  const double two_pi = 6.283185307179586476925287;
  std::vector<double> d(static_cast<size_t>(G) * S);
  for (int j = 0; j < G; ++j)
    for (int p = 0; p < S; ++p) {
      const double delta = static_cast<double>(j - G / 2) * S / G -
                           (static_cast<double>(p) + 0.5 - S / 2);
      double sum = 1.0;
      for (int k = 1; 2 * k < S; ++k)
        sum += 2.0 * std::cos(two_pi * k * delta / S);
      if (S % 2 == 0) sum += std::cos(0.5 * two_pi * delta);
      d[static_cast<size_t>(j) * S + p] = sum / S;
    }
  // out = d taper d^T, the x sum first
  std::vector<double> rows(static_cast<size_t>(S) * G);
  for (int py = 0; py < S; ++py)
    for (int j = 0; j < G; ++j) {
      double sum = 0.0;
      for (int px = 0; px < S; ++px)
        sum += static_cast<double>(spheroidal[py * S + px]) *
               d[static_cast<size_t>(j) * S + px];
      rows[static_cast<size_t>(py) * G + j] = sum;
    }
  for (int i = 0; i < G; ++i)
    for (int j = 0; j < G; ++j) {
      double sum = 0.0;
      for (int py = 0; py < S; ++py)
        sum += d[static_cast<size_t>(i) * S + py] *
               rows[static_cast<size_t>(py) * G + j];
      out[static_cast<size_t>(i) * G + j] = sum;
    }
}

}  // namespace host
}  // namespace idg_mi355x
