// multiscale.cpp -- the host twins of multi-scale CLEAN (host.hpp): the scale
// taps, the dense separable convolution, the prepare step and the minor cycle
// (the one of host/minor_cycle.hpp under ms::Cycle).
#include <algorithm>
#include <vector>

#include "host/host.hpp"
#include "host/minor_cycle.hpp"

namespace idg_mi355x {
namespace host {

namespace {

double scale_sigma(double scale) { return scale * 3.0 / 16.0; }

}  // namespace

int ms_scale_radius(double scale) {
  if (!(scale >= 0.0)) return -1;
  if (scale == 0.0) return 0;
  const double r = std::ceil(3.0 * scale_sigma(scale));
  return r <= ms::kMaxRadius ? static_cast<int>(r) : -1;
}

void ms_scale_taps(double scale, int radius, float *taps) {
  if (scale == 0.0) {
    taps[0] = 1.0f;
    return;
  }
  const double sigma = scale_sigma(scale);
  const double d = 2.0 * sigma * sigma;
  double sum = 0.0;
  for (int j = -radius; j <= radius; ++j)
    sum += std::exp(-static_cast<double>(j * j) / d);
  for (int k = -radius; k <= radius; ++k)
    taps[k + radius] =
        static_cast<float>(std::exp(-static_cast<double>(k * k) / d) / sum);
}

void convolve_separable(int grid_size, int radius, const float *in,
                        const float *taps, float *tmp, float *out) {
  const int G = grid_size, r = radius;
  for (int y = 0; y < G; ++y) {
    const float *row = in + static_cast<size_t>(y) * G;
    float *trow = tmp + static_cast<size_t>(y) * G;
    for (int x = 0; x < G; ++x) {
      float acc = 0.0f;
      const int k0 = std::max(-r, -x), k1 = std::min(r, G - 1 - x);
      for (int k = k0; k <= k1; ++k) acc = ms::tap(row[x + k], taps[k + r], acc);
      trow[x] = acc;
    }
  }
  for (int y = 0; y < G; ++y) {
    float *orow = out + static_cast<size_t>(y) * G;
    const int k0 = std::max(-r, -y), k1 = std::min(r, G - 1 - y);
    for (int x = 0; x < G; ++x) {
      float acc = 0.0f;
      for (int k = k0; k <= k1; ++k)
        acc = ms::tap(tmp[static_cast<size_t>(y + k) * G + x], taps[k + r], acc);
      orow[x] = acc;
    }
  }
}

void ms_prepare(const ms::Params &p, const float *residual, const float *psf,
                const float *taps, float *planes, float *cross_psf,
                float *tmp) {
  const int G = p.base.grid_size, Gp = p.base.psf_size, Ns = p.nr_scales;
  const size_t cells = static_cast<size_t>(G) * G;
  const size_t pcells = static_cast<size_t>(Gp) * Gp;
  if (planes != residual) std::copy(residual, residual + cells, planes);
  for (int s = 1; s < Ns; ++s)
    convolve_separable(G, p.radius[s], residual, taps + ms::taps_at(p, s), tmp,
                       planes + s * cells);
  // cross(s, s)'s patch holds convolve(psf, h_s) until every cross(s, q > s) is
  // made from it, then takes its own second convolution in place
  for (int s = 0; s < Ns; ++s) {
    const float *hs = taps + ms::taps_at(p, s);
    float *first = cross_psf + ms::cross_at(Ns, s, s) * pcells;
    convolve_separable(Gp, p.radius[s], psf, hs, tmp, first);
    for (int q = s + 1; q < Ns; ++q)
      convolve_separable(Gp, p.radius[q], first, taps + ms::taps_at(p, q), tmp,
                         cross_psf + ms::cross_at(Ns, s, q) * pcells);
    convolve_separable(Gp, p.radius[s], first, hs, tmp, first);
  }
}

std::string ms_clean(const ms::Params &p, float *planes,
                     const float *cross_psf, const float *taps,
                     const uint8_t *mask, float *model,
                     ms::Component *components, ms::State *state) {
  const int G = p.base.grid_size;
  // step 7: the component's footprint, clipped at the image's edge
  return minor_cycle<ms::Cycle>(
      "idg_ms_clean", p, planes, cross_psf, mask, components, state,
      [&](float c, int s, uint32_t, int py, int px) {
        const int r = p.radius[s];
        const float *h = taps + ms::taps_at(p, s);
        for (int y = std::max(py - r, 0); y <= std::min(py + r, G - 1); ++y)
          for (int x = std::max(px - r, 0); x <= std::min(px + r, G - 1); ++x) {
            float *m = model + static_cast<size_t>(y) * G + x;
            *m = ms::model_add(c, h[y - py + r], h[x - px + r], *m);
          }
      });
}

}  // namespace host
}  // namespace idg_mi355x
