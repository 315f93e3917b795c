// restore.cpp -- the clean beam (fit, axes, radius, taps) and the host twin of
// the restore step (host.hpp).
#include "host/host.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace idg_mi355x {
namespace host {

namespace {

namespace rs = idg_mi355x::restore;

constexpr int kFitReach = 32;  // the fit's window: |dy|, |dx| <= 32
constexpr double kPi = 3.14159265358979323846;

// major, minor, pa of a beam whose a, b, c are a positive definite form.
void axes_of(Beam *beam) {
  const double mean = 0.5 * (beam->a + beam->c);
  const double half = 0.5 * (beam->a - beam->c);
  const double root = std::sqrt(half * half + beam->b * beam->b);
  const double ln2 = std::log(2.0);
  beam->major = 2.0 * std::sqrt(ln2 / (mean - root));
  beam->minor = 2.0 * std::sqrt(ln2 / (mean + root));
  // the major axis is the eigen-direction of the smaller eigenvalue
  double pa = 0.5 * std::atan2(beam->b == 0.0 ? 0.0 : -2.0 * beam->b,
                               beam->c - beam->a);
  if (pa <= -0.5 * kPi) pa += kPi;
  beam->pa = pa;
}

}  // namespace

bool beam_ok(const Beam &beam) {
  return std::isfinite(beam.a) && std::isfinite(beam.b) &&
         std::isfinite(beam.c) && beam.a > 0.0 && beam.c > 0.0 &&
         beam.a * beam.c - beam.b * beam.b > 0.0;
}

std::string beam_from_axes(double major, double minor, double pa, Beam *out) {
  if (!std::isfinite(major) || !std::isfinite(minor) || !std::isfinite(pa) ||
      !(minor > 0.0) || !(major >= minor))
    return "idg_beam_from_axes: major >= minor > 0 and a finite pa required";
  pa -= kPi * std::ceil((pa - 0.5 * kPi) / kPi);  // into (-pi/2, pi/2]
  const double ln2 = std::log(2.0);
  const double lmaj = 4.0 * ln2 / (major * major);
  const double lmin = 4.0 * ln2 / (minor * minor);
  const double cs = std::cos(pa), sn = std::sin(pa);
  Beam beam;
  beam.a = lmaj * cs * cs + lmin * sn * sn;
  beam.b = (lmaj - lmin) * sn * cs;
  beam.c = lmaj * sn * sn + lmin * cs * cs;
  beam.major = major;
  beam.minor = minor;
  beam.pa = pa;
  if (!beam_ok(beam))
    return "idg_beam_from_axes: the axes give no positive definite beam";
  *out = beam;
  return {};
}

std::string beam_fit(int psf_size, const float *psf, float level, Beam *out) {
  const int Gp = psf_size, centre = Gp / 2;
  const size_t stride = static_cast<size_t>(Gp);
  const double p0 = static_cast<double>(psf[centre * stride + centre]);
  if (!std::isfinite(p0) || !(p0 > 0.0))
    return "idg_beam_fit: the psf's centre is not finite and positive";

  // the region: q >= level, 4-connected to the centre, inside the window
  constexpr int kSide = 2 * kFitReach + 1;
  std::vector<uint8_t> in(kSide * kSide, 0);
  std::vector<int> todo;
  const auto at = [](int dy, int dx) {
    return (dy + kFitReach) * kSide + dx + kFitReach;
  };
  const auto q_of = [&](int dy, int dx) {
    return static_cast<double>(
               psf[static_cast<size_t>(centre + dy) * stride + centre + dx]) /
           p0;
  };
  in[at(0, 0)] = 1;
  todo.push_back(at(0, 0));
  bool at_edge = false;
  while (!todo.empty()) {
    const int cell = todo.back();
    todo.pop_back();
    const int dy = cell / kSide - kFitReach, dx = cell % kSide - kFitReach;
    if (std::abs(dy) == kFitReach || std::abs(dx) == kFitReach) at_edge = true;
    const int next[4][2] = {{dy - 1, dx}, {dy + 1, dx}, {dy, dx - 1},
                            {dy, dx + 1}};
    for (const auto &n : next) {
      const int ny = n[0], nx = n[1];
      if (std::abs(ny) > kFitReach || std::abs(nx) > kFitReach) continue;
      if (centre + ny < 0 || centre + ny >= Gp || centre + nx < 0 ||
          centre + nx >= Gp)
        continue;
      if (in[at(ny, nx)] || !(q_of(ny, nx) >= static_cast<double>(level)))
        continue;
      in[at(ny, nx)] = 1;
      todo.push_back(at(ny, nx));
    }
  }
  if (at_edge)
    return "idg_beam_fit: the main lobe reaches the edge of the +-32 pixel "
           "window (lobe too wide)";

  // normal equations of min sum w (a X + b2 Y + c Z + ln q)^2, w = q^2,
  // X = dx^2, Y = dx dy, Z = dy^2, over the region in row-major order
  double m[3][4] = {{0.0}};
  int pixels = 0;
  for (int dy = -kFitReach; dy <= kFitReach; ++dy)
    for (int dx = -kFitReach; dx <= kFitReach; ++dx) {
      if (!in[at(dy, dx)] || (dy == 0 && dx == 0)) continue;
      ++pixels;
      const double q = q_of(dy, dx);
      const double w = q * q, l = std::log(q);
      const double v[3] = {static_cast<double>(dx) * dx,
                           static_cast<double>(dx) * dy,
                           static_cast<double>(dy) * dy};
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) m[i][j] += w * v[i] * v[j];
        m[i][3] -= w * l * v[i];
      }
    }
  if (pixels < 3)
    return "idg_beam_fit: fewer than three pixels besides the centre reach "
           "the level (" + std::to_string(pixels) + ")";

  // elimination with row pivoting
  for (int k = 0; k < 3; ++k) {
    int pivot = k;
    for (int i = k + 1; i < 3; ++i)
      if (std::fabs(m[i][k]) > std::fabs(m[pivot][k])) pivot = i;
    if (pivot != k)
      for (int j = 0; j < 4; ++j) std::swap(m[k][j], m[pivot][j]);
    if (!std::isfinite(m[k][k]) || m[k][k] == 0.0)
      return "idg_beam_fit: the fit's system is singular or not finite";
    for (int i = k + 1; i < 3; ++i) {
      const double f = m[i][k] / m[k][k];
      for (int j = k; j < 4; ++j) m[i][j] -= f * m[k][j];
    }
  }
  double x[3];
  for (int k = 2; k >= 0; --k) {
    double s = m[k][3];
    for (int j = k + 1; j < 3; ++j) s -= m[k][j] * x[j];
    x[k] = s / m[k][k];
  }
  if (!std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2]))
    return "idg_beam_fit: the fit's system is singular or not finite";
  Beam beam;
  beam.a = x[0];
  beam.b = 0.5 * x[1];
  beam.c = x[2];
  if (!beam_ok(beam))
    return "idg_beam_fit: the fitted form is not positive definite (a <= 0, "
           "c <= 0 or a c - b^2 <= 0)";
  axes_of(&beam);
  *out = beam;
  return {};
}

double beam_reach(const Beam &beam, double cutoff) {
  const double mean = 0.5 * (beam.a + beam.c);
  const double half = 0.5 * (beam.a - beam.c);
  const double smaller = mean - std::sqrt(half * half + beam.b * beam.b);
  return std::floor(std::sqrt(-std::log(cutoff) / smaller));
}

void beam_taps(const Beam &beam, int radius, float *taps) {
  const int side = 2 * radius + 1;
  for (int dy = -radius; dy <= radius; ++dy)
    for (int dx = -radius; dx <= radius; ++dx) {
      const double x = dx, y = dy;
      taps[(dy + radius) * side + dx + radius] = static_cast<float>(
          std::exp(-(beam.a * (x * x) + (2.0 * beam.b) * (x * y) +
                     beam.c * (y * y))));
    }
}

std::string restore(const rs::Params &p, const float *model,
                    const float *residual, const float *taps,
                    float *restored) {
  const int G = p.grid_size, R = p.radius, side = 2 * R + 1;
  const size_t cells = static_cast<size_t>(G) * G;
  // zeroed pages the sparse walk never touches cost nothing
  float *acc = static_cast<float *>(std::calloc(cells, sizeof(float)));
  if (acc == nullptr) return "idg_restore: no memory for the accumulator";
  for (int ys = 0; ys < G; ++ys) {
    const float *mrow = model + static_cast<size_t>(ys) * G;
    for (int xs = 0; xs < G; ++xs) {
      const float m = mrow[xs];
      if (!rs::taken(m)) continue;
      const int y0 = ys - R > 0 ? ys - R : 0;
      const int y1 = ys + R < G - 1 ? ys + R : G - 1;
      const int x0 = xs - R > 0 ? xs - R : 0;
      const int x1 = xs + R < G - 1 ? xs + R : G - 1;
      for (int y = y0; y <= y1; ++y) {
        float *arow = acc + static_cast<size_t>(y) * G;
        const float *trow = taps + (y - ys + R) * side + (R - xs);
        for (int x = x0; x <= x1; ++x)
          arow[x] = rs::accumulate(m, trow[x], arow[x]);
      }
    }
  }
  const bool has = residual != nullptr;
  for (size_t i = 0; i < cells; ++i)
    restored[i] = rs::finish(has, has ? residual[i] : 0.0f, acc[i]);
  std::free(acc);
  return {};
}

}  // namespace host
}  // namespace idg_mi355x
