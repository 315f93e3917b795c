// image_mi355x.hip.cpp -- the steps between the uv grid and the image
// (DESIGN.md §13): the G x G grid FFT with the centre shifts inside its
// passes, and the w-stacking phasor with the sum (or broadcast) over the
// w-layers and the taper correction as one per-pixel launch beside it.
//
// None of this is in the reference.  The conventions are those the oracle
// gridder / degridder and the adder / splitter (pipeline_mi355x.hip.cpp)
// require, derived numerically (tests/test_image_host.py):
//
//   grid_to_image: image[pol][i][j] = correction[i][j] *
//       sum_z exp(-2 pi i w_step (z + 0.5) n(l_j, m_i)) *
//       sum_{Y,X} grid[z][pol][Y][X] *
//                 exp(-2 pi i ((X - G/2)(j - G/2) + (Y - G/2)(i - G/2)) / G)
//   image_to_grid: its exact adjoint, every layer overwritten
//
// with l_j = (j - G/2) image_size / G and n = 1 - sqrt(1 - l^2 - m^2).  No
// further phase ramp and no factor of G: the uv cell (X - G/2, Y - G/2) and
// the image pixel (j - G/2, i - G/2) are both integer-centred, and 4 | G
// makes exp(-i pi G / 2) = 1, so the centre shifts are the sign flips
// (-1)^(X + Y) on the grid side and (-1)^(i + j) on the image side.
//
// A length G = N1 N2 transform (N1, N2 in {8, 16, 32, 64}) of sequence
// element p = N2 n1 + n2 to output k = k1 + N1 k2:
//   step A  item (sequence, n2): N1 values into registers, the N1-point
//           transform (fft.hpp), times exp(sign 2 pi i n2 k1 / G), to LDS at
//           [k1][n2] (rows padded to N2 + 1: step B's reads hit 32 distinct
//           8-byte bank pairs);
//   step B  item (sequence, k1): N2 values from LDS, the N2-point transform,
//           outputs k1 + N1 k2 to memory.
// A workgroup of 256 threads takes B = 256 / max(N1, N2) sequences, one item
// per thread in each step; both steps read and write memory straight from
// registers, so a plane passes through LDS once per pass.  Sequences are
// rows (row pass: lanes along the row) or B adjacent columns (column pass:
// lanes across the columns first, panels of neighbouring columns on one XCD).
// Passes are ordered by kernel boundaries: no atomics, no cross-workgroup
// waits, no scratch besides the grid itself.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../util.hpp"
#include "device.hpp"
#include "fft.hpp"  // cmulf, fft_dif_registers, bit_reverse

namespace idg_mi355x {

namespace {

// cos / sin of 2 pi j / 64, j < 32, rounded from double: the register
// transforms' twiddles, constants after unrolling.
__device__ __forceinline__ constexpr float cos64(int j) {
  constexpr float t[32] = {
      1.0f,          0.99518472f,   0.980785251f,  0.956940353f,
      0.923879504f,  0.881921291f,  0.831469595f,  0.773010433f,
      0.707106769f,  0.634393275f,  0.555570245f,  0.471396744f,
      0.382683426f,  0.290284663f,  0.195090324f,  0.0980171412f,
      0.0f,          -0.0980171412f, -0.195090324f, -0.290284663f,
      -0.382683426f, -0.471396744f, -0.555570245f, -0.634393275f,
      -0.707106769f, -0.773010433f, -0.831469595f, -0.881921291f,
      -0.923879504f, -0.956940353f, -0.980785251f, -0.99518472f};
  return t[j];
}
__device__ __forceinline__ constexpr float sin64(int j) {
  return j <= 16 ? cos64(16 - j) : cos64(j - 16);
}

template <int N>
__device__ __forceinline__ void register_twiddles(float2 (&tw)[N / 2],
                                                  float sign) {
#pragma unroll
  for (int j = 0; j < N / 2; ++j)
    tw[j] = make_float2(cos64(j * (64 / N)), sign * sin64(j * (64 / N)));
}

// exp(sign 2 pi i j / G), 0 <= j < G, G a power of two: 2 j / G is exact
// and sincospif has no argument reduction to lose anything in.
__device__ __forceinline__ float2 step_twiddle(int j, float two_over_g,
                                               float sign) {
  float s, c;
  sincospif(static_cast<float>(j) * two_over_g, &s, &c);
  return make_float2(c, sign * s);
}

// exp(sgn 2 pi i wrev n(l, m)), wrev = w_step (z + 0.5) in wavelengths: n
// and the product in double, reduced to a revolution before the f32
// sin / cos, so phases of hundreds of radians keep f32-accurate phasors.
__device__ __forceinline__ float2 w_phasor(double l2, double m, double wrev,
                                           float sgn) {
  const double tmp = __builtin_fma(m, m, l2);
  const double n = tmp > 1.0 ? 1.0 : tmp / (1.0 + __builtin_sqrt(1.0 - tmp));
  const double rev = wrev * n;
  const double r = rev - __builtin_rint(rev);
  float s, c;
  sincospif(static_cast<float>(2.0 * r), &s, &c);
  return make_float2(c, sgn * s);
}

__device__ __forceinline__ float2 flip_if(float2 v, int odd) {
  return (odd & 1) ? make_float2(-v.x, -v.y) : v;
}

template <int N1, int N2, bool COLS>
struct Pass {
  static constexpr int G = N1 * N2;
  static constexpr int NMAX = N1 > N2 ? N1 : N2;
  static constexpr int B = 256 / NMAX;  // sequences per workgroup
  static constexpr int RS = N2 + 1;     // padded LDS row (complex)
  static constexpr int kLds = B * N1 * RS;
  static_assert(N1 * N2 >= 64 && NMAX <= 64 && G % B == 0, "shape");

  __device__ static int lds_index(int b, int k1, int n2) {
    return COLS ? (k1 * RS + n2) * B + b : (b * N1 + k1) * RS + n2;
  }
  // step A item of thread t: sequence b, residue n2 (t < B N2)
  __device__ static void item_a(int t, int *b, int *n2) {
    if (COLS) {
      *b = t % B;
      *n2 = t / B;
    } else {
      *n2 = t % N2;
      *b = t / N2;
    }
  }
  // step B item of thread t: sequence b, output residue k1 (t < B N1)
  __device__ static void item_b(int t, int *b, int *k1) {
    if (COLS) {
      *b = t % B;
      *k1 = t / B;
    } else {
      *k1 = t % N1;
      *b = t / N1;
    }
  }
  // offset of element p of sequence b in a plane whose first sequence of
  // this workgroup is s0
  __device__ static size_t offset(int s0, int b, int p) {
    return COLS ? static_cast<size_t>(p) * G + s0 + b
                : static_cast<size_t>(s0 + b) * G + p;
  }

  // x[n1] = element N2 n1 + n2 on entry; on exit the transformed, twiddled
  // values are in LDS
  __device__ static void step_a(float2 (&x)[N1], float2 *lds, int b, int n2,
                                float sign) {
    float2 tw[N1 / 2];
    register_twiddles<N1>(tw, sign);
    fft_dif_registers<N1>(x, tw);
    const float two_over_g = 2.0f / static_cast<float>(G);
#pragma unroll
    for (int k1 = 0; k1 < N1; ++k1) {
      const float2 v = x[bit_reverse<N1>(k1)];
      lds[lds_index(b, k1, n2)] =
          k1 == 0 ? v : cmulf(v, step_twiddle(n2 * k1, two_over_g, sign));
    }
  }
  // y[bit_reverse(k2)] = output k1 + N1 k2 on exit
  __device__ static void step_b(float2 (&y)[N2], const float2 *lds, int b,
                                int k1, float sign) {
#pragma unroll
    for (int n2 = 0; n2 < N2; ++n2) y[n2] = lds[lds_index(b, k1, n2)];
    float2 tw[N2 / 2];
    register_twiddles<N2>(tw, sign);
    fft_dif_registers<N2>(y, tw);
  }
};

// One pass of the plain transform, in place: the rows (COLS = false) or the
// columns of plane blockIdx.y.  flip bit 0: the input is multiplied by
// (-1)^(x + y); bit 1: the output.
template <int N1, int N2, bool COLS>
__global__ void __launch_bounds__(256)
    kernel_grid_fft_pass(float2 *__restrict__ planes, float sign, float scale,
                         int flip) {
  using P = Pass<N1, N2, COLS>;
  __shared__ float2 lds[P::kLds];
  const int tid = threadIdx.x;
  const int wg = COLS ? xcd_subgrid(blockIdx.x, gridDim.x) : blockIdx.x;
  const int s0 = wg * P::B;
  float2 *plane = planes + static_cast<size_t>(blockIdx.y) * P::G * P::G;
  if (tid < P::B * N2) {
    int b, n2;
    P::item_a(tid, &b, &n2);
    float2 x[N1];
#pragma unroll
    for (int n1 = 0; n1 < N1; ++n1) {
      const int p = N2 * n1 + n2;
      x[n1] = flip_if(plane[P::offset(s0, b, p)], flip & (s0 + b + p));
    }
    P::step_a(x, lds, b, n2, sign);
  }
  __syncthreads();
  if (tid < P::B * N1) {
    int b, k1;
    P::item_b(tid, &b, &k1);
    float2 y[N2];
    P::step_b(y, lds, b, k1, sign);
#pragma unroll
    for (int k2 = 0; k2 < N2; ++k2) {
      const int k = k1 + N1 * k2;
      const float2 v = y[bit_reverse<N2>(k2)];
      plane[P::offset(s0, b, k)] = flip_if(
          make_float2(v.x * scale, v.y * scale), (flip >> 1) & (s0 + b + k));
    }
  }
}

struct ImageArgs {
  int nr_w_layers;
  float image_size;
  float w_step;
  const float *correction;  // [G][G] or null
};

// The image-side work, a launch of its own beside the transform (inside the
// transform's row pass it measured slower): one thread per
// pixel, all four correlations (they share the w phasor), lanes along the
// row.
__global__ void __launch_bounds__(256)
    kernel_layers_to_image(const float2 *__restrict__ grid,
                           float2 *__restrict__ image, ImageArgs a, int G) {
  const size_t plane_px = static_cast<size_t>(G) * G;
  const size_t px = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  const int y = static_cast<int>(px / G), x = static_cast<int>(px % G);
  const double cell = static_cast<double>(a.image_size) / G;
  const double l = (x - G / 2) * cell, m = (y - G / 2) * cell;
  const bool use_w = a.w_step != 0.0f;
  float2 acc[4];
#pragma unroll
  for (int pol = 0; pol < 4; ++pol) acc[pol] = make_float2(0.0f, 0.0f);
  for (int z = 0; z < a.nr_w_layers; ++z) {
    float2 v[4];
#pragma unroll
    for (int pol = 0; pol < 4; ++pol)
      v[pol] = grid[(static_cast<size_t>(z) * 4 + pol) * plane_px + px];
    const float2 ph =
        use_w ? w_phasor(l * l, m, static_cast<double>(a.w_step) * (z + 0.5),
                         -1.0f)
              : make_float2(1.0f, 0.0f);
#pragma unroll
    for (int pol = 0; pol < 4; ++pol) {
      const float2 w = use_w ? cmulf(v[pol], ph) : v[pol];
      acc[pol].x += w.x;
      acc[pol].y += w.y;
    }
  }
  const float c = a.correction != nullptr ? a.correction[px] : 1.0f;
#pragma unroll
  for (int pol = 0; pol < 4; ++pol)
    image[pol * plane_px + px] =
        flip_if(make_float2(acc[pol].x * c, acc[pol].y * c), x + y);
}

__global__ void __launch_bounds__(256)
    kernel_image_to_layers(const float2 *__restrict__ image,
                           float2 *__restrict__ grid, ImageArgs a, int G) {
  const size_t plane_px = static_cast<size_t>(G) * G;
  const size_t px = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  const int y = static_cast<int>(px / G), x = static_cast<int>(px % G);
  const double cell = static_cast<double>(a.image_size) / G;
  const double l = (x - G / 2) * cell, m = (y - G / 2) * cell;
  const bool use_w = a.w_step != 0.0f;
  const float c = a.correction != nullptr ? a.correction[px] : 1.0f;
  float2 v[4];
#pragma unroll
  for (int pol = 0; pol < 4; ++pol) {
    const float2 s = image[pol * plane_px + px];
    v[pol] = flip_if(make_float2(s.x * c, s.y * c), x + y);
  }
  for (int z = 0; z < a.nr_w_layers; ++z) {
    const float2 ph =
        use_w ? w_phasor(l * l, m, static_cast<double>(a.w_step) * (z + 0.5),
                         1.0f)
              : make_float2(1.0f, 0.0f);
#pragma unroll
    for (int pol = 0; pol < 4; ++pol)
      grid[(static_cast<size_t>(z) * 4 + pol) * plane_px + px] =
          use_w ? cmulf(v[pol], ph) : v[pol];
  }
}

template <int N1, int N2, bool COLS>
hipError_t launch_pass(void *planes, int nr_planes, float sign, float scale,
                       int flip, hipStream_t stream) {
  using P = Pass<N1, N2, COLS>;
  hipLaunchKernelGGL((kernel_grid_fft_pass<N1, N2, COLS>),
                     dim3(P::G / P::B, nr_planes), dim3(256), 0, stream,
                     static_cast<float2 *>(planes), sign, scale, flip);
  return hipGetLastError();
}

enum class Op { kFft, kToImage, kToGrid };

struct Call {
  Op op;
  int nr_planes;  // kFft
  float sign, scale;
  ImageArgs image;
  void *grid;   // the planes of kFft
  void *pixels;  // the image
};

// The plain transform; grid_to_image: the transform (sign -1, the grid-side
// flip on the column pass's loads), then the layers onto the image;
// image_to_grid: the image onto the layers, then the transform (sign +1, the
// flip on the row pass's stores).
template <int N1, int N2>
hipError_t run(const Call &c, hipStream_t stream) {
  constexpr int G = N1 * N2;
  const int planes = 4 * c.image.nr_w_layers;
  const dim3 per_pixel(G * G / 256);
  hipError_t err = hipSuccess;
  switch (c.op) {
    case Op::kFft:
      err = launch_pass<N1, N2, false>(c.grid, c.nr_planes, c.sign, 1.0f, 0,
                                       stream);
      if (err != hipSuccess) return err;
      return launch_pass<N1, N2, true>(c.grid, c.nr_planes, c.sign, c.scale,
                                       0, stream);
    case Op::kToImage:
      err = launch_pass<N1, N2, true>(c.grid, planes, -1.0f, 1.0f, 1, stream);
      if (err != hipSuccess) return err;
      err = launch_pass<N1, N2, false>(c.grid, planes, -1.0f, 1.0f, 0, stream);
      if (err != hipSuccess) return err;
      hipLaunchKernelGGL(kernel_layers_to_image, per_pixel, dim3(256), 0,
                         stream, static_cast<const float2 *>(c.grid),
                         static_cast<float2 *>(c.pixels), c.image, G);
      return hipGetLastError();
    case Op::kToGrid:
      hipLaunchKernelGGL(kernel_image_to_layers, per_pixel, dim3(256), 0,
                         stream, static_cast<const float2 *>(c.pixels),
                         static_cast<float2 *>(c.grid), c.image, G);
      err = hipGetLastError();
      if (err != hipSuccess) return err;
      err = launch_pass<N1, N2, true>(c.grid, planes, 1.0f, 1.0f, 0, stream);
      if (err != hipSuccess) return err;
      return launch_pass<N1, N2, false>(c.grid, planes, 1.0f, 1.0f, 2, stream);
  }
  return hipErrorInvalidValue;
}

hipError_t dispatch(int G, const Call &c, hipStream_t stream) {
  switch (G) {
    case 64: return run<8, 8>(c, stream);
    case 128: return run<8, 16>(c, stream);
    case 256: return run<16, 16>(c, stream);
    case 512: return run<16, 32>(c, stream);
    case 1024: return run<32, 32>(c, stream);
    case 2048: return run<32, 64>(c, stream);
    case 4096: return run<64, 64>(c, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

bool grid_fft_supported(int grid_size) {
  return grid_size >= 64 && grid_size <= 4096 &&
         (grid_size & (grid_size - 1)) == 0;
}

hipError_t launch_grid_fft(int grid_size, int nr_planes, int sign, float scale,
                           void *d_planes, hipStream_t stream) {
  if (!grid_fft_supported(grid_size)) return hipErrorInvalidValue;
  const size_t plane_px = static_cast<size_t>(grid_size) * grid_size;
  // the planes are the launch grid's y: at most 65,535 per launch
  for (int p0 = 0; p0 < nr_planes; p0 += 65535) {
    Call c{};
    c.op = Op::kFft;
    c.nr_planes = std::min(65535, nr_planes - p0);
    c.sign = sign >= 0 ? 1.0f : -1.0f;
    c.scale = scale;
    c.grid = static_cast<float2 *>(d_planes) + p0 * plane_px;
    const hipError_t err = dispatch(grid_size, c, stream);
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

hipError_t launch_grid_to_image(int grid_size, int nr_w_layers,
                                float image_size, float w_step_in_lambda,
                                const float *d_correction, void *d_grid,
                                void *d_image, hipStream_t stream) {
  Call c{};
  c.op = Op::kToImage;
  c.image = ImageArgs{nr_w_layers, image_size, w_step_in_lambda, d_correction};
  c.grid = d_grid;
  c.pixels = d_image;
  return dispatch(grid_size, c, stream);
}

hipError_t launch_image_to_grid(int grid_size, int nr_w_layers,
                                float image_size, float w_step_in_lambda,
                                const float *d_correction, const void *d_image,
                                void *d_grid, hipStream_t stream) {
  Call c{};
  c.op = Op::kToGrid;
  c.image = ImageArgs{nr_w_layers, image_size, w_step_in_lambda, d_correction};
  c.grid = d_grid;
  c.pixels = const_cast<void *>(d_image);
  return dispatch(grid_size, c, stream);
}

}  // namespace idg_mi355x
