// clark_mi355x.hip.cpp -- Clark CLEAN on the device, bit for bit
// the host entry idg_clark (host/clark.cpp; common/clark.hpp and
// common/clean.hpp hold the arithmetic of both).  A round selects the
// brightest pixels, runs the minor cycle on that list inside one workgroup --
// many components per launch, __syncthreads() its only ordering -- and then
// subtracts the components found from the whole residual.  The image is cut
// into the tiles of minor_cycle.hpp (kTileCols columns x `rows` rows).
//   begin    one workgroup: the caller's record into the workspace, the
//            histogram and the counter zeroed
//   per round, in this order:
//   scan     every tile's peak as a partial (key and signed value, as
//            minor::search leaves them) and the histogram of the magnitude
//            bins: uint32 LDS atomics per workgroup, then integer global
//            atomics on the occupied bins
//   limit    one workgroup: the peak from the partials, the decision of the
//            round's step 1, the suffix counts of the bins, tbits and
//            round_limit; it reads each bin once and zeroes it behind itself
//   compact  {index, value} of every candidate into the list through an
//            integer counter; a tile whose partial lies below the limit reads
//            no pixel
//   cycle    one workgroup of 1,024 threads, a thread's candidates in its
//            registers: per iteration one workgroup max, the decision taken
//            by every thread from the same inputs, the subtraction on the
//            thread's own entries inside the patch
//   apply    a workgroup streams the round's records through LDS, keeps in
//            record order those whose patch meets its tile, and runs per
//            pixel the fmafs in that order; a tile no patch meets reads no
//            pixel
//   after the last round:
//   scan     (without the histogram) the partials of the residual as it stands
//   finish   one workgroup: the state's peak, the state back to the caller
// No scratch, no cross-workgroup wait: kernel boundaries order the launches.
// The only atomics are integer adds, whose sums do not depend on any order,
// and the list's order, which does, is seen by nothing outside: the peak is
// an integer max, and an entry's subtraction is its own.  Per buffer:
//   residual    read by scan and compact; apply: a workgroup reads and writes
//               the pixels of its own tile
//   psf, mask   read only
//   model       cycle: a pixel is read and written by the one thread that
//               holds its list entry
//   components  written by cycle (the thread that holds the peak), read by
//               apply
//   partials    written by scan, read by limit, compact and finish
//   histogram   scan adds, limit reads and zeroes
//   list, counter   compact writes, cycle reads; limit zeroes the counter
//   state       written by the one-workgroup launches only (begin, limit,
//               cycle), read by the others; the caller's record is read by
//               begin and written by finish
// Workspace (util.hpp kWorkspaceClark): all of the above but the caller's.
#include "common/clark.hpp"
#include "hip/kernels/minor_cycle.hpp"

namespace idg_mi355x {

namespace {

using minor::block_max;
using minor::kBlock;
using minor::kTileCols;
using minor::kWaves;
using minor::Tiling;
using minor::u64;

constexpr int kCycleBlock = 1024;
constexpr int kCycleWaves = kCycleBlock / 64;
constexpr int kMaxSlots = clark::kMaxCandidates / kCycleBlock;
constexpr int kBinsPerThread = clark::kBins / kBlock;
static_assert(kBinsPerThread == 16 && kMaxSlots == 16, "the limit's scan");

// The state as the launches hand it on.
struct alignas(8) DevState {
  clark::State s;
  uint32_t tbits;  // the round's limit
  int32_t n0;      // n_components when the round began: apply's first record
  int32_t live;    // the round has a limit: compact and cycle run
};
static_assert(sizeof(DevState) == 48, "the lease's layout");

__device__ inline bool runs(const clark::State &s, const clark::Params &p) {
  return s.base.reason == clean::kRunning && clean::state_ok(s.base, p.base);
}

// The groups of pixels of tile `tile` this thread owns, as minor::scan_tile
// cuts them: body(y, col) for a group of kVec ? 4 : 1 pixels from column col
// of row y.  kVec: G % 4 == 0 and the planes are aligned.
template <bool kVec, class Body>
__device__ inline void for_tile(int G, const Tiling &t, int tile, Body body) {
  const int tid = threadIdx.x;
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows;
  const int row1 = row0 + t.rows < G ? row0 + t.rows : G;
  const int col = tx * kTileCols + (kVec ? (tid & 63) * 4 : tid);
  if (col >= G) return;
  for (int y = row0 + (kVec ? tid >> 6 : 0); y < row1; y += kVec ? kWaves : 1)
    body(y, col);
}

template <bool kVec>
__device__ inline void load_group(const float *plane,
                                  const uint8_t *__restrict__ mask, size_t at,
                                  float *r, uint32_t *m) {
  *m = 0x01010101u;
  if constexpr (kVec) {
    const float4 v = *reinterpret_cast<const float4 *>(plane + at);
    r[0] = v.x, r[1] = v.y, r[2] = v.z, r[3] = v.w;
    if (mask != nullptr) *m = *reinterpret_cast<const uint32_t *>(mask + at);
  } else {
    r[0] = plane[at];
    if (mask != nullptr) *m = mask[at];
  }
}

__global__ void __launch_bounds__(kBlock)
    kernel_clark_begin_mi355x(const clark::State *caller_state, DevState *st,
                              uint32_t *hist, uint32_t *count) {
  for (int i = threadIdx.x; i < clark::kBins; i += kBlock) hist[i] = 0;
  if (threadIdx.x == 0) {
    DevState d;
    d.s = *caller_state;
    d.tbits = 0;
    d.n0 = d.s.base.n_components;
    d.live = 0;
    *st = d;
    *count = 0;
  }
}

// kHist: a round's scan, which runs only from a state a round may run from;
// else the scan before finish, which always runs.
template <bool kVec, bool kHist>
__global__ void __launch_bounds__(kBlock)
    kernel_clark_scan_mi355x(clark::Params p, Tiling t,
                             const float *__restrict__ residual,
                             const uint8_t *__restrict__ mask,
                             const DevState *__restrict__ st, u64 *keys_out,
                             float *vals_out, uint32_t *hist) {
  constexpr int kN = kVec ? 4 : 1;
  __shared__ u64 lds[kWaves];
  __shared__ uint32_t lds_hist[kHist ? clark::kBins : 1];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int G = p.base.grid_size;
  // whole bins below the level's never decide the limit (clark::limit_bits)
  uint32_t floor_bin = 0;
  if constexpr (kHist) {
    const clark::State s = st->s;
    if (!runs(s, p)) return;
    if (s.base.started != 0) floor_bin = clark::bin_of(s.base.level);
    for (int i = tid; i < clark::kBins; i += kBlock) lds_hist[i] = 0;
    __syncthreads();
  }
  u64 best = 0;
  float best_v = 0.0f;
  for_tile<kVec>(G, t, tile, [&](int y, int col) {
    const size_t at = static_cast<size_t>(y) * G + col;
    float r[kN];
    uint32_t m;
    load_group<kVec>(residual, mask, at, r, &m);
#pragma unroll
    for (int k = 0; k < kN; ++k) {
      const u64 key = clean::key_of(r[k], static_cast<uint32_t>(at + k),
                                    ((m >> (8 * k)) & 0xffu) != 0);
      if (key > best) {
        best = key;
        best_v = r[k];
      }
      if constexpr (kHist) {
        const uint32_t bin = clark::bin_of(r[k]);
        if (key != 0 && bin >= floor_bin) atomicAdd(&lds_hist[bin], 1u);
      }
    }
  });
  const u64 top = block_max(best, lds);  // (its barrier ends the LDS adds)
  if (top != 0 ? best == top : tid == 0) {
    keys_out[tile] = top;
    vals_out[tile] = top != 0 ? best_v : 0.0f;
  }
  if constexpr (kHist) {
    for (int i = tid; i < clark::kBins; i += kBlock) {
      const uint32_t c = lds_hist[i];
      if (c != 0) atomicAdd(&hist[i], c);
    }
  }
}

__global__ void __launch_bounds__(kBlock)
    kernel_clark_limit_mi355x(clark::Params p, Tiling t, DevState *st,
                              const u64 *__restrict__ keys,
                              const float *__restrict__ vals, uint32_t *hist,
                              uint32_t *count) {
  __shared__ u64 lds[kWaves];
  __shared__ uint32_t lds_chunk[kBlock];
  __shared__ uint32_t lds_over, lds_occupied;
  const int tid = threadIdx.x;
  DevState d = *st;
  if (!runs(d.s, p)) {
    // (scan added nothing.)  No record is new: apply does nothing.
    if (tid == 0) {
      st->n0 = d.s.base.n_components;
      st->live = 0;
    }
    return;
  }
  u64 key = 0;
  for (int i = tid; i < t.nr_tiles; i += kBlock) {
    const u64 k = keys[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds);
  float v = 0.0f;
  if (key != 0) {
    const uint32_t index = clean::index_of(key);
    const int G = p.base.grid_size;
    const int py = static_cast<int>(index / static_cast<uint32_t>(G));
    const int px = static_cast<int>(index - static_cast<uint32_t>(py) * G);
    v = vals[(py / t.rows) * t.tiles_x + px / kTileCols];
  }
  const bool go = clark::begin_round(&d.s, p, key, v);

  // bins [16 tid, 16 tid + 16): read once, zeroed for the next round
  uint4 *mine = reinterpret_cast<uint4 *>(hist) + tid * (kBinsPerThread / 4);
  uint32_t h[kBinsPerThread];
  uint32_t sum = 0;
#pragma unroll
  for (int q = 0; q < kBinsPerThread / 4; ++q) {
    const uint4 w = mine[q];
    h[4 * q] = w.x, h[4 * q + 1] = w.y, h[4 * q + 2] = w.z, h[4 * q + 3] = w.w;
    sum += w.x + w.y + w.z + w.w;
    mine[q] = make_uint4(0, 0, 0, 0);
  }
  lds_chunk[tid] = sum;
  if (tid == 0) lds_over = 0, lds_occupied = 0;
  __syncthreads();
  uint32_t suffix = 0;
  for (int j = tid + 1; j < kBlock; ++j) suffix += lds_chunk[j];
  uint32_t over = 0, occupied = 0;
#pragma unroll
  for (int k = kBinsPerThread - 1; k >= 0; --k) {
    suffix += h[k];
    over += suffix > static_cast<uint32_t>(p.max_candidates) ? 1u : 0u;
    occupied += suffix > 0 ? 1u : 0u;
  }
  if (over != 0) atomicAdd(&lds_over, over);
  if (occupied != 0) atomicAdd(&lds_occupied, occupied);
  __syncthreads();
  if (tid == 0) {
    d.n0 = d.s.base.n_components;
    d.live = 0;
    if (go) {
      d.tbits = clark::limit_bits(d.s.base.level, p.select_fraction, v,
                                  lds_over, lds_occupied);
      d.s.round_limit = clean::float_of(d.tbits);
      d.live = 1;
      *count = 0;
    }
    *st = d;
  }
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_clark_compact_mi355x(clark::Params p, Tiling t,
                                const float *__restrict__ residual,
                                const uint8_t *__restrict__ mask,
                                const DevState *__restrict__ st,
                                const u64 *__restrict__ keys, uint32_t *count,
                                uint2 *list) {
  constexpr int kN = kVec ? 4 : 1;
  const int tile = blockIdx.x;
  if (st->live == 0) return;
  const uint32_t tbits = st->tbits;
  // the tile's largest searchable magnitude is below the limit
  if (static_cast<uint32_t>(keys[tile] >> 32) < tbits) return;
  const int G = p.base.grid_size;
  const uint32_t room = static_cast<uint32_t>(p.max_candidates);
  for_tile<kVec>(G, t, tile, [&](int y, int col) {
    const size_t at = static_cast<size_t>(y) * G + col;
    float r[kN];
    uint32_t m;
    load_group<kVec>(residual, mask, at, r, &m);
#pragma unroll
    for (int k = 0; k < kN; ++k) {
      if (clark::is_candidate(r[k], ((m >> (8 * k)) & 0xffu) != 0, tbits)) {
        // (per lane in the source; the compiler issues one add a wave)
        const uint32_t to = atomicAdd(count, 1u);
        // (the limit keeps the count within max_candidates; no bug may write
        // past the lease)
        if (to < room)
          list[to] = make_uint2(static_cast<uint32_t>(at + k),
                                clean::bits_of(r[k]));
      }
    }
  });
}

// A listed pixel in a register: y << 14 | x, which orders as the linear index
// does (x < 2^14) and needs no division by G.
constexpr int kPosShift = 14;
constexpr uint32_t kPosMask = (1u << 28) - 1;

// kSlots: candidates a thread holds, entries slot * 1024 + tid of the list.
template <int kSlots>
__global__ void __launch_bounds__(kCycleBlock)
    kernel_clark_cycle_mi355x(clark::Params p, DevState *st,
                              const uint32_t *__restrict__ count,
                              const uint2 *__restrict__ list,
                              const float *__restrict__ psf, float *model,
                              clean::Component *components) {
  // one barrier an iteration: iteration k's slots are rewritten by k + 2,
  // which no wave reaches before every wave has read them and met barrier k + 1
  __shared__ u64 lds[2][kCycleWaves];
  const int tid = threadIdx.x;
  DevState d = *st;
  if (d.live == 0) return;
  const uint32_t counted = *count;
  const uint32_t n = counted < static_cast<uint32_t>(p.max_candidates)
                         ? counted
                         : static_cast<uint32_t>(p.max_candidates);
  d.s.n_candidates = static_cast<int32_t>(n);
  if (n == 0) {
    d.s.base.reason = clark::kNoCandidate;
    if (tid == 0) *st = d;
    return;
  }
  const int G = p.base.grid_size, Gp = p.base.psf_size;
  const uint32_t tbits = d.tbits;

  // an empty slot holds a NaN: its key is 0 and no subtraction changes it
  uint32_t pos[kSlots];
  float val[kSlots];
#pragma unroll
  for (int j = 0; j < kSlots; ++j) {
    const uint32_t e = static_cast<uint32_t>(j) * kCycleBlock + tid;
    uint2 q = make_uint2(0u, 0x7fc00000u);
    if (e < n) q = list[e];
    const uint32_t y = q.x / static_cast<uint32_t>(G);
    pos[j] = (y << kPosShift) | (q.x - y * static_cast<uint32_t>(G));
    val[j] = clean::float_of(q.y);
  }

  for (int k = 0; k < p.iterations_per_round; ++k) {
    // The list's peak.  A thread's entry as |value|'s bits, then ~pos, then
    // the sign: ordered as clean::key_of orders (no two entries share a pos,
    // so the sign never decides), and the winner's signed value rides along.
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const uint32_t b = clean::bits_of(val[j]);
      const uint32_t mag = b & 0x7fffffffu;
      const u64 packed = (static_cast<u64>(mag) << 29) |
                         (static_cast<u64>(~pos[j] & kPosMask) << 1) |
                         (b >> 31);
      const u64 mine = mag <= 0x7f800000u ? packed : 0;
      best = mine > best ? mine : best;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const u64 o = __shfl_xor(best, s, 64);
      best = o > best ? o : best;
    }
    u64 *slot = lds[k & 1];
    if ((tid & 63) == 0) slot[tid >> 6] = best;
    __syncthreads();
    // (a lane reads one wave's and four shuffle steps finish the max: two
    // registers where reading all sixteen would take thirty-two)
    u64 top = slot[tid & (kCycleWaves - 1)];
#pragma unroll
    for (int s = kCycleWaves / 2; s > 0; s >>= 1) {
      const u64 o = __shfl_xor(top, s, 64);
      top = o > top ? o : top;
    }

    // the decision, by every thread from the same inputs
    const uint32_t mag = static_cast<uint32_t>(top >> 29);
    const uint32_t wpos = ~static_cast<uint32_t>(top >> 1) & kPosMask;
    const int py = static_cast<int>(wpos >> kPosShift);
    const int px = static_cast<int>(wpos & ((1u << kPosShift) - 1));
    const uint32_t index = static_cast<uint32_t>(py) * G + px;
    // (an all-zero entry: a zero at the last pixel of G = 16384, which like
    // key 0 is below every limit)
    const u64 key = top != 0 ? (static_cast<u64>(mag) << 32) | ~index : 0;
    const float v =
        clean::float_of(mag | (static_cast<uint32_t>(top & 1) << 31));
    if (!clark::in_round(key, tbits)) break;
    float c = 0.0f;
    if (!clean::step(&d.s.base, p.base, key, v, &c)) break;

    // The entry that is the peak: its holder records the component.  (One
    // workgroup, and a pixel has one holder: its adds to the model stay in
    // order.)
    const int oy = py - Gp / 2, ox = px - Gp / 2;
    if constexpr (kSlots <= 8) {
      // Every load of the iteration is issued before the first is waited
      // for -- the model pixel, then a tap per entry, from element 0 where
      // the entry lies outside the patch -- so an iteration pays one trip to
      // L2, not one per entry.
      bool holder = false;
#pragma unroll
      for (int j = 0; j < kSlots; ++j)
        holder = holder || (pos[j] == wpos &&
                            mag == (clean::bits_of(val[j]) & 0x7fffffffu));
      float m = 0.0f;
      if (holder) m = model[index];
      float tap[kSlots];
      bool inside[kSlots];
#pragma unroll
      for (int j = 0; j < kSlots; ++j) {
        const int dy = static_cast<int>(pos[j] >> kPosShift) - oy;
        const int dx = static_cast<int>(pos[j] & ((1u << kPosShift) - 1)) - ox;
        inside[j] = static_cast<uint32_t>(dy) < static_cast<uint32_t>(Gp) &&
                    static_cast<uint32_t>(dx) < static_cast<uint32_t>(Gp);
        tap[j] = psf[inside[j] ? static_cast<size_t>(dy) * Gp + dx : 0];
      }
#pragma unroll
      for (int j = 0; j < kSlots; ++j)
        val[j] = inside[j] ? clean::subtract(c, tap[j], val[j]) : val[j];
      if (holder) {
        components[d.s.base.n_components - 1] = {py, px, c};
        model[index] = m + c;
      }
    } else {
      // Sixteen entries a thread: that many taps in flight do not fit the 128
      // registers a workgroup of 1,024 threads leaves a thread without
      // scratch, so here an entry inside the patch loads and uses its own.
#pragma unroll
      for (int j = 0; j < kSlots; ++j) {
        const int dy = static_cast<int>(pos[j] >> kPosShift) - oy;
        const int dx = static_cast<int>(pos[j] & ((1u << kPosShift) - 1)) - ox;
        if (static_cast<uint32_t>(dy) < static_cast<uint32_t>(Gp) &&
            static_cast<uint32_t>(dx) < static_cast<uint32_t>(Gp)) {
          if (pos[j] == wpos &&
              mag == (clean::bits_of(val[j]) & 0x7fffffffu)) {
            components[d.s.base.n_components - 1] = {py, px, c};
            model[index] = model[index] + c;
          }
          val[j] = clean::subtract(
              c, psf[static_cast<size_t>(dy) * Gp + dx], val[j]);
        }
      }
    }
  }

  if (tid == 0) *st = d;
}

template <bool kVec>
__global__ void __launch_bounds__(kBlock)
    kernel_clark_apply_mi355x(clark::Params p, Tiling t, float *residual,
                              const float *__restrict__ psf,
                              const clean::Component *__restrict__ components,
                              const DevState *__restrict__ st) {
  constexpr int kN = kVec ? 4 : 1;
  __shared__ int lds_count[2][kWaves];
  __shared__ float lds_c[kBlock];
  __shared__ int2 lds_o[kBlock];  // {oy, ox}
  const int tid = threadIdx.x, lane = tid & 63, tile = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = st->n0, n1 = st->s.base.n_components;
  if (n1 <= n0) return;
  const int G = p.base.grid_size, Gp = p.base.psf_size;
  const int ty = tile / t.tiles_x, tx = tile - ty * t.tiles_x;
  const int row0 = ty * t.rows, col0 = tx * kTileCols;
  const int row1 = row0 + t.rows < G ? row0 + t.rows : G;
  const int col1 = col0 + kTileCols < G ? col0 + kTileCols : G;
  const u64 below = (1ull << lane) - 1;

  int round = 0;
  for (int first = n0; first < n1; first += kBlock, ++round) {
    const int i = first + tid;
    bool hit = false;
    clean::Component rec = {0, 0, 0.0f};
    if (i < n1) {
      rec = components[i];
      const clean::Patch pt = clean::patch_of(p.base, rec.y, rec.x);
      hit = row0 < pt.y1 && row1 > pt.y0 && col0 < pt.x1 && col1 > pt.x0;
    }
    const u64 b = __ballot(hit);
    // (the counts of round r + 1 go to the other set: a wave that found round
    // r empty may be there while another still reads round r's)
    if (lane == 0) lds_count[round & 1][wave] = __popcll(b);
    __syncthreads();
    int base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = lds_count[round & 1][w];
      base += w < wave ? c : 0;
      all += c;
    }
    if (all == 0) continue;
    if (hit) {
      const int to = base + __popcll(b & below);
      lds_c[to] = rec.value;
      lds_o[to] = make_int2(rec.y - Gp / 2, rec.x - Gp / 2);
    }
    __syncthreads();
    for_tile<kVec>(G, t, tile, [&](int y, int col) {
      const size_t at = static_cast<size_t>(y) * G + col;
      float r[kN];
      if constexpr (kVec) {
        const float4 q = *reinterpret_cast<const float4 *>(residual + at);
        r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
      } else {
        r[0] = residual[at];
      }
      bool any = false;
      for (int e = 0; e < all; ++e) {
        const int2 o = lds_o[e];
        const int dy = y - o.x;
        if (static_cast<uint32_t>(dy) >= static_cast<uint32_t>(Gp)) continue;
        const float c = lds_c[e];
        const float *prow = psf + static_cast<size_t>(dy) * Gp;
#pragma unroll
        for (int k = 0; k < kN; ++k) {
          const int dx = col + k - o.y;
          if (static_cast<uint32_t>(dx) < static_cast<uint32_t>(Gp)) {
            r[k] = clean::subtract(c, prow[dx], r[k]);
            any = true;
          }
        }
      }
      // (pixels of the float4 outside every patch go back as the bits read)
      if (any) {
        if constexpr (kVec)
          *reinterpret_cast<float4 *>(residual + at) =
              make_float4(r[0], r[1], r[2], r[3]);
        else
          residual[at] = r[0];
      }
    });
    // (the next round's list is written after its barrier)
  }
}

__global__ void __launch_bounds__(kBlock)
    kernel_clark_finish_mi355x(int nr_tiles, const DevState *__restrict__ st,
                               const u64 *__restrict__ keys,
                               clark::State *caller_state) {
  __shared__ u64 lds[kWaves];
  u64 key = 0;
  for (int i = threadIdx.x; i < nr_tiles; i += kBlock) {
    const u64 k = keys[i];
    key = k > key ? k : key;
  }
  key = block_max(key, lds);
  if (threadIdx.x == 0) {
    clark::State s = st->s;
    clean::set_peak(&s.base, key);
    *caller_state = s;
  }
}

template <int kSlots>
const void *cycle_kernel() {
  return reinterpret_cast<const void *>(&kernel_clark_cycle_mi355x<kSlots>);
}

}  // namespace

hipError_t launch_clark(const clark::Params &params, float *d_residual,
                        const float *d_psf, const uint8_t *d_mask,
                        float *d_model, void *d_components, void *d_state,
                        hipStream_t stream) {
  clark::Params p = params;
  const int G = p.base.grid_size;
  Tiling t = minor::tiling_of(G);
  const bool vec =
      G % 4 == 0 && minor::aligned(d_residual, 16) && minor::aligned(d_mask, 4);
  const size_t n = static_cast<size_t>(t.nr_tiles);
  const size_t room = static_cast<size_t>(p.max_candidates);
  WorkspaceLease lease;
  hipError_t err = lease.acquire(
      stream, kWorkspaceClark,
      n * sizeof(u64) + room * sizeof(uint2) + sizeof(DevState) +
          (clark::kBins + 4) * sizeof(uint32_t) + n * sizeof(float));
  if (err != hipSuccess) return err;
  // (the histogram first: the limit kernel reads it 16 bytes at a time)
  uint32_t *hist = static_cast<uint32_t *>(lease.ptr);
  u64 *keys = reinterpret_cast<u64 *>(hist + clark::kBins);
  uint2 *list = reinterpret_cast<uint2 *>(keys + n);
  DevState *st = reinterpret_cast<DevState *>(list + room);
  uint32_t *count = reinterpret_cast<uint32_t *>(st + 1);
  float *vals = reinterpret_cast<float *>(count + 4);

  const void *scan_hist =
      vec ? reinterpret_cast<const void *>(&kernel_clark_scan_mi355x<true, true>)
          : reinterpret_cast<const void *>(
                &kernel_clark_scan_mi355x<false, true>);
  const void *scan_only =
      vec ? reinterpret_cast<const void *>(
                &kernel_clark_scan_mi355x<true, false>)
          : reinterpret_cast<const void *>(
                &kernel_clark_scan_mi355x<false, false>);
  const void *compact =
      vec ? reinterpret_cast<const void *>(&kernel_clark_compact_mi355x<true>)
          : reinterpret_cast<const void *>(
                &kernel_clark_compact_mi355x<false>);
  const void *apply =
      vec ? reinterpret_cast<const void *>(&kernel_clark_apply_mi355x<true>)
          : reinterpret_cast<const void *>(&kernel_clark_apply_mi355x<false>);
  // the fewest slots a thread needs for max_candidates entries
  const void *cycle = room <= 1 * kCycleBlock   ? cycle_kernel<1>()
                      : room <= 2 * kCycleBlock ? cycle_kernel<2>()
                      : room <= 4 * kCycleBlock ? cycle_kernel<4>()
                      : room <= 8 * kCycleBlock ? cycle_kernel<8>()
                                                : cycle_kernel<16>();

  {
    void *args[] = {&d_state, &st, &hist, &count};
    err = hipLaunchKernel(
        reinterpret_cast<const void *>(&kernel_clark_begin_mi355x), dim3(1),
        dim3(kBlock), args, 0, stream);
    if (err != hipSuccess) return err;
  }
  void *scan_args[] = {&p, &t, &d_residual, &d_mask, &st, &keys, &vals, &hist};
  for (int r = 0; r < p.nr_rounds; ++r) {
    err = hipLaunchKernel(scan_hist, dim3(t.nr_tiles), dim3(kBlock), scan_args,
                          0, stream);
    if (err != hipSuccess) return err;
    void *limit_args[] = {&p, &t, &st, &keys, &vals, &hist, &count};
    err = hipLaunchKernel(
        reinterpret_cast<const void *>(&kernel_clark_limit_mi355x), dim3(1),
        dim3(kBlock), limit_args, 0, stream);
    if (err != hipSuccess) return err;
    void *compact_args[] = {&p,  &t,    &d_residual, &d_mask,
                            &st, &keys, &count,      &list};
    err = hipLaunchKernel(compact, dim3(t.nr_tiles), dim3(kBlock),
                          compact_args, 0, stream);
    if (err != hipSuccess) return err;
    void *cycle_args[] = {&p,     &st,      &count,       &list,
                          &d_psf, &d_model, &d_components};
    err = hipLaunchKernel(cycle, dim3(1), dim3(kCycleBlock), cycle_args, 0,
                          stream);
    if (err != hipSuccess) return err;
    void *apply_args[] = {&p, &t, &d_residual, &d_psf, &d_components, &st};
    err = hipLaunchKernel(apply, dim3(t.nr_tiles), dim3(kBlock), apply_args, 0,
                          stream);
    if (err != hipSuccess) return err;
  }
  err = hipLaunchKernel(scan_only, dim3(t.nr_tiles), dim3(kBlock), scan_args, 0,
                        stream);
  if (err != hipSuccess) return err;
  void *args[] = {&t.nr_tiles, &st, &keys, &d_state};
  return hipLaunchKernel(
      reinterpret_cast<const void *>(&kernel_clark_finish_mi355x), dim3(1),
      dim3(kBlock), args, 0, stream);
}

}  // namespace idg_mi355x
