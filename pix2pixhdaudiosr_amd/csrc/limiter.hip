// Whole-file generation (pix2pixhdaudiosr_amd/generate/): a look-ahead true-peak limiter -- a gain curve that brings every crest
// of the clip under a ceiling and leaves the rest of the clip alone, where the guard of truepeak.hip has one gain for the whole
// file.  Launch family "limiter", two launches per clip: the envelope, then the curve and its application.
//
// Inputs: the clip x[C][L] in fp32 as the encoder would see it, the ceiling c > 0, the look-ahead A in [1, 1024] and the hold H in
// [0, 4096] samples, the true-peak table tab[F][P] exactly as p2phd_truepeak takes it, the smoothing window w[0..A].
//
//   envelope   x~ and y[i][p] are those of truepeak.hip: x~ = the row, 0 outside [0, L), a NaN or infinite sample taken as 0;
//              y[i][p] = sum_k tab[p][k] x~[i + k - (P/2 - 1)] for p = 1 .. F - 1 and i = -1 .. L - 1: one fp32 accumulator from +0,
//              acc = fma(tab[p][k], x~, acc) for k = 0, 1, .., P - 1 in that order -- every y has the bits p2phd_truepeak gives it.
//              m[i] = max over channels of max(|x~[i]|, max_p |y[i][p]|, max_p |y[i-1][p]|)   for i = 0 .. L - 1: a sample answers
//              for the crests on both of its sides, and all channels share one curve, so the stereo image does not move.
//              r[i] = m[i] > c ? c / m[i] : 1, one fp32 division; r is taken as 1 outside [0, L).
//              peak = the largest m: the clip's true peak in front of the limiter, the largest tpeak of p2phd_truepeak bit for bit.
//   curve      h[j] = min(r[j - H .. j + A])        a sliding minimum, exact in any order
//              d[j] = 1.0f - h[j]
//              s[i] = sum_{k = 0 .. A} w[k] d[i - k]   one fp32 accumulator from +0, fma in ascending k
//              g[i] = min(r[i], 1.0f - s[i])
//              h[i - k] <= r[i] for every k in [-H, A] and sum w = 1: the curve never asks for less reduction than a sample needs,
//              and the final min makes that hold in fp32 too.  The deficit form makes g exactly 1 wherever nothing within reach is
//              over the ceiling: a tile whose staged r are all 1 copies its samples and skips the sums -- the same bits either way.
//   window     (host, float64) w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (A + 2)), divided by its sum, rounded once to fp32; w[k] and
//              w[A - k] are written from one value.
//   apply      out[c][i] = x[c][i] g[i], one fp32 multiply, into a buffer of its own; a non-finite sample passes through the
//              multiply as it is.
//   statistics the smallest g and the number of i with g[i] < 1, folded in the launch of the curve.
//
// The limited clip's own true peak can still lie a hair over c: the interpolator mixes neighbours that carry slightly different
// gains.  The limiter does not promise otherwise; p2phd_pcm_peak / p2phd_truepeak and the guard's one gain run behind it unchanged.
//
// envelope kernel: the staging and the walk of truepeak_kernel, both from firwalk.h (stage_finite, polyphase_walk_up), which owns
// the layout and the order of the fmas: the same code forms every y in both files.  Instant j stands for i = j - 1.
// The channels are walked inside the workgroup with the maxima kept in registers, so one r per sample leaves.  m[i] needs the
// fractional phases of instants i and i + 1: a tile of 2048 instants therefore yields 2047 samples, and tiles are laid 2047
// apart -- one instant in 2048 is formed twice, to the same bits.  Workgroup maxima of the bit patterns are stored and folded by
// the last workgroup (common.h: fold_arrive_last): nothing is zeroed before the launch, no float atomic.
// curve kernel: one tile of 2048 samples at a time; r with its 2 A + H halo is staged in LDS (at most 8192 floats).  The sliding
// minimum over W = A + H + 1 goes in two block passes: suffix minima and prefix minima of blocks of W, each a thread-local pass
// over a chunk of consecutive positions, a segmented scan of the 256 chunk results, and a pass that hands the carry on up to the
// chunk's first block edge; h = min(suffix[q], prefix[q + W - 1]).  Its cost does not grow with the window.  d is written in
// place of the suffix minima, in the padded layout of firwalk.h, and the sum takes the register-window walk of xover_kernel: a tap
// costs one conflict-free LDS read and 8 fmas per thread.  The sums go back through LDS, so that r, x, g and out are read and
// written with consecutive lanes on consecutive floats.  LDS: (2048 + 2 A + H) * 17 / 8 floats: 29 KiB at A = 240, H = 960,
// 68 KiB at the caps, beside 6.3 KiB of scan and fold arrays.
// No roofline claim: see DESIGN.md section 6.
#include "common.h"
#include "convplan.h"
#include "firwalk.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#pragma clang fp contract(off)      // d, 1 - s and the product x g are separately rounded; the tap products use fma explicitly

namespace {
constexpr int kThreads = 256;
constexpr int kIn = 8;                        // instants / samples per thread (firwalk.h)
constexpr int kTile = kThreads * kIn;         // instants per envelope tile, samples per curve tile
constexpr int kEnvStep = kTile - 1;           // samples an envelope tile yields
constexpr int kMaxLookahead = 1024, kMaxHold = 4096;
constexpr int kEnvParts = 16384;              // words of the fold region the envelope's partial maxima take
constexpr int kStatWords = 3;                 // per workgroup of the curve kernel: min g, count (low, high)

using namespace p2phd::fir;
static_assert(kThreads == kWalkThreads && kIn == 8, "firwalk.h is written for 256 threads of 8 outputs");

// NP = F - 1 fractional phases.  grid (gx): workgroup b takes tiles b, b + gx, ..; tile t holds instants 2047 t .. 2047 t + 2047
// and yields r of the samples 2047 t .. 2047 t + 2046.
template <int NP>
__global__ __launch_bounds__(kThreads) void limiter_envelope_kernel(const float* __restrict__ planar, long ld, long L, int C,
                                                                    const float* __restrict__ tab, int P, long tiles, float ceiling,
                                                                    float* __restrict__ r_out, uint32_t* __restrict__ part,
                                                                    unsigned* __restrict__ ticket, float* __restrict__ peak) {
  __shared__ float s_x[lds_floats(kTile + kMaxTaps)];
  __shared__ uint32_t s_full[kThreads * (kIn + 1)];               // per instant: max(|x~[i]|, max_p |y[i][p]|) over the channels
  __shared__ uint32_t s_frac[kThreads * (kIn + 1)];               // per instant: max_p |y[i][p]| over the channels
  __shared__ uint32_t s_pk[kThreads];
  const int tid = threadIdx.x, gx = gridDim.x;
  const int half = P / 2 - 1;                                     // taps in front of the instant's own sample
  const int base = tid * kIn;
  uint32_t pk = 0u;
  for (long tile = blockIdx.x; tile < tiles; tile += gx) {
    const long j0 = tile * kEnvStep;                              // first instant of the tile: i = j0 - 1
    const int len = (int)min((long)kTile, L + 1 - j0);            // instants of this tile, >= 2
    const int len8 = (len + kIn - 1) & ~(kIn - 1);                // ... up to whole threads: everything a thread reads is staged
    const int n = len8 + P - 1;                                   // staged samples: position q holds x~[j0 - 1 - half + q]
    const long g0 = j0 - 1 - half;
    uint32_t full[kIn], frac[kIn];
#pragma unroll
    for (int r = 0; r < kIn; ++r) full[r] = frac[r] = 0u;
    for (int c = 0; c < C; ++c) {
      stage_finite(s_x, planar + (long)c * ld, g0, n, L, tid);
      __syncthreads();
      if (base < len) {
        // phase 0: the instants' own samples (i = -1 holds x~ = 0)
#pragma unroll
        for (int r = 0; r < kIn; ++r) full[r] = max(full[r], abs_bits(s_x[pad8(base + r + half)]));
        if constexpr (NP > 0) {
          float acc[NP][kIn] = {};
          polyphase_walk_up<NP, kIn>(s_x, tab, P, base, n, acc);
#pragma unroll
          for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int r = 0; r < kIn; ++r) frac[r] = max(frac[r], abs_bits(acc[p][r]));
        }
      }
      __syncthreads();                                            // every window read is done: the region takes the next channel
    }
#pragma unroll
    for (int r = 0; r < kIn; ++r) {
      s_frac[tid * (kIn + 1) + r] = frac[r];                      // = pad8(base + r)
      s_full[tid * (kIn + 1) + r] = max(full[r], frac[r]);
    }
    __syncthreads();
    // sample q of the tile (i = j0 + q) lies between the instants q and q + 1
    for (int q = tid; q < len - 1; q += kThreads) {
      const uint32_t mb = max(s_frac[pad8(q)], s_full[pad8(q + 1)]);
      const float m = __uint_as_float(mb);
      r_out[j0 + q] = m > ceiling ? ceiling / m : 1.0f;
      pk = max(pk, mb);
    }
    __syncthreads();                                              // (the maxima are read: the arrays take the next tile)
  }
  lds_max256(s_pk, tid, pk);
  if (tid == 0) part_store(part + blockIdx.x, s_pk[0]);
  if (!p2phd::fold_arrive_last(ticket, (unsigned)gx)) return;
  // the last workgroup: a maximum does not depend on the order
  uint32_t p = 0u;
  for (int b = tid; b < gx; b += kThreads) p = max(p, part_load(part + b));
  lds_max256(s_pk, tid, p);
  if (tid == 0) *peak = __uint_as_float(s_pk[0]);
}

// Minima of blocks of W over the n staged r in s_r, from the block's first position up to each position (MIRROR = false, written
// in place) or from each position up to the block's last (MIRROR = true, written to s_s in the padded layout).  The walk runs
// over v = 0 .. total - 1, total = the blocks' whole span, v = p or total - 1 - p: positions behind n count as +inf.  Thread t
// takes the chunk v = t E .. t E + E - 1.
template <bool MIRROR>
__device__ __forceinline__ void block_minima(float* s_r, float* s_s, int n, int W, int total, int E, float (*s_v)[kThreads], int (*s_f)[kThreads]) {
  const int tid = threadIdx.x;
  const int v0 = min(tid * E, total), v1 = min(v0 + E, total);
  // the thread's own chunk: a running minimum that starts again at every block edge
  float run = INFINITY;
  int edge = 0, first = v1;                                       // first: the chunk's first block edge (v1: none)
  int ph = v0 % W;
  for (int v = v0; v < v1; ++v) {
    if (ph == 0) { run = INFINITY; if (!edge) first = v; edge = 1; }
    const int p = MIRROR ? total - 1 - v : v;
    if (p < n) {
      run = fminf(run, s_r[p]);
      if (MIRROR) s_s[pad8(p)] = run; else s_r[p] = run;
    }
    if (++ph == W) ph = 0;
  }
  // segmented scan of the chunk results (value: the minimum since the chunk's last edge, flag: the chunk holds an edge)
  int cur = 0;
  s_v[0][tid] = run; s_f[0][tid] = edge;
  __syncthreads();
  for (int o = 1; o < kThreads; o <<= 1) {
    float v2 = s_v[cur][tid]; int f2 = s_f[cur][tid];
    if (tid >= o) {
      const float v1_ = s_v[cur][tid - o]; const int f1 = s_f[cur][tid - o];
      if (!f2) v2 = fminf(v1_, v2);
      f2 |= f1;
    }
    s_v[cur ^ 1][tid] = v2; s_f[cur ^ 1][tid] = f2;
    cur ^= 1;
    __syncthreads();
  }
  // what the chunks in front hand on reaches up to the chunk's first edge
  const float carry = tid > 0 ? s_v[cur][tid - 1] : INFINITY;
  for (int v = v0; v < first; ++v) {
    const int p = MIRROR ? total - 1 - v : v;
    if (p < n) {
      if (MIRROR) s_s[pad8(p)] = fminf(s_s[pad8(p)], carry); else s_r[p] = fminf(s_r[p], carry);
    }
  }
  __syncthreads();
}

// s_min[0], s_cnt[0] = the smallest gmin and the sum of cnt of the 256 threads (neither depends on the order); ends behind a barrier
__device__ __forceinline__ void fold_stats(float* s_min, unsigned long long* s_cnt, int tid, float gmin, unsigned long long cnt) {
  s_min[tid] = gmin; s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) { s_min[tid] = fminf(s_min[tid], s_min[tid + o]); s_cnt[tid] += s_cnt[tid + o]; }
    __syncthreads();
  }
}

// grid (gx): workgroup b takes the tiles b, b + gx, .. of 2048 samples
__global__ __launch_bounds__(kThreads) void limiter_apply_kernel(const float* __restrict__ planar, long ld, long L, int C, const float* __restrict__ rr,
                                                                 int A, int H, const float* __restrict__ win, long tiles,
                                                                 float* __restrict__ out, long out_ld, float* __restrict__ g_out,
                                                                 uint32_t* __restrict__ part, unsigned* __restrict__ ticket,
                                                                 uint32_t* __restrict__ stats) {
  extern __shared__ float s_dyn[];
  __shared__ float s_v[2][kThreads];
  __shared__ int s_f[2][kThreads];
  __shared__ unsigned long long s_cnt[kThreads];
  const int tid = threadIdx.x, gx = gridDim.x;
  const int W = A + H + 1, taps = A + 1;
  float* s_r = s_dyn;                                             // r, then its prefix minima: kTile + 2 A + H floats
  float* s_s = s_dyn + (kTile + 2 * A + H);                       // suffix minima, then d, then the sums: padded layout
  const int base = tid * kIn;
  float gmin = 1.0f;
  unsigned long long cnt = 0ull;
  for (long tile = blockIdx.x; tile < tiles; tile += gx) {
    const long t0 = tile * kTile;
    const int len = (int)min((long)kTile, L - t0);                // samples of this tile, >= 1
    const int len8 = (len + kIn - 1) & ~(kIn - 1);
    const int nd = len8 + A;                                      // d: position q holds d[t0 - A + q]
    const int n = nd + A + H;                                     // r: position p holds r[t0 - A - H + p]
    const long g0 = t0 - A - H;
    int over = 0;
    for (int p = tid; p < n; p += kThreads) {
      const long j = g0 + p;
      float v = 1.0f;
      if (j >= 0 && j < L) v = rr[j];
      over |= __float_as_uint(v) != 0x3F800000u;
      s_r[p] = v;
    }
    if (!__syncthreads_or(over)) {
      // nothing within reach is over the ceiling: g is exactly 1
      for (int p = tid; p < len; p += kThreads) {
        if (g_out) g_out[t0 + p] = 1.0f;
        for (int c = 0; c < C; ++c) out[(long)c * out_ld + t0 + p] = planar[(long)c * ld + t0 + p];
      }
      __syncthreads();                                            // (the staged r are read: the region takes the next tile)
      continue;
    }
    const int total = (n + W - 1) / W * W;
    const int E = (total + kThreads - 1) / kThreads;
    block_minima<true>(s_r, s_s, n, W, total, E, s_v, s_f);
    block_minima<false>(s_r, s_s, n, W, total, E, s_v, s_f);
    for (int q = tid; q < nd; q += kThreads) {
      const float h = fminf(s_s[pad8(q)], s_r[q + W - 1]);
      s_s[pad8(q)] = 1.0f - h;
    }
    __syncthreads();
    float acc[kIn];
#pragma unroll
    for (int r = 0; r < kIn; ++r) acc[r] = 0.0f;
    if (base < len) {
      // sample r of this thread at tap k reads position base + r + (taps - 1 - k); w[r] is that d at the current tap
      float w[kIn];
#pragma unroll
      for (int r = 0; r < kIn; ++r) w[r] = s_s[pad8(base + r + taps - 1)];
      int k = 0;
      for (; k + kIn <= taps; k += kIn) {
        // eight taps with the window rotating through the registers: at step u the d of sample r is w[(r - u) & 7]
#pragma unroll
        for (int u = 0; u < kIn; ++u) {
          const float hk = win[k + u];
#pragma unroll
          for (int r = 0; r < kIn; ++r) acc[r] = __builtin_fmaf(hk, w[(r - u) & (kIn - 1)], acc[r]);
          // the next tap: every sample moves one position down, sample 0 takes a new one
          const int q = base + taps - 2 - (k + u);                // >= base - 1 at the last tap: then it is not read
          w[(-u - 1) & (kIn - 1)] = s_s[pad8(max(q, 0))];
        }
      }
      for (; k < taps; ++k) {                                     // the last taps mod 8, with the window in place
        const float hk = win[k];
#pragma unroll
        for (int r = 0; r < kIn; ++r) acc[r] = __builtin_fmaf(hk, w[r], acc[r]);
#pragma unroll
        for (int r = kIn - 1; r > 0; --r) w[r] = w[r - 1];
        w[0] = s_s[pad8(max(base + taps - 2 - k, 0))];
      }
    }
    __syncthreads();                                              // every window read is done: the region takes the sums
#pragma unroll
    for (int r = 0; r < kIn; ++r) s_s[tid * (kIn + 1) + r] = acc[r];           // = pad8(base + r)
    __syncthreads();
    for (int p = tid; p < len; p += kThreads) {
      const float g = fminf(rr[t0 + p], 1.0f - s_s[pad8(p)]);
      if (g_out) g_out[t0 + p] = g;
      for (int c = 0; c < C; ++c) out[(long)c * out_ld + t0 + p] = planar[(long)c * ld + t0 + p] * g;
      gmin = fminf(gmin, g);
      cnt += g < 1.0f ? 1ull : 0ull;
    }
    __syncthreads();                                              // (the sums are read: the region takes the next tile)
  }
  fold_stats(s_v[0], s_cnt, tid, gmin, cnt);
  if (tid == 0) {
    uint32_t* mine = part + (size_t)blockIdx.x * kStatWords;
    part_store(mine, __float_as_uint(s_v[0][0]));
    part_store(mine + 1, (uint32_t)s_cnt[0]);
    part_store(mine + 2, (uint32_t)(s_cnt[0] >> 32));
  }
  if (!p2phd::fold_arrive_last(ticket, (unsigned)gx)) return;
  // the last workgroup: a minimum and an integer sum do not depend on the order
  gmin = 1.0f; cnt = 0ull;
  for (int b = tid; b < gx; b += kThreads) {
    const uint32_t* its = part + (size_t)b * kStatWords;
    gmin = fminf(gmin, __uint_as_float(part_load(its)));
    cnt += (unsigned long long)part_load(its + 1) | ((unsigned long long)part_load(its + 2) << 32);
  }
  fold_stats(s_v[0], s_cnt, tid, gmin, cnt);
  if (tid == 0) {
    stats[0] = __float_as_uint(s_v[0][0]);
    stats[1] = s_cnt[0] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s_cnt[0];
  }
}

// workgroups: one per tile, as far as the partial table has rows (and the "limiter_grid" option allows)
int tile_grid(int64_t tiles, int64_t rows) {
  int64_t cap = rows;
  if (p2phd::g_opt_limiter_grid > 0) cap = std::min<int64_t>(cap, p2phd::g_opt_limiter_grid);
  return (int)std::max<int64_t>(1, std::min<int64_t>(tiles, cap));
}

bool spans_overlap(const float* a, int64_t ld_a, const float* b, int64_t ld_b, int64_t C, int64_t L) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a1 = a0 + (uintptr_t)((C - 1) * ld_a + L) * sizeof(float), b1 = b0 + (uintptr_t)((C - 1) * ld_b + L) * sizeof(float);
  return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int p2phd_limiter_tile_len(void) { return kTile; }

extern "C" int p2phd_limiter_window_fill(int lookahead, float* out) {
  P2PHD_REQUIRE(lookahead >= 1 && lookahead <= kMaxLookahead, "limiter_window_fill: lookahead must be in [1, %d], got %d", kMaxLookahead, lookahead);
  P2PHD_REQUIRE(out != nullptr, "limiter_window_fill: null output");
  const int A = lookahead;
  const double pi = 3.14159265358979323846;
  std::vector<double> v((size_t)A + 1);
  for (int k = 0; 2 * k <= A; ++k) {
    v[(size_t)k] = 0.5 - 0.5 * std::cos(2.0 * pi * (double)(k + 1) / (double)(A + 2));
    v[(size_t)(A - k)] = v[(size_t)k];                            // symmetric bit for bit
  }
  double sum = 0.0;
  for (int k = 0; k <= A; ++k) sum += v[(size_t)k];
  for (int k = 0; k <= A; ++k) out[k] = (float)(v[(size_t)k] / sum);
  return P2PHD_OK;
}

extern "C" int p2phd_limiter_envelope(const float* planar, int64_t frames, int channels, int64_t ld, const float* table_dev, int factor,
                                      int taps_per_phase, float ceiling, float* r_out, float* peak_in_out, void* stream) {
  if (const int rc = p2phd::pcm_check_rows("limiter_envelope", frames, channels, ld, P2PHD_PCM_F32, true)) return rc;
  P2PHD_REQUIRE(table_ok(factor, taps_per_phase), "limiter_envelope: factor must be 1, 2 or 4 and taps_per_phase even and in [%d, %d], got %d and %d",
                kMinTaps, kMaxTaps, factor, taps_per_phase);
  P2PHD_REQUIRE(ceiling > 0.0f && std::isfinite(ceiling), "limiter_envelope: ceiling must be finite and > 0, got %g", (double)ceiling);
  P2PHD_REQUIRE(peak_in_out && table_dev, "limiter_envelope: null output or table pointer");
  P2PHD_REQUIRE(frames == 0 || (planar && r_out), "limiter_envelope: null pointer");
  P2PHD_REQUIRE(((reinterpret_cast<uintptr_t>(planar) | reinterpret_cast<uintptr_t>(table_dev) | reinterpret_cast<uintptr_t>(r_out) |
                  reinterpret_cast<uintptr_t>(peak_in_out)) & 3) == 0, "limiter_envelope: a pointer is not aligned to a float");
  hipStream_t st = (hipStream_t)stream;
  const p2phd::FoldScratch fs = p2phd::fold_scratch(p2phd::FOLD_LIMITER, st);
  if (fs.part == nullptr) return P2PHD_EINVAL;                   // (refused: error text set by fold_scratch)
  P2PHD_REQUIRE(fs.floats >= (size_t)kEnvParts * (1 + kStatWords) && fs.tickets >= 2, "limiter_envelope: reduction scratch too small");
  // frames = 0 launches too -- one workgroup without a tile: the peak (0) is valid after every call
  const int64_t tiles = p2phd::cdiv(frames, (int64_t)kEnvStep);
  const dim3 grid(tile_grid(tiles, kEnvParts));
  uint32_t* part = reinterpret_cast<uint32_t*>(fs.part);
  const auto kernel = factor == 4 ? limiter_envelope_kernel<3> : factor == 2 ? limiter_envelope_kernel<1> : limiter_envelope_kernel<0>;
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, planar, (long)ld, (long)frames, channels, table_dev, taps_per_phase, (long)tiles, ceiling,
                     r_out, part, fs.ticket, peak_in_out);
  if (frames > 0) ++p2phd::g_launch_count[p2phd::LC_LIMITER];
  return p2phd::check_launch("limiter_envelope");
}

extern "C" int p2phd_limiter_apply(const float* planar, int64_t frames, int channels, int64_t ld, const float* r, int lookahead, int hold,
                                   const float* window_dev, float* out, int64_t out_ld, float* g_out, void* stats_out, void* stream) {
  if (const int rc = p2phd::pcm_check_rows("limiter_apply", frames, channels, ld, P2PHD_PCM_F32, true)) return rc;
  P2PHD_REQUIRE(lookahead >= 1 && lookahead <= kMaxLookahead && hold >= 0 && hold <= kMaxHold,
                "limiter_apply: lookahead must be in [1, %d] and hold in [0, %d], got %d and %d", kMaxLookahead, kMaxHold, lookahead, hold);
  P2PHD_REQUIRE(out_ld >= frames && out_ld <= (int64_t(1) << 44), "limiter_apply: out_ld %lld is shorter than the %lld frames of a row, or too large",
                (long long)out_ld, (long long)frames);
  P2PHD_REQUIRE(stats_out && window_dev, "limiter_apply: null statistics or window pointer");
  P2PHD_REQUIRE(frames == 0 || (planar && r && out), "limiter_apply: null pointer");
  P2PHD_REQUIRE(((reinterpret_cast<uintptr_t>(planar) | reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(window_dev) |
                  reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(g_out) | reinterpret_cast<uintptr_t>(stats_out)) & 3) == 0,
                "limiter_apply: a pointer is not aligned to a float");
  P2PHD_REQUIRE(frames == 0 || !spans_overlap(out, out_ld, planar, ld, channels, frames), "limiter_apply: out overlaps the clip (it is written to a buffer of its own)");
  hipStream_t st = (hipStream_t)stream;
  const p2phd::FoldScratch fs = p2phd::fold_scratch(p2phd::FOLD_LIMITER, st);
  if (fs.part == nullptr) return P2PHD_EINVAL;                   // (refused: error text set by fold_scratch)
  P2PHD_REQUIRE(fs.floats >= (size_t)kEnvParts * (1 + kStatWords) && fs.tickets >= 2, "limiter_apply: reduction scratch too small");
  // frames = 0 launches too -- one workgroup without a tile: the statistics (1 and 0) are valid after every call
  const int64_t tiles = p2phd::cdiv(frames, (int64_t)kTile);
  const dim3 grid(tile_grid(tiles, kEnvParts));
  const int n_r = kTile + 2 * lookahead + hold;
  const size_t lds = ((size_t)n_r + lds_floats(n_r)) * sizeof(float);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(limiter_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  uint32_t* part = reinterpret_cast<uint32_t*>(fs.part) + kEnvParts;
  hipLaunchKernelGGL(limiter_apply_kernel, grid, dim3(kThreads), lds, st, planar, (long)ld, (long)frames, channels, r, lookahead, hold, window_dev,
                     (long)tiles, out, (long)out_ld, g_out, part, fs.ticket + 1, reinterpret_cast<uint32_t*>(stats_out));
  if (frames > 0) ++p2phd::g_launch_count[p2phd::LC_LIMITER];
  return p2phd::check_launch("limiter_apply");
}
