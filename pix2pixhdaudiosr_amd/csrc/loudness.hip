// Whole-file generation (pix2pixhdaudiosr_amd/generate/): integrated loudness after ITU-R BS.1770-4 / EBU R 128, the gain
// that brings a clip to a wanted level, and the loudness range after EBU Tech 3342.  Launch family "loudness".
//
//   coeffs_fill (host) the K-weighting pair for a sampling rate, float64: the high shelf, then the high-pass (b0 b1 b2 a1 a2 each).
//   hops        z[c][j] = sum over hop j (rate / 10 samples, 100 ms) of y^2, y = row c through shelf and high-pass.
//   gate        400 ms blocks of four hops at 75 % overlap, the channel weights, the absolute gate at -70 LUFS, the relative gate
//               10 LU under the ungated mean -> {I, the loudest block, the relative threshold, blocks kept} and the gain to a target.
//   blocks      p[b] = the channel-weighted power of 400 ms block b of one clip, the gate's own expression, written where the caller
//               points: a slice of a buffer that holds the blocks of every file of a folder.
//   gate_blocks the gate over such a buffer -- the folder as one programme (EBU R 128 album loudness).  The same body as `gate`,
//               so for the blocks of one file it returns the bits `gate` returns for that file's z.  One workgroup on purpose: a
//               grid-wide sum would need another summation order.
//   short_term  p[b] = the power of the 3 s block of 30 hops that starts at hop b (100 ms step), the channels weighted, times the
//               square of a gain read from device memory where one is given.  Every block sums its own 30 hops left to right: no
//               running sum, so p[b] does not depend on where the block lies.
//   range       p -> the loudness range: the absolute gate at -70 LUFS, the relative gate 20 LU under the mean of what passed, the
//               10th and 95th percentile of what is left -> {LRA, both levels, the threshold, blocks kept, the loudest block, both
//               selected powers}.  The percentiles are exact order statistics: a power behind the gates is positive, so it orders
//               as its bit pattern read as an unsigned integer, and an MSB-first radix select -- eight passes over p, a 256-bin
//               histogram of integer counts in LDS per wanted rank, a scan, a descent into the bin that holds the rank -- ends with
//               the 64 bits of the wanted element.  Counts are integers (no float atomics), so the order in which the adds land does
//               not show; the gates are re-evaluated per element from two thresholds, so there is no compacted copy and no
//               workspace, and p is only read.
//
// The recursion made parallel: zero-state warm-up.  The work item of hop j starts from zero state at sample (j - 2) hop -- 200 ms in
// front of its hop -- or at sample 0 where that is nearer (hops 0 .. 2 are the sequential recursion itself), runs both biquads
// through the warm-up without counting and sums y^2 over its own hop alone.  What it lacks is the response of the state the
// sequential filter holds at (j - 2) hop, which decays with the slowest pole: the high-pass has a double pole at radius
// r = 1 - 2 pi 38.1 / rate (0.995 at 48 kHz), so after 200 ms the state's response is down by about n r^n, n = rate / 5:
// e^-48 = 1.4e-21 times 9600 at 48 kHz and the same in time at every rate -- far below the float64 rounding of the recursion
// itself (2^-53 / (1 - r)^2 = 4e-12).  Samples in front of sample 0 are fed as zeros, which leaves a zero state exactly zero, so
// every work item walks the same 3 hop samples and the loop bounds are uniform.
//
// One wave per workgroup, lane = hop, blockIdx.y = row: 64 neighbouring hops of one row.  Lane r needs the samples from
// (j0 + r - 2) hop on -- a stride of hop floats across the lanes -- so the wave stages them through LDS: a load instruction takes
// 32 consecutive floats of two tile rows, one per half wave (two coalesced 128-byte requests), the tile is [64 hops][32 samples]
// with a row pitch of 33 floats (lane r then reads bank (r + k) mod 32: conflict-free), and the next tile's 32 requests are in
// flight, in registers, while the wave runs the recursion over the current one.  State and sums are float64 (an fp32 recursion leaves up to
// 1.5 % in the energy of a quiet hop behind a loud one); transposed direct form II, every product-sum one explicit fma, nothing
// else contracted, so the bits do not depend on the grid, the number of rows or the alignment of a row.  No atomics, no
// workspace, nothing that depends on scheduling: z[c][j] has one writer.
#include "common.h"
#include "convplan.h"
#include "streamgrid.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {
constexpr int kLanes = 64;                    // hops per workgroup = lanes of its one wave
constexpr int kChunk = 32;                    // samples per staged tile row: half a wave loads one
constexpr int kPitch = kChunk + 1;
constexpr int kWarmHops = 2;                  // 200 ms of warm-up
constexpr int kGateThreads = 256;
constexpr int kMaxGateChannels = 64;

struct KWeight { double b0, b1, b2, a1, a2, ha1, ha2; };      // shelf; high-pass (its b is 1, -2, 1)

// b0 b1 b2 a1 a2 of the shelf, then of the high-pass, for `rate`
void k_weighting(double rate, double* out10) {
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = std::tan(pi * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    out10[0] = (Vh + Vb * K / Q + K * K) / a0;
    out10[1] = 2.0 * (K * K - Vh) / a0;
    out10[2] = (Vh - Vb * K / Q + K * K) / a0;
    out10[3] = 2.0 * (K * K - 1.0) / a0;
    out10[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = std::tan(pi * f0 / rate);
    const double a0 = 1.0 + K / Q + K * K;
    out10[5] = 1.0;
    out10[6] = -2.0;
    out10[7] = 1.0;
    out10[8] = 2.0 * (K * K - 1.0) / a0;
    out10[9] = (1.0 - K / Q + K * K) / a0;
  }
}

bool rate_ok(double rate) { return rate >= 8000.0 && rate <= 384000.0 && std::floor(rate) == rate && std::fmod(rate, 10.0) == 0.0; }

// one sample through both biquads (transposed direct form II); COUNT: its square joins the hop's sum
template <bool COUNT>
__device__ __forceinline__ void k_step(const KWeight& k, float xf, double& s1, double& s2, double& t1, double& t2, double& acc) {
  const double x = (double)xf;
  const double y1 = __builtin_fma(k.b0, x, s1);
  s1 = __builtin_fma(-k.a1, y1, __builtin_fma(k.b1, x, s2));
  s2 = __builtin_fma(-k.a2, y1, k.b2 * x);
  const double y2 = y1 + t1;
  t1 = __builtin_fma(-k.ha1, y2, __builtin_fma(-2.0, y1, t2));
  t2 = __builtin_fma(-k.ha2, y2, y1);
  if (COUNT) acc = __builtin_fma(y2, y2, acc);
}

// grid (ceil(J / 64), channels), one wave.  Lane r is hop j = 64 blockIdx.x + r; at local time tau in [0, 3 hop) it takes sample
// (j - 2) hop + tau of its row (zero in front of sample 0), counting from tau = 2 hop.  The last sample read is (j + 1) hop - 1 <
// J hop <= frames; lanes with j >= J walk a copy of the last hop's samples and write nothing.
__global__ __launch_bounds__(kLanes) void loudness_hops_kernel(const float* __restrict__ planar, long ld, long hop, long J, KWeight k,
                                                               double* __restrict__ z) {
  __shared__ float s_x[kLanes * kPitch];
  const int lane = threadIdx.x;
  const long j0 = (long)blockIdx.x * kLanes;
  const float* row = planar + (long)blockIdx.y * ld;
  const long warm = kWarmHops * hop, span = warm + hop;
  const long first = (j0 - kWarmHops) * hop;                      // sample of tile row 0 at tau = 0 (may be negative)
  const int rows = (int)min((long)kLanes, J - j0);                // hops of this workgroup, >= 1
  const int half = lane >> 5, col = lane & (kChunk - 1);          // this lane loads column `col` of the tile rows 2 u + half
  float pre[kLanes / 2];
  double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, acc = 0.0;

  // every address is clamped into what the workgroup may read (a row past `rows` repeats the last one, whose lane writes nothing;
  // a column past `span` repeats the last sample, which is not walked); a sample in front of sample 0 is a zero
#define P2PHD_LOUDNESS_FETCH(T0)                                                               \
  {                                                                                            \
    const long tau = min((T0) + col, span - 1);                                                \
    _Pragma("unroll") for (int u = 0; u < kLanes / 2; ++u) {                                   \
      const long idx = first + (long)min(2 * u + half, rows - 1) * hop + tau;                  \
      const float v = row[max(idx, 0L)];                                                       \
      pre[u] = idx >= 0 ? v : 0.0f;                                                            \
    }                                                                                          \
  }

  P2PHD_LOUDNESS_FETCH(0)
  for (long t0 = 0; t0 < span; t0 += kChunk) {
    __syncthreads();                                              // the tile of the step before has been read
#pragma unroll
    for (int u = 0; u < kLanes / 2; ++u) s_x[(2 * u + half) * kPitch + col] = pre[u];
    __syncthreads();
    if (t0 + kChunk < span) P2PHD_LOUDNESS_FETCH(t0 + kChunk)      // in flight while the recursion runs
    const float* mine = s_x + lane * kPitch;
    if (t0 + kChunk <= warm) {
#pragma unroll
      for (int i = 0; i < kChunk; ++i) k_step<false>(k, mine[i], s1, s2, t1, t2, acc);
    } else if (t0 >= warm && t0 + kChunk <= span) {
#pragma unroll
      for (int i = 0; i < kChunk; ++i) k_step<true>(k, mine[i], s1, s2, t1, t2, acc);
    } else {                                                      // the tile with the first counted sample, and the last one
      const int n = (int)min((long)kChunk, span - t0);
      for (int i = 0; i < n; ++i) {
        if (t0 + i >= warm) k_step<true>(k, mine[i], s1, s2, t1, t2, acc);
        else k_step<false>(k, mine[i], s1, s2, t1, t2, acc);
      }
    }
  }
#undef P2PHD_LOUDNESS_FETCH
  if (lane < rows) z[(long)blockIdx.y * J + j0 + lane] = acc;
}

struct GateWeights { float w[kMaxGateChannels]; };

__device__ __forceinline__ double lufs(double p) { return -0.691 + 10.0 * log10(p); }

// mean square of block b over its four hops, the channels weighted
__device__ __forceinline__ double block_power(const double* __restrict__ z, long J, int C, const GateWeights& gw, double norm, long b) {
  double p = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* zc = z + (long)c * J + b;
    const double P = (((zc[0] + zc[1]) + zc[2]) + zc[3]) / norm;
    p = p + (double)gw.w[c] * P;
  }
  return p;
}

// fixed-order sum of one double and one count per thread over the workgroup; every thread gets the totals
__device__ __forceinline__ void gate_fold(double* s_sum, long* s_cnt, double& sum, long& cnt) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_sum[tid] = sum; s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = kGateThreads / 2; o > 0; o >>= 1) {
    if (tid < o) { s_sum[tid] = s_sum[tid] + s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
    __syncthreads();
  }
  sum = s_sum[0]; cnt = s_cnt[0];
}

// The two places a 400 ms block's power comes from: the hop energies of one clip (computed where it is needed), or a buffer of
// powers that loudness_blocks_kernel has filled.  block_power is the same function in both, so the bits are too.
struct HopBlocks {
  const double* __restrict__ z; long J; int C; double norm; const GateWeights& gw;
  __device__ __forceinline__ double operator()(long b) const { return block_power(z, J, C, gw, norm, b); }
};
struct StoredBlocks {
  const double* __restrict__ p;
  __device__ __forceinline__ double operator()(long b) const { return p[b]; }
};

// The gate, whichever way the powers come.  One workgroup.  Thread t takes the blocks t, t + 256, .. in ascending order, the
// partial sums meet in a fixed tree.  A block whose level is NaN passes both gates (the comparisons are "not at or below"), so a
// NaN in z reaches I instead of being gated out.
template <class Blocks>
__device__ __forceinline__ void gate_body(const Blocks& power, long NB, double target, const double* __restrict__ target_dev, double max_gain_db,
                                          double* __restrict__ res4, float* __restrict__ gain) {
  __shared__ double s_sum[kGateThreads];
  __shared__ long s_cnt[kGateThreads];
  __shared__ double s_max[kGateThreads];
  const int tid = threadIdx.x;
  const double ninf = -__builtin_inf();
  double sum = 0.0, top = ninf;
  long cnt = 0;
  for (long b = tid; b < NB; b += kGateThreads) {
    const double p = power(b), l = lufs(p);
    top = fmax(top, l);                                           // (a NaN never wins)
    if (!(l <= -70.0)) { sum = sum + p; ++cnt; }
  }
  s_max[tid] = top;
  gate_fold(s_sum, s_cnt, sum, cnt);
  for (int o = kGateThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_max[tid] = fmax(s_max[tid], s_max[tid + o]);
    __syncthreads();
  }
  top = s_max[0];
  const double gamma = cnt > 0 ? lufs(sum / (double)cnt) - 10.0 : ninf;
  sum = 0.0; cnt = 0;
  for (long b = tid; b < NB; b += kGateThreads) {
    const double p = power(b), l = lufs(p);
    if (!(l <= -70.0) && !(l <= gamma)) { sum = sum + p; ++cnt; }
  }
  gate_fold(s_sum, s_cnt, sum, cnt);
  if (tid == 0) {
    const double I = cnt > 0 ? lufs(sum / (double)cnt) : ninf;
    res4[0] = I; res4[1] = top; res4[2] = gamma; res4[3] = (double)cnt;
    const double T = target_dev ? *target_dev : target;
    float g = 1.0f;
    if (isfinite(T) && isfinite(I)) g = (float)pow(10.0, fmin(fmax(T - I, -max_gain_db), max_gain_db) / 20.0);
    gain[0] = g;
  }
}

__global__ __launch_bounds__(kGateThreads) void loudness_gate_kernel(const double* __restrict__ z, long J, int C, double norm, GateWeights gw,
                                                                     double target, const double* __restrict__ target_dev, double max_gain_db,
                                                                     double* __restrict__ res4, float* __restrict__ gain) {
  gate_body(HopBlocks{z, J, C, norm, gw}, J > 3 ? J - 3 : 0, target, target_dev, max_gain_db, res4, gain);
}

// the gate over powers that are already there: the blocks of a whole folder, every file's behind the other's
__global__ __launch_bounds__(kGateThreads) void loudness_gate_blocks_kernel(const double* __restrict__ p, long NB, double target,
                                                                            const double* __restrict__ target_dev, double max_gain_db,
                                                                            double* __restrict__ res4, float* __restrict__ gain) {
  gate_body(StoredBlocks{p}, NB, target, target_dev, max_gain_db, res4, gain);
}

constexpr int kBlocksThreads = 256;
constexpr int kBlocksMaxGrid = 2048;          // workgroups at most; the blocks beyond are walked with the grid's stride

// grid-stride over the 400 ms blocks of one clip, one thread per block: p[b] = block_power(b), the gate's own expression.
// Neighbouring threads read neighbouring hops, so every load of a wave is one contiguous run; p[b] has one writer.
__global__ __launch_bounds__(kBlocksThreads) void loudness_blocks_kernel(const double* __restrict__ z, long J, int C, double norm, GateWeights gw,
                                                                         double* __restrict__ p) {
  const long NB = J - 3;
  for (long b = (long)blockIdx.x * kBlocksThreads + threadIdx.x; b < NB; b += (long)gridDim.x * kBlocksThreads)
    p[b] = block_power(z, J, C, gw, norm, b);
}

constexpr int kShortHops = 30;                // hops of a short-term block: 3 s
constexpr int kShortThreads = 256;
constexpr int kShortMaxGrid = 2048;           // workgroups at most; the blocks beyond are walked with the grid's stride
static_assert(kBlocksThreads == 256 && kShortThreads == 256 && kBlocksMaxGrid == 2048 && kShortMaxGrid == 2048, "streamgrid.h, SG_LOUDNESS");
constexpr int kRadixBins = 256;               // 8 bits per pass, eight passes over the 64 bits of a double
constexpr double kAbsGatePower = 1.1724653045822981e-07;       // 10^((-70 + 0.691) / 10): the power of -70 LUFS
static_assert(kRadixBins == kGateThreads, "the range kernel gives every thread one bin of the histogram");

// grid-stride over the short-term blocks, one thread per block: p[b] = sum_c w[c] (z[c][b] + .. + z[c][b + 29]) / norm, times
// g^2 where gain_dev is given.  Neighbouring threads read neighbouring hops, so every load of a wave is one contiguous run.
__global__ __launch_bounds__(kShortThreads) void loudness_short_term_kernel(const double* __restrict__ z, long J, int C, double norm, GateWeights gw,
                                                                            const float* __restrict__ gain_dev, double* __restrict__ p) {
  const long NS = J - (kShortHops - 1);
  double gg = 1.0;
  if (gain_dev) { const double g = (double)gain_dev[0]; gg = g * g; }
  for (long b = (long)blockIdx.x * kShortThreads + threadIdx.x; b < NS; b += (long)gridDim.x * kShortThreads) {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
      const double* zc = z + (long)c * J + b;
      double S = zc[0] + zc[1];
#pragma unroll
      for (int i = 2; i < kShortHops; ++i) S = S + zc[i];
      acc = acc + (double)gw.w[c] * (S / norm);
    }
    if (gain_dev) acc = acc * gg;
    p[b] = acc;
  }
}

// One workgroup of 256 threads.  Pass 0: the loudest block, whether a power is NaN, and the mean of the powers over the absolute
// gate (thread t takes the blocks t, t + 256, .. in ascending order, the partial sums meet in gate_fold's tree).  Then the radix
// select: in pass d every thread walks its blocks again, keeps those behind both gates whose top 8 d bits are the prefix found so
// far and counts the next 8 bits into the histogram -- one histogram while both ranks share a prefix, two from where they part.
// An inclusive scan over the 256 bins (eight doubling steps in LDS) gives every thread the ranks its bin holds; the one thread
// whose bin holds the wanted rank publishes the bin and the rank within it.  Pass 0 also counts n, from which both ranks come.
__global__ __launch_bounds__(kGateThreads) void loudness_range_kernel(const double* __restrict__ p, long NS, double* __restrict__ res8) {
  __shared__ double s_sum[kGateThreads];
  __shared__ long s_cnt[kGateThreads];
  __shared__ double s_max[kGateThreads];
  __shared__ unsigned long long s_hist[2][kRadixBins];
  __shared__ unsigned long long s_scan[2][2][kRadixBins];
  __shared__ unsigned long long s_pick[2][2];                     // per rank: the bin, the rank within the bin
  const int tid = threadIdx.x;
  const double ninf = -__builtin_inf(), nan = __builtin_nan("");
  double sum = 0.0, top = 0.0;
  long cnt = 0, bad = 0;
  for (long b = tid; b < NS; b += kGateThreads) {
    const double v = p[b];
    top = fmax(top, v);                                           // (a NaN never wins)
    if (v != v) ++bad;
    if (v > kAbsGatePower) { sum = sum + v; ++cnt; }
  }
  s_max[tid] = top;
  gate_fold(s_sum, s_cnt, sum, cnt);
  for (int o = kGateThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s_max[tid] = fmax(s_max[tid], s_max[tid + o]);
    __syncthreads();
  }
  top = s_max[0];
  double none = 0.0;
  gate_fold(s_sum, s_cnt, none, bad);
  // a power at or under a threshold is gated out; nothing is over +inf
  const double rel = cnt > 0 ? 0.01 * (sum / (double)cnt) : __builtin_inf();

  unsigned long long pre[2] = {0ull, 0ull}, rank[2] = {0ull, 0ull}, n = 0ull;
  for (int d = 0; d < 8; ++d) {
    const int shift = 56 - 8 * d;
    const bool split = pre[0] != pre[1];
    s_hist[0][tid] = 0ull; s_hist[1][tid] = 0ull;
    __syncthreads();
    for (long b = tid; b < NS; b += kGateThreads) {
      const double v = p[b];
      if (v > kAbsGatePower && v > rel) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
        const unsigned long long head = d == 0 ? 0ull : bits >> (shift + 8);
        const int bin = (int)((bits >> shift) & (kRadixBins - 1));
        if (head == pre[0]) atomicAdd(&s_hist[0][bin], 1ull);
        if (split && head == pre[1]) atomicAdd(&s_hist[1][bin], 1ull);
      }
    }
    __syncthreads();
    const unsigned long long h0 = s_hist[0][tid], h1 = split ? s_hist[1][tid] : h0;
    s_scan[0][0][tid] = h0; s_scan[1][0][tid] = h1;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < kRadixBins; o <<= 1) {                     // eight steps: the result is in buffer 0 again
      const unsigned long long a0 = s_scan[0][cur][tid] + (tid >= o ? s_scan[0][cur][tid - o] : 0ull);
      const unsigned long long a1 = s_scan[1][cur][tid] + (tid >= o ? s_scan[1][cur][tid - o] : 0ull);
      s_scan[0][cur ^ 1][tid] = a0; s_scan[1][cur ^ 1][tid] = a1;
      __syncthreads();
      cur ^= 1;
    }
    if (d == 0) {
      n = s_scan[0][cur][kRadixBins - 1];
      if (n > 0) { rank[0] = ((n - 1) * 10 + 50) / 100; rank[1] = ((n - 1) * 95 + 50) / 100; }
    }
    if (n == 0 || bad > 0) break;                                 // (the same for every thread)
    const unsigned long long i0 = s_scan[0][cur][tid], i1 = s_scan[1][cur][tid];
    if (h0 > 0 && i0 - h0 <= rank[0] && rank[0] < i0) { s_pick[0][0] = (unsigned long long)tid; s_pick[0][1] = rank[0] - (i0 - h0); }
    if (h1 > 0 && i1 - h1 <= rank[1] && rank[1] < i1) { s_pick[1][0] = (unsigned long long)tid; s_pick[1][1] = rank[1] - (i1 - h1); }
    __syncthreads();
    pre[0] = (pre[0] << 8) | s_pick[0][0]; rank[0] = s_pick[0][1];
    pre[1] = (pre[1] << 8) | s_pick[1][0]; rank[1] = s_pick[1][1];
  }
  if (tid == 0) {
    double lra = 0.0, low = ninf, high = ninf, qlo = 0.0, qhi = 0.0;
    if (bad > 0) {
      lra = low = high = qlo = qhi = nan;
    } else if (n > 0) {
      qlo = __longlong_as_double((long long)pre[0]); qhi = __longlong_as_double((long long)pre[1]);
      low = lufs(qlo); high = lufs(qhi);
      lra = high - low;
    }
    res8[0] = lra; res8[1] = low; res8[2] = high; res8[3] = cnt > 0 ? lufs(rel) : ninf;
    res8[4] = (double)n; res8[5] = lufs(top); res8[6] = qlo; res8[7] = qhi;
  }
}

// the checks the gate and the short-term entry share
int gate_weights_fill(const char* who, int channels, const float* weights, GateWeights& gw) {
  for (int c = 0; c < kMaxGateChannels; ++c) gw.w[c] = 0.0f;
  for (int c = 0; c < channels; ++c) {
    gw.w[c] = weights ? weights[c] : 1.0f;
    P2PHD_REQUIRE(std::isfinite(gw.w[c]) && gw.w[c] >= 0.0f, "%s: weight %d must be finite and >= 0, got %g", who, c, (double)gw.w[c]);
  }
  return P2PHD_OK;
}

}  // namespace

extern "C" int p2phd_loudness_coeffs_fill(double rate, double* out10) {
  P2PHD_REQUIRE(rate_ok(rate), "loudness_coeffs_fill: rate must be a multiple of 10 in [8000, 384000] Hz (a hop is rate / 10 samples), got %g", rate);
  P2PHD_REQUIRE(out10 != nullptr, "loudness_coeffs_fill: null output");
  k_weighting(rate, out10);
  return P2PHD_OK;
}

extern "C" int p2phd_loudness_hops(const float* planar, int64_t frames, int channels, int64_t ld, int rate, double* z, void* stream) {
  if (const int rc = p2phd::pcm_check_rows("loudness_hops", frames, channels, ld, P2PHD_PCM_F32, true)) return rc;
  P2PHD_REQUIRE(rate_ok((double)rate), "loudness_hops: rate must be a multiple of 10 in [8000, 384000] Hz (a hop is rate / 10 samples), got %d", rate);
  const int64_t hop = rate / 10, J = frames / hop;
  if (J == 0) return P2PHD_OK;
  P2PHD_REQUIRE(planar && z, "loudness_hops: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(planar) & 3) == 0 && (reinterpret_cast<uintptr_t>(z) & 7) == 0,
                "loudness_hops: planar is not aligned to a float or z not to a double");
  double c[10];
  k_weighting((double)rate, c);
  const KWeight k{c[0], c[1], c[2], c[3], c[4], c[8], c[9]};
  const dim3 grid((unsigned)p2phd::cdiv(J, kLanes), (unsigned)channels);
  hipLaunchKernelGGL(loudness_hops_kernel, grid, dim3(kLanes), 0, (hipStream_t)stream, planar, (long)ld, (long)hop, (long)J, k, z);
  ++p2phd::g_launch_count[p2phd::LC_LOUDNESS];
  return p2phd::check_launch("loudness_hops");
}

extern "C" int p2phd_loudness_gate(const double* z, int64_t J, int channels, int rate, const float* weights, double target, const double* target_dev,
                                   double max_gain_db, double* res4, float* gain, void* stream) {
  P2PHD_REQUIRE(J >= 0 && J <= (int64_t(1) << 40) && channels >= 1 && channels <= kMaxGateChannels,
                "loudness_gate: need J >= 0 and 1 <= channels <= %d (J %lld, channels %d)", kMaxGateChannels, (long long)J, channels);
  P2PHD_REQUIRE(rate_ok((double)rate), "loudness_gate: rate must be a multiple of 10 in [8000, 384000] Hz (a hop is rate / 10 samples), got %d", rate);
  P2PHD_REQUIRE(max_gain_db >= 0.0 && std::isfinite(max_gain_db), "loudness_gate: max_gain_db must be finite and >= 0, got %g", max_gain_db);
  P2PHD_REQUIRE(res4 && gain && (z || J < 4), "loudness_gate: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(z) & 7) == 0 && (reinterpret_cast<uintptr_t>(target_dev) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(res4) & 7) == 0 && (reinterpret_cast<uintptr_t>(gain) & 3) == 0,
                "loudness_gate: a pointer is not aligned to its type");
  GateWeights gw;
  if (const int rc = gate_weights_fill("loudness_gate", channels, weights, gw)) return rc;
  // every call launches: res4 and gain are valid after it whatever J is
  hipLaunchKernelGGL(loudness_gate_kernel, dim3(1), dim3(kGateThreads), 0, (hipStream_t)stream, z, (long)J, channels, 4.0 * (double)(rate / 10), gw,
                     target, target_dev, max_gain_db, res4, gain);
  ++p2phd::g_launch_count[p2phd::LC_LOUDNESS];
  return p2phd::check_launch("loudness_gate");
}

extern "C" int p2phd_loudness_short_term(const double* z, int64_t J, int channels, int rate, const float* weights, const float* gain_dev, double* p,
                                         void* stream) {
  P2PHD_REQUIRE(J >= 0 && J <= (int64_t(1) << 40) && channels >= 1 && channels <= kMaxGateChannels,
                "loudness_short_term: need J >= 0 and 1 <= channels <= %d (J %lld, channels %d)", kMaxGateChannels, (long long)J, channels);
  P2PHD_REQUIRE(rate_ok((double)rate), "loudness_short_term: rate must be a multiple of 10 in [8000, 384000] Hz (a hop is rate / 10 samples), got %d",
                rate);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(z) & 7) == 0 && (reinterpret_cast<uintptr_t>(p) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(gain_dev) & 3) == 0, "loudness_short_term: a pointer is not aligned to its type");
  GateWeights gw;
  if (const int rc = gate_weights_fill("loudness_short_term", channels, weights, gw)) return rc;
  const int64_t NS = J - (kShortHops - 1);
  if (NS <= 0) return P2PHD_OK;
  P2PHD_REQUIRE(z && p, "loudness_short_term: null pointer");
  const unsigned grid = (unsigned)p2phd::stream_grid_of(p2phd::SG_LOUDNESS, P2PHD_F32, NS, 1).used;     // (streamgrid.h)
  hipLaunchKernelGGL(loudness_short_term_kernel, dim3(grid), dim3(kShortThreads), 0, (hipStream_t)stream, z, (long)J, channels,
                     (double)kShortHops * (double)(rate / 10), gw, gain_dev, p);
  ++p2phd::g_launch_count[p2phd::LC_LOUDNESS];
  return p2phd::check_launch("loudness_short_term");
}

extern "C" int p2phd_loudness_range(const double* p, int64_t NS, double* res8, void* stream) {
  P2PHD_REQUIRE(NS >= 0 && NS <= (int64_t(1) << 40), "loudness_range: need 0 <= NS <= 2^40, got %lld", (long long)NS);
  P2PHD_REQUIRE(res8 && (p || NS == 0), "loudness_range: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(p) & 7) == 0 && (reinterpret_cast<uintptr_t>(res8) & 7) == 0,
                "loudness_range: a pointer is not aligned to a double");
  // every call launches: res8 is valid after it whatever NS is
  hipLaunchKernelGGL(loudness_range_kernel, dim3(1), dim3(kGateThreads), 0, (hipStream_t)stream, p, (long)NS, res8);
  ++p2phd::g_launch_count[p2phd::LC_LOUDNESS];
  return p2phd::check_launch("loudness_range");
}

extern "C" int p2phd_loudness_blocks(const double* z, int64_t J, int channels, int rate, const float* weights, double* p, void* stream) {
  P2PHD_REQUIRE(J >= 0 && J <= (int64_t(1) << 40) && channels >= 1 && channels <= kMaxGateChannels,
                "loudness_blocks: need J >= 0 and 1 <= channels <= %d (J %lld, channels %d)", kMaxGateChannels, (long long)J, channels);
  P2PHD_REQUIRE(rate_ok((double)rate), "loudness_blocks: rate must be a multiple of 10 in [8000, 384000] Hz (a hop is rate / 10 samples), got %d", rate);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(z) & 7) == 0 && (reinterpret_cast<uintptr_t>(p) & 7) == 0,
                "loudness_blocks: a pointer is not aligned to a double");
  GateWeights gw;
  if (const int rc = gate_weights_fill("loudness_blocks", channels, weights, gw)) return rc;
  const int64_t NB = J - 3;
  if (NB <= 0) return P2PHD_OK;
  P2PHD_REQUIRE(z && p, "loudness_blocks: null pointer");
  const unsigned grid = (unsigned)p2phd::stream_grid_of(p2phd::SG_LOUDNESS, P2PHD_F32, NB, 1).used;     // (streamgrid.h)
  hipLaunchKernelGGL(loudness_blocks_kernel, dim3(grid), dim3(kBlocksThreads), 0, (hipStream_t)stream, z, (long)J, channels,
                     4.0 * (double)(rate / 10), gw, p);
  ++p2phd::g_launch_count[p2phd::LC_LOUDNESS];
  return p2phd::check_launch("loudness_blocks");
}

extern "C" int p2phd_loudness_gate_blocks(const double* p, int64_t NB, double target, const double* target_dev, double max_gain_db, double* res4,
                                          float* gain, void* stream) {
  P2PHD_REQUIRE(NB >= 0 && NB <= (int64_t(1) << 40), "loudness_gate_blocks: need 0 <= NB <= 2^40, got %lld", (long long)NB);
  P2PHD_REQUIRE(max_gain_db >= 0.0 && std::isfinite(max_gain_db), "loudness_gate_blocks: max_gain_db must be finite and >= 0, got %g", max_gain_db);
  P2PHD_REQUIRE(res4 && gain && (p || NB == 0), "loudness_gate_blocks: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(p) & 7) == 0 && (reinterpret_cast<uintptr_t>(target_dev) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(res4) & 7) == 0 && (reinterpret_cast<uintptr_t>(gain) & 3) == 0,
                "loudness_gate_blocks: a pointer is not aligned to its type");
  // every call launches: res4 and gain are valid after it whatever NB is
  hipLaunchKernelGGL(loudness_gate_blocks_kernel, dim3(1), dim3(kGateThreads), 0, (hipStream_t)stream, p, (long)NB, target, target_dev, max_gain_db,
                     res4, gain);
  ++p2phd::g_launch_count[p2phd::LC_LOUDNESS];
  return p2phd::check_launch("loudness_gate_blocks");
}
