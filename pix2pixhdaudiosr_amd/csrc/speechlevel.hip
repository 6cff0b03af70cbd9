// Whole-file generation (pix2pixhdaudiosr_amd/generate/): the active speech level of a clip after ITU-T P.56 method B, its
// activity factor, and the gain that brings the clip to a wanted active level.  Launch family "speechlevel", three counted
// launches per clip: the envelope, the counts, the decision.  The definition -- every expression and its order -- is the
// section "Active speech level" of include/p2phd.h; this comment says how the kernels are laid out.
//
//   consts_fill (host) g, h, gL, hL, M, the lowest threshold, L and I for a sampling rate, float64.
//   envelope    three kernels behind one another on the stream, counted as one launch:
//               chunks   a lane owns one (chunk, row) chain of L = 256 samples: the two-pole envelope from (0, 0) -> (zp, zq), and the
//                        chunk's energy s.  One wave per workgroup takes 64 neighbouring chunks of a row -- a tile of 16384 samples.
//               carry    one workgroup of one wave per row walks the chunks left to right: (P, Q) at every chunk's start, in place of
//                        (zp, zq), and sq, the sum of s.  675 000 dependent steps for an hour at 48 kHz: the chunk results come and go
//                        through LDS in coalesced pieces of 512, lane 0 runs the chain over LDS.
//               index    the chunk kernel again from (P, Q): q at every sample -> m, the number of thresholds at or under q, one byte.
//   counts      tm = the trailing maximum of m over I + 1 samples, a[c][j] = the number of samples with tm > j.
//   decide      one workgroup: lane c takes row c, lane 0 then the file's figure and the gain.
//
// A lane that read its 256 consecutive floats on its own would put a stride of 1 KiB across the wave.  The wave stages time
// tiles instead, [64 chunks][64 samples]: a load instruction takes 64 consecutive floats of one chunk (a row that starts on a
// 16-byte boundary: four chunks at 16 bytes per lane), the tile has a row pitch of 65 floats (lane r then reads bank (r + i)
// mod 32: the reads, which the recursion waits for, are conflict-free; the 16-byte path's stores into the tile are not -- the 16
// lanes of a chunk stride by 4 floats, two lanes to a bank -- which costs a second pass per store instruction and no bits) and the
// next tile's loads are in flight, in registers, while the recursion runs over the current one.
// m goes back the same way: a lane packs four m into a word of a [64][17]-word tile, and the wave writes runs of 64 consecutive
// bytes (rows of m on a 4-byte boundary: four chunks at a word per lane).
//
// m is a byte and not a bit mask or q itself: the counts need nothing but the index, a byte is an eighth of q's traffic, and
// the trailing maximum of an index is the hangover of all fifteen thresholds at once (the thresholds are nested).
//
// counts kernel: a tile of 16384 samples with the I samples in front of it sits in LDS, one byte each (54784 bytes at 192 kHz).
// The trailing maximum over W = I + 1 goes in two block passes, as the sliding minimum of limiter.hip: maxima of blocks of W
// from the block's first position up to each position, and from each position up to the block's last; each pass is a
// thread-local walk over a chunk of consecutive positions, a segmented scan of the 256 chunk results and a walk that hands the
// carry on up to the chunk's first block edge.  m < 16, so both maxima share the byte: the prefix maximum takes the high
// nibble, the suffix maximum replaces m in the low one.  tm = max(suffix[q], prefix[q + I]).  The fifteen counts are wave
// ballots (integers in scalar registers), met in LDS and added to a with 64-bit integer atomics: the order does not show.
// No float atomics, no scratch, nothing waits on the host.  No roofline claim: see DESIGN.md section 6.
#include "common.h"
#include "convplan.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

// Every float64 product and sum below is written with the plain operators under this pragma and is rounded on its own.  (The
// __dmul_rn / __dadd_rn of the HIP headers are inline functions compiled under the headers' own contraction setting: inlined here,
// the compiler fused their products into the sums that follow.)
#pragma clang fp contract(off)

namespace {
constexpr int kLanes = 64;                    // chunks per workgroup = lanes of its one wave
constexpr int kChunk = 256;                   // L: samples of a chunk
constexpr int kStep = 64;                     // samples of a chunk per staged tile
constexpr int kPitch = kStep + 1;             // floats
constexpr int kMPitch = kStep / 4 + 1;        // words
constexpr int kTile = kLanes * kChunk;        // samples per workgroup tile, of both grid kernels
constexpr int kMaxGrid = 2048;                // workgroups per row at most; the tiles beyond are walked with the grid's stride
constexpr int kCarryPiece = 512;              // chunks the carry kernel holds in LDS at a time
constexpr int kCountThreads = 256;
constexpr int kThresholds = 15;
constexpr int kMaxChannels = 64;
constexpr int kMinRate = 8000, kMaxRate = 192000;

struct Consts { double g, h, gL, hL; };

bool rate_ok(int rate) { return rate >= kMinRate && rate <= kMaxRate; }
int hang_of(int rate) { return (rate + 4) / 5; }                 // I = ceil(0.2 rate)

void consts_of(int rate, double* out8) {
  const double g = std::exp(-1.0 / (0.03 * (double)rate));
  const double h = 1.0 - g;
  double gL = g;
  for (int i = 0; i < 8; ++i) gL = gL * gL;
  out8[0] = g; out8[1] = h; out8[2] = gL; out8[3] = (256.0 * h) * gL;
  out8[4] = 15.9; out8[5] = std::ldexp(1.0, -15); out8[6] = (double)kChunk; out8[7] = (double)hang_of(rate);
}

// the number of j in 0 .. 14 with q >= 2^(j - 15): q is never negative, so its exponent field answers; a NaN gives 0
__device__ __forceinline__ unsigned index_of(double q) {
  const int e = ((__double2hiint(q) >> 20) & 0x7FF) - 1023;
  const int m = min(max(e + 16, 0), kThresholds);
  return q != q ? 0u : (unsigned)m;
}

// One sample of the envelope: every operation a separate IEEE double multiply or add.
__device__ __forceinline__ void env_step(const Consts& k, float xf, double& p, double& q) {
  const double r = (double)fabsf(xf);
  const double gp = k.g * p, hr = k.h * r;
  p = gp + hr;
  const double gq = k.g * q, hp = k.h * p;
  q = gq + hp;
}

// INDEX = false: chunks -> zp, zq, s.  INDEX = true: from (P, Q) -> m.  VEC: every row of planar starts on a 16-byte boundary and
// every row of m on a 4-byte one.  grid (gx, channels), one wave: workgroup b takes the tiles b, b + gx, .. of its row; lane r of
// tile t owns chunk 64 t + r.  Every address is clamped into the row (a chunk past the last repeats the last one, a sample past
// the last repeats the last sample; neither is walked).
template <bool INDEX, bool VEC>
__global__ __launch_bounds__(kLanes) void speechlevel_chunks_kernel(const float* __restrict__ planar, long ld, long frames, long nchunks, long tiles,
                                                                    Consts k, double* __restrict__ work, uint8_t* __restrict__ m, long ld_m) {
  __shared__ float s_x[kLanes * kPitch];
  __shared__ unsigned s_m[INDEX ? kLanes * kMPitch : 1];
  const int lane = threadIdx.x;
  const float* row = planar + (long)blockIdx.y * ld;
  double* zp = work + (long)blockIdx.y * 3 * nchunks;
  double* zq = zp + nchunks;
  double* se = zq + nchunks;
  uint8_t* mrow = INDEX ? m + (long)blockIdx.y * ld_m : nullptr;
  const int vrow = lane >> 4, vcol = (lane & 15) * 4;             // VEC: this lane's chunk within a group of four, its first sample
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long k0 = tile * kLanes, base = k0 * kChunk;
    const int rows = (int)min((long)kLanes, nchunks - k0);        // chunks of this tile, >= 1
    const long mine = k0 + lane;
    const int len = lane < rows ? (int)min((long)kChunk, frames - mine * kChunk) : 0;
    double p = 0.0, q = 0.0, s = 0.0;
    if (INDEX && lane < rows) { p = zp[mine]; q = zq[mine]; }
    float pre[kStep];

#define P2PHD_SPEECHLEVEL_FETCH(T0)                                                            \
  if (VEC) {                                                                                   \
    _Pragma("unroll") for (int u = 0; u < kStep / 4; ++u) {                                    \
      const long idx = base + (long)min(4 * u + vrow, rows - 1) * kChunk + (T0) + vcol;        \
      if (idx + 4 <= frames) {                                                                 \
        const float4 v = *reinterpret_cast<const float4*>(row + idx);                          \
        pre[4 * u] = v.x; pre[4 * u + 1] = v.y; pre[4 * u + 2] = v.z; pre[4 * u + 3] = v.w;    \
      } else {                                                                                 \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) pre[4 * u + e] = row[min(idx + e, frames - 1)]; \
      }                                                                                        \
    }                                                                                          \
  } else {                                                                                     \
    _Pragma("unroll") for (int u = 0; u < kStep; ++u)                                          \
      pre[u] = row[min(base + (long)min(u, rows - 1) * kChunk + (T0) + lane, frames - 1)];     \
  }

    P2PHD_SPEECHLEVEL_FETCH(0)
    for (int t0 = 0; t0 < kChunk; t0 += kStep) {
      __syncthreads();                                            // the tiles of the step before have been read
      if (VEC) {
#pragma unroll
        for (int u = 0; u < kStep / 4; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) s_x[(4 * u + vrow) * kPitch + vcol + e] = pre[4 * u + e];
      } else {
#pragma unroll
        for (int u = 0; u < kStep; ++u) s_x[u * kPitch + lane] = pre[u];
      }
      __syncthreads();
      if (t0 + kStep < kChunk) { P2PHD_SPEECHLEVEL_FETCH(t0 + kStep) }    // in flight while the recursion runs
      const float* own = s_x + lane * kPitch;
      const int n = min(max(len - t0, 0), kStep);
      if (n == kStep) {
#pragma unroll
        for (int i = 0; i < kStep; i += 4) {
          unsigned word = 0u;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = own[i + e];
            env_step(k, x, p, q);
            if (INDEX) word |= index_of(q) << (8 * e);
            else { const double xd = (double)x, xx = xd * xd; s = s + xx; }
          }
          if (INDEX) s_m[lane * kMPitch + (i >> 2)] = word;
        }
      } else {
        for (int i = 0; i < n; i += 4) {
          unsigned word = 0u;
          for (int e = 0; e < 4 && i + e < n; ++e) {
            const float x = own[i + e];
            env_step(k, x, p, q);
            if (INDEX) word |= index_of(q) << (8 * e);
            else { const double xd = (double)x, xx = xd * xd; s = s + xx; }
          }
          if (INDEX) s_m[lane * kMPitch + (i >> 2)] = word;
        }
      }
      if (INDEX) {
        __syncthreads();
        if (VEC) {
#pragma unroll
          for (int u = 0; u < kStep / 4; ++u) {
            const int r = 4 * u + vrow;
            const long idx = base + (long)r * kChunk + t0 + vcol;
            if (r < rows && idx < frames) {
              const unsigned word = s_m[r * kMPitch + (vcol >> 2)];
              if (idx + 4 <= frames) *reinterpret_cast<unsigned*>(mrow + idx) = word;
              else for (int e = 0; e < 4 && idx + e < frames; ++e) mrow[idx + e] = (uint8_t)(word >> (8 * e));
            }
          }
        } else {
          for (int u = 0; u < rows; ++u) {
            const long idx = base + (long)u * kChunk + t0 + lane;
            if (idx < frames) mrow[idx] = (uint8_t)(s_m[u * kMPitch + (lane >> 2)] >> (8 * (lane & 3)));
          }
        }
      }
    }
#undef P2PHD_SPEECHLEVEL_FETCH
    if (!INDEX && lane < rows) { zp[mine] = p; zq[mine] = q; se[mine] = s; }
  }
}

// grid (channels), one wave.  (zp, zq) of the row's chunks become (P, Q) at the chunks' starts, in place; sq[row] = the sum of s.
// The chain is lane 0's: three dependent float64 operations a step.  What it reads and what it writes are separate LDS arrays, so
// the reads of the next steps are issued ahead of the chain and do not wait behind its stores.
__global__ __launch_bounds__(kLanes) void speechlevel_carry_kernel(double* __restrict__ work, long nchunks, Consts k, double* __restrict__ sq) {
  __shared__ double s_zp[kCarryPiece], s_zq[kCarryPiece], s_s[kCarryPiece], s_P[kCarryPiece], s_Q[kCarryPiece];
  const int lane = threadIdx.x;
  double* zp = work + (long)blockIdx.x * 3 * nchunks;
  double* zq = zp + nchunks;
  const double* se = zq + nchunks;
  double P = 0.0, Q = 0.0, sum = 0.0;                             // (lane 0's)
  for (long c0 = 0; c0 < nchunks; c0 += kCarryPiece) {
    const int n = (int)min((long)kCarryPiece, nchunks - c0);
    for (int i = lane; i < n; i += kLanes) { s_zp[i] = zp[c0 + i]; s_zq[i] = zq[c0 + i]; s_s[i] = se[c0 + i]; }
    __syncthreads();
    if (lane == 0) {
#pragma unroll 8
      for (int i = 0; i < n; ++i) {
        const double a = s_zp[i], b = s_zq[i];
        s_P[i] = P; s_Q[i] = Q;
        sum = sum + s_s[i];
        const double gq = k.gL * Q, hp = k.hL * P, gp = k.gL * P;
        Q = (gq + hp) + b;
        P = gp + a;
      }
    }
    __syncthreads();
    for (int i = lane; i < n; i += kLanes) { zp[c0 + i] = s_P[i]; zq[c0 + i] = s_Q[i]; }
    __syncthreads();                                              // (the piece is written: the arrays take the next one)
  }
  if (lane == 0) sq[blockIdx.x] = sum;
}

// Maxima of blocks of W over the n staged bytes, from the block's first position up to each position (MIRROR = false: into the
// high nibble) or from each position up to the block's last (MIRROR = true: in place of m in the low nibble, so this pass runs
// second).  The walk runs over v = 0 .. total - 1, total = the blocks' whole span, v = p or total - 1 - p: positions behind n
// count as 0.  Thread t takes the chunk v = t E .. t E + E - 1; a byte is read and written by the one thread that owns it.
template <bool MIRROR>
__device__ __forceinline__ void block_maxima(uint8_t* s_b, int n, int W, int total, int E, unsigned (*s_v)[kCountThreads], int (*s_f)[kCountThreads]) {
  const int tid = threadIdx.x;
  const int v0 = min(tid * E, total), v1 = min(v0 + E, total);
  // the thread's own chunk: a running maximum of m that starts again at every block edge
  unsigned run = 0u;
  int edge = 0, first = v1;                                       // first: the chunk's first block edge (v1: none)
  int ph = v0 % W;
  for (int v = v0; v < v1; ++v) {
    if (ph == 0) { run = 0u; if (!edge) first = v; edge = 1; }
    const int p = MIRROR ? total - 1 - v : v;
    if (p < n) {
      const unsigned b = s_b[p];
      run = max(run, b & 15u);
      s_b[p] = (uint8_t)(MIRROR ? ((b & 0xF0u) | run) : ((b & 15u) | (run << 4)));
    }
    if (++ph == W) ph = 0;
  }
  // segmented scan of the chunk results (value: the maximum since the chunk's last edge, flag: the chunk holds an edge)
  int cur = 0;
  s_v[0][tid] = run; s_f[0][tid] = edge;
  __syncthreads();
  for (int o = 1; o < kCountThreads; o <<= 1) {
    unsigned v2 = s_v[cur][tid]; int f2 = s_f[cur][tid];
    if (tid >= o) {
      const unsigned v1_ = s_v[cur][tid - o]; const int f1 = s_f[cur][tid - o];
      if (!f2) v2 = max(v1_, v2);
      f2 |= f1;
    }
    s_v[cur ^ 1][tid] = v2; s_f[cur ^ 1][tid] = f2;
    cur ^= 1;
    __syncthreads();
  }
  // what the chunks in front hand on reaches up to the chunk's first edge
  const unsigned carry = tid > 0 ? s_v[cur][tid - 1] : 0u;
  for (int v = v0; v < first; ++v) {
    const int p = MIRROR ? total - 1 - v : v;
    if (p < n) {
      const unsigned b = s_b[p];
      s_b[p] = (uint8_t)(MIRROR ? ((b & 0xF0u) | max(b & 15u, carry)) : ((b & 15u) | (max(b >> 4, carry) << 4)));
    }
  }
  __syncthreads();
}

// grid (gx, channels): workgroup b takes the tiles b, b + gx, .. of 16384 samples of its row.  Dynamic LDS: 16384 + I bytes and up to 6 of alignment.
__global__ __launch_bounds__(kCountThreads) void speechlevel_counts_kernel(const uint8_t* __restrict__ m, long ld_m, long frames, int I, long tiles,
                                                                          unsigned long long* __restrict__ a) {
  extern __shared__ uint32_t s_raw[];
  __shared__ unsigned s_v[2][kCountThreads];
  __shared__ int s_f[2][kCountThreads];
  __shared__ unsigned long long s_tot[kThresholds];
  const int tid = threadIdx.x;
  const uint8_t* row = m + (long)blockIdx.y * ld_m;
  const int W = I + 1;
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 3) == 0;
  unsigned long long cnt[kThresholds];                            // the wave's counts: every lane holds the same
#pragma unroll
  for (int j = 0; j < kThresholds; ++j) cnt[j] = 0ull;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long t0 = tile * kTile;
    const int len = (int)min((long)kTile, frames - t0);           // samples of this tile, >= 1
    const int n = len + I;                                        // position p holds sample t0 - I + p; in front of sample 0: 0
    // Position 0 sits `shift` bytes into the region, so that a sample index that is a multiple of 4 falls on an LDS word: a row of m
    // on a 4-byte boundary is then staged a word a thread; the words that reach out of [max(t0 - I, 0), t0 + len), and every word
    // of another row, go byte by byte.
    const long first = t0 - I;
    const int shift = (int)(first & 3);
    uint8_t* s_b = reinterpret_cast<uint8_t*>(s_raw) + shift;
    const long a0 = first - shift;                                // the sample index of LDS word 0: a multiple of 4, may be negative
    const int words = (shift + n + 3) >> 2;
    for (int k = tid; k < words; k += kCountThreads) {
      const long j4 = a0 + 4L * k;
      if (aligned && j4 >= first && j4 >= 0 && j4 + 4 <= t0 + len) {
        s_raw[k] = *reinterpret_cast<const uint32_t*>(row + j4) & 0x0F0F0F0Fu;
      } else {
        for (int e = 0; e < 4; ++e) {
          const long j = j4 + e;
          if (j >= first && j < t0 + len) s_b[j - first] = j >= 0 ? (uint8_t)(row[j] & 15u) : (uint8_t)0;
        }
      }
    }
    __syncthreads();
    const int total = (n + W - 1) / W * W;
    const int E = (total + kCountThreads - 1) / kCountThreads;
    block_maxima<false>(s_b, n, W, total, E, s_v, s_f);
    block_maxima<true>(s_b, n, W, total, E, s_v, s_f);
    // sample q of the tile sits at position q + I: its window starts at position q
    for (int q0 = 0; q0 < len; q0 += kCountThreads) {
      const int q = q0 + tid;
      unsigned tm = 0u;
      if (q < len) tm = max((unsigned)s_b[q] & 15u, (unsigned)s_b[q + I] >> 4);
#pragma unroll
      for (int j = 0; j < kThresholds; ++j) cnt[j] += (unsigned long long)__popcll(__ballot(tm > (unsigned)j));
    }
    __syncthreads();                                              // (the maxima are read: the region takes the next tile)
  }
  if (tid < kThresholds) s_tot[tid] = 0ull;
  __syncthreads();
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < kThresholds; ++j) atomicAdd(&s_tot[j], cnt[j]);
  }
  __syncthreads();
  if (tid < kThresholds && s_tot[tid] != 0ull) atomicAdd(a + (long)blockIdx.y * 16 + tid, s_tot[tid]);
}

struct RowFigure { double active, long_term, activity, bracket; };

// the decision of one row: sq, the fifteen counts, n frames
__device__ RowFigure decide_row(double sq, const long long* __restrict__ a, long frames) {
  const double ninf = -__builtin_inf(), M = 15.9;
  RowFigure f;
  f.long_term = 10.0 * log10(sq / (double)frames);
  if (a[0] <= 0) { f.active = ninf; f.activity = 0.0; f.bracket = -1.0; return f; }
  double A = 0.0, Ap = 0.0, Dp = 0.0;
  int j = 0, found = -1;
  for (; j < kThresholds && a[j] > 0; ++j) {
    const double Aj = 10.0 * log10(sq / (double)a[j]);
    const double Dj = Aj - 20.0 * log10(ldexp(1.0, j - 15));
    if (Dj <= M) {
      if (j == 0) A = Aj;
      else { const double t = (Dp - M) / (Dp - Dj); A = Ap + t * (Aj - Ap); }
      found = j;
      break;
    }
    Ap = Aj; Dp = Dj;
  }
  if (found < 0) { A = Ap; found = j - 1; }                        // no crossing: the last valid threshold's level
  f.active = A;
  f.activity = pow(10.0, (f.long_term - A) / 10.0);
  f.bracket = (double)found;
  return f;
}

__global__ __launch_bounds__(kLanes) void speechlevel_decide_kernel(const double* __restrict__ sq, const long long* __restrict__ a, long frames, int C,
                                                                   double target, const double* __restrict__ target_dev, double max_gain_db,
                                                                   double* __restrict__ res, float* __restrict__ gain) {
  __shared__ double s_active[kMaxChannels];
  const int tid = threadIdx.x;
  if (tid < C) {
    RowFigure f;
    if (frames > 0) f = decide_row(sq[tid], a + (long)tid * 16, frames);
    else { f.active = -__builtin_inf(); f.long_term = -__builtin_inf(); f.activity = 0.0; f.bracket = -1.0; }
    res[4 * tid] = f.active; res[4 * tid + 1] = f.long_term; res[4 * tid + 2] = f.activity; res[4 * tid + 3] = f.bracket;
    s_active[tid] = f.active;
  }
  __syncthreads();
  if (tid == 0) {
    // the channel with the highest finite level, the lowest index on a tie; none finite: the first that is not -inf, else channel 0
    int pick = -1;
    for (int c = 0; c < C; ++c)
      if (isfinite(s_active[c]) && (pick < 0 || s_active[c] > s_active[pick])) pick = c;
    if (pick < 0) {
      pick = 0;
      for (int c = 0; c < C; ++c)
        if (!(s_active[c] == -__builtin_inf())) { pick = c; break; }
    }
    const double A = res[4 * pick];
    res[4 * C] = A; res[4 * C + 1] = res[4 * pick + 1]; res[4 * C + 2] = res[4 * pick + 2]; res[4 * C + 3] = (double)pick;
    const double T = target_dev ? *target_dev : target;
    float g = 1.0f;
    if (isfinite(T) && isfinite(A)) g = (float)pow(10.0, fmin(fmax(T - A, -max_gain_db), max_gain_db) / 20.0);
    gain[0] = g;
  }
}

// workgroups per row: one per tile up to the cap (and what the "speechlevel_grid" option allows)
unsigned tile_grid(int64_t tiles) {
  int64_t cap = kMaxGrid;
  if (p2phd::g_opt_speechlevel_grid > 0) cap = std::min<int64_t>(cap, p2phd::g_opt_speechlevel_grid);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, cap));
}

int check_clip(const char* who, int64_t frames, int channels, int rate) {
  P2PHD_REQUIRE(frames >= 0 && frames <= (int64_t(1) << 40) && channels >= 1 && channels <= kMaxChannels,
                "%s: need 0 <= frames <= 2^40 and 1 <= channels <= %d (frames %lld, channels %d)", who, kMaxChannels, (long long)frames, channels);
  P2PHD_REQUIRE(rate_ok(rate), "%s: rate must be in [%d, %d] Hz, got %d", who, kMinRate, kMaxRate, rate);
  return P2PHD_OK;
}

}  // namespace

extern "C" int p2phd_speechlevel_tile_len(void) { return kTile; }

extern "C" int p2phd_speechlevel_consts_fill(int rate, double* out8, int* hang) {
  P2PHD_REQUIRE(rate_ok(rate), "speechlevel_consts_fill: rate must be in [%d, %d] Hz, got %d", kMinRate, kMaxRate, rate);
  P2PHD_REQUIRE(out8 != nullptr && hang != nullptr, "speechlevel_consts_fill: null output");
  consts_of(rate, out8);
  *hang = hang_of(rate);
  return P2PHD_OK;
}

extern "C" size_t p2phd_speechlevel_workspace_bytes(int64_t frames, int channels) {
  if (frames <= 0 || frames > (int64_t(1) << 40) || channels < 1 || channels > kMaxChannels) return 0;
  return (size_t)channels * (size_t)p2phd::cdiv(frames, (int64_t)kChunk) * 3 * sizeof(double);
}

extern "C" int p2phd_speechlevel_envelope(const float* planar, int64_t frames, int channels, int64_t ld, int rate, uint8_t* m, int64_t ld_m,
                                          double* sq, void* workspace, void* stream) {
  if (const int rc = p2phd::pcm_check_rows("speechlevel_envelope", frames, channels, ld, P2PHD_PCM_F32, true)) return rc;
  if (const int rc = check_clip("speechlevel_envelope", frames, channels, rate)) return rc;
  P2PHD_REQUIRE(ld_m >= frames && ld_m <= (int64_t(1) << 44), "speechlevel_envelope: ld_m %lld is shorter than the %lld frames of a row, or too large",
                (long long)ld_m, (long long)frames);
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(planar && m && sq && workspace, "speechlevel_envelope: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(planar) & 3) == 0 && (reinterpret_cast<uintptr_t>(sq) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "speechlevel_envelope: a pointer is not aligned to its type");
  double c[8];
  consts_of(rate, c);
  const Consts k{c[0], c[1], c[2], c[3]};
  const int64_t nchunks = p2phd::cdiv(frames, (int64_t)kChunk), tiles = p2phd::cdiv(nchunks, (int64_t)kLanes);
  const bool vec = (reinterpret_cast<uintptr_t>(planar) & 15) == 0 && (channels == 1 || (ld & 3) == 0) &&
                   (reinterpret_cast<uintptr_t>(m) & 3) == 0 && (channels == 1 || (ld_m & 3) == 0);
  const dim3 grid(tile_grid(tiles), (unsigned)channels);
  hipStream_t st = (hipStream_t)stream;
  double* work = reinterpret_cast<double*>(workspace);
  if (vec) hipLaunchKernelGGL((speechlevel_chunks_kernel<false, true>), grid, dim3(kLanes), 0, st, planar, (long)ld, (long)frames, (long)nchunks, (long)tiles, k, work, (uint8_t*)nullptr, 0L);
  else hipLaunchKernelGGL((speechlevel_chunks_kernel<false, false>), grid, dim3(kLanes), 0, st, planar, (long)ld, (long)frames, (long)nchunks, (long)tiles, k, work, (uint8_t*)nullptr, 0L);
  hipLaunchKernelGGL(speechlevel_carry_kernel, dim3((unsigned)channels), dim3(kLanes), 0, st, work, (long)nchunks, k, sq);
  if (vec) hipLaunchKernelGGL((speechlevel_chunks_kernel<true, true>), grid, dim3(kLanes), 0, st, planar, (long)ld, (long)frames, (long)nchunks, (long)tiles, k, work, m, (long)ld_m);
  else hipLaunchKernelGGL((speechlevel_chunks_kernel<true, false>), grid, dim3(kLanes), 0, st, planar, (long)ld, (long)frames, (long)nchunks, (long)tiles, k, work, m, (long)ld_m);
  ++p2phd::g_launch_count[p2phd::LC_SPEECHLEVEL];
  return p2phd::check_launch("speechlevel_envelope");
}

extern "C" int p2phd_speechlevel_counts(const uint8_t* m, int64_t frames, int channels, int64_t ld_m, int rate, int64_t* a, void* stream) {
  if (const int rc = check_clip("speechlevel_counts", frames, channels, rate)) return rc;
  P2PHD_REQUIRE(ld_m >= frames && ld_m <= (int64_t(1) << 44), "speechlevel_counts: ld_m %lld is shorter than the %lld frames of a row, or too large",
                (long long)ld_m, (long long)frames);
  P2PHD_REQUIRE(a != nullptr && (m != nullptr || frames == 0), "speechlevel_counts: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(a) & 7) == 0, "speechlevel_counts: a is not aligned to an int64");
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(a, 0, (size_t)channels * 16 * sizeof(int64_t), st);
  P2PHD_REQUIRE(e == hipSuccess, "speechlevel_counts: clearing a failed: %s", hipGetErrorString(e));
  if (frames == 0) return P2PHD_OK;
  const int I = hang_of(rate);
  const int64_t tiles = p2phd::cdiv(frames, (int64_t)kTile);
  const size_t lds = ((size_t)(kTile + I) + 3 + 3) / 4 * 4;      // the tile, its halo, and up to 3 bytes in front that align it to m's words
  if (lds > 48 * 1024) {
    // once per process: the largest region any rate needs
    static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(speechlevel_counts_kernel),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (kTile + hang_of(kMaxRate) + 8) / 4 * 4);
    P2PHD_REQUIRE(raised == hipSuccess, "speechlevel_counts: %zu bytes of LDS were refused: %s", lds, hipGetErrorString(raised));
  }
  const dim3 grid(tile_grid(tiles), (unsigned)channels);
  hipLaunchKernelGGL(speechlevel_counts_kernel, grid, dim3(kCountThreads), lds, st, m, (long)ld_m, (long)frames, I, (long)tiles,
                     reinterpret_cast<unsigned long long*>(a));
  ++p2phd::g_launch_count[p2phd::LC_SPEECHLEVEL];
  return p2phd::check_launch("speechlevel_counts");
}

extern "C" int p2phd_speechlevel_decide(const double* sq, const int64_t* a, int64_t frames, int channels, double target, const double* target_dev,
                                        double max_gain_db, double* res, float* gain, void* stream) {
  P2PHD_REQUIRE(frames >= 0 && frames <= (int64_t(1) << 40) && channels >= 1 && channels <= kMaxChannels,
                "speechlevel_decide: need 0 <= frames <= 2^40 and 1 <= channels <= %d (frames %lld, channels %d)", kMaxChannels, (long long)frames, channels);
  P2PHD_REQUIRE(max_gain_db >= 0.0 && std::isfinite(max_gain_db), "speechlevel_decide: max_gain_db must be finite and >= 0, got %g", max_gain_db);
  P2PHD_REQUIRE(res && gain && ((sq && a) || frames == 0), "speechlevel_decide: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(sq) & 7) == 0 && (reinterpret_cast<uintptr_t>(a) & 7) == 0 && (reinterpret_cast<uintptr_t>(target_dev) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(res) & 7) == 0 && (reinterpret_cast<uintptr_t>(gain) & 3) == 0,
                "speechlevel_decide: a pointer is not aligned to its type");
  // every call launches: res and gain are valid after it whatever frames is
  hipLaunchKernelGGL(speechlevel_decide_kernel, dim3(1), dim3(kLanes), 0, (hipStream_t)stream, sq, reinterpret_cast<const long long*>(a), (long)frames,
                     channels, target, target_dev, max_gain_db, res, gain);
  if (frames > 0) ++p2phd::g_launch_count[p2phd::LC_SPEECHLEVEL];
  return p2phd::check_launch("speechlevel_decide");
}
