// Whole-file generation (pix2pixhdaudiosr_amd/generate/): the rate converter of the output stage (--output_rate) -- a rational
// polyphase FIR from the model's rate to the rate that is written.  Launch family "rateconv".  (The feeder's resampler,
// resample.hip, restates the reference's training-time torchaudio resample and stays what the model was trained on; this one is
// the delivery-grade converter: a Kaiser-windowed sinc planned for a stated passband and attenuation.)
//
//   g = gcd(in, out), o = in / g, n = out / g, half = P / 2 - 1
//   plan       (host) Kaiser's beta and length for a passband and an attenuation: P taps per phase, n phases.
//   taps_fill  (host) the table c[n][P], phase-major, float64, every phase with DC gain 1, rounded once to fp32.
//   fwd        x~ = the row, 0 outside [0, L) (a NaN or infinite sample is a sample like any other); output m = j n + p, p < n:
//              y[m] = sum_k c[p][k] x~[j o + (p o) div n + k - half],   m = 0 .. L_out - 1,   L_out = ceil(L n / o).
//
// Arithmetic of a y, the same whatever the grid, the tile or the number of rows: one fp32 accumulator that starts at +0 and takes
// acc = fma(c[p][k], x~, acc) for k = 0, 1, .., P - 1 in that order (one rounding per tap).
//
// One workgroup per (run of G * kR blocks j, chunk of PT phases, row); a row is a channel, on blockIdx.y.  A thread owns one
// (phase p, group jg) and the kR blocks j = j0 + r G + jg: a coefficient is read once per tap and used kR times, against kR
// samples that lie G o apart.  The samples are staged in LDS as kR segments, segment r holding what the blocks j0 + r G .. j0 + r G +
// G - 1 read in this chunk of phases, P - 1 halo included and zero outside the row.  The table is staged transposed, [k][PT] with an
// odd row pitch: consecutive lanes are consecutive phases (a wave rarely spans two groups), so the coefficient reads are
// conflict-free and the sample reads advance by o / n per lane.  At 160 -> 147 that is 1 or 2: the 32 lanes of a 4-byte read span
// about 35 consecutive addresses, so a few banks are hit twice in EVERY read and it takes two LDS cycles, not one -- measured, 45 %
// of the kernel's LDS-active cycles are bank-conflict cycles (8 of its 9 reads per tap are sample reads); upsampling (o < n) has
// neighbours share an address, which broadcasts.  Where n <= 1024 one chunk holds every phase (PT = n) and G is chosen so that G n fills the workgroup's passes best
// within 1024 samples per segment; a larger n is cut into chunks with G = 1.  Where PT * P exceeds the table's share of LDS the
// taps are walked in runs of KC, the table run restaged between barriers; k still ascends, so the bits are the same.
// 160 -> 147, P = 92: PT = 147, G = 3, segments of 571 samples, 24 blocks = 3528 outputs per workgroup, 71 KiB of LDS.
// Every output is written by one thread: no atomics, no workspace, nothing zeroed before the launch.  No roofline claim: the
// inner loop is bound by its 4-byte LDS reads (kR + 1 per kR fmas), see DESIGN.md section 6.
#include "common.h"
#include "convplan.h"
#include "kaiser.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {
constexpr int kThreads = 512;
constexpr int kR = 8;                         // blocks j per thread
constexpr int kMinTaps = 4, kMaxTaps = 256;   // per phase
constexpr int kMaxTable = 1 << 20;            // n * P at most
constexpr int kMaxPT = 1024;                  // phases per chunk at most
constexpr int kSegMax = 1024;                 // samples per staged segment at most (kMaxTaps fits with room for a phase chunk)
constexpr int kItemsMax = 2048;               // (phase, group) pairs per workgroup at most
constexpr int kTabFloats = 14336;             // the staged table's share of LDS, in floats (56 KiB)

// how a (o, n, P) is tiled: see the file comment
struct Tile { int PT, chunks, G, KC, SEG, PTS; };

__host__ __device__ inline long cdivl(long a, long b) { return (a + b - 1) / b; }

Tile tile_plan(int o, int n, int P) {
  Tile t;
  // (PT - 1) o / n + P <= kSegMax with G = 1, whatever o / n is: PT >= 1 always fits since P <= kMaxTaps < kSegMax
  t.PT = (int)std::min<long>(std::min(n, kMaxPT), (long)(kSegMax - P) * n / o + 1);
  t.chunks = (int)cdivl(n, t.PT);
  const int span = (int)cdivl((long)(t.PT - 1) * o, n);           // samples the phases of a chunk spread over, at most
  t.G = 1;
  if (t.chunks == 1) {
    // the G whose G n items fill whole passes of kThreads best; of equals the largest
    const long gmax = std::min<long>(std::max(1, kItemsMax / n), (long)(kSegMax - P - span) / o + 1);
    long best_items = n, best_passes = cdivl(n, kThreads);
    for (long g = 2; g <= gmax; ++g) {
      const long items = g * n, passes = cdivl(items, kThreads);
      if (items * best_passes >= best_items * passes) { t.G = (int)g; best_items = items; best_passes = passes; }
    }
  }
  t.SEG = (t.G - 1) * o + span + P;
  t.PTS = t.PT | 1;
  t.KC = std::min(P, kTabFloats / t.PTS);
  return t;
}

size_t tile_lds_bytes(const Tile& t) { return ((size_t)kR * t.SEG + (size_t)t.PTS * t.KC) * sizeof(float); }

// taps [kc, kc + kn) of the chunk's phases, transposed: s_tab[kk * PTS + pl] = c[p0 + pl][kc + kk]
__device__ __forceinline__ void stage_table(float* s_tab, const float* __restrict__ tab, int P, int p0, int pt, int PTS, int kc, int kn) {
  for (int e = threadIdx.x; e < pt * kn; e += kThreads) {
    const int pl = e / kn, kk = e - pl * kn;
    s_tab[kk * PTS + pl] = tab[(long)(p0 + pl) * P + kc + kk];
  }
}

// grid (tiles * chunks, channels): workgroup (b, c) takes blocks j0 = (b / chunks) G kR .. and phases p0 = (b % chunks) PT .. of row c
__global__ __launch_bounds__(kThreads) void rateconv_kernel(const float* __restrict__ planar, long ld, long L, const float* __restrict__ tab, int o,
                                                            int n, int P, Tile t, float* __restrict__ out, long out_ld, long L_out) {
  extern __shared__ float s_mem[];
  float* s_x = s_mem;                                             // kR segments of t.SEG samples
  float* s_tab = s_mem + kR * t.SEG;                              // t.KC rows of t.PTS coefficients
  const int tid = threadIdx.x;
  const long tile = blockIdx.x / (unsigned)t.chunks;
  const int p0 = (int)(blockIdx.x - tile * t.chunks) * t.PT, pt = min(t.PT, n - p0);
  const long j0 = tile * (long)(t.G * kR);
  const long d0 = (long)p0 * o / n;                               // (p o) div n of the chunk's first phase
  const int half = P / 2 - 1;
  const float* row = planar + (long)blockIdx.y * ld;
  float* orow = out + (long)blockIdx.y * out_ld;
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const long g0 = (j0 + (long)r * t.G) * o + d0 - half;         // position q of segment r holds x~[g0 + q]
    for (int q = tid; q < t.SEG; q += kThreads) {
      const long i = g0 + q;
      s_x[r * t.SEG + q] = i >= 0 && i < L ? row[i] : 0.0f;
    }
  }
  const bool single = t.KC >= P;                                  // the whole table of the chunk fits: staged once
  if (single) stage_table(s_tab, tab, P, p0, pt, t.PTS, 0, P);
  __syncthreads();
  const int items = t.G * pt;
  for (int base = 0; base < items; base += kThreads) {
    const int item = base + tid;
    const bool active = item < items;
    const int jg = active ? item / pt : 0, pl = active ? item - jg * pt : 0;
    const int p = p0 + pl;
    const float* xw = s_x + jg * o + (int)((long)p * o / n - d0); // tap k of block r reads xw[r * SEG + k]
    float acc[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[r] = 0.0f;
    for (int kc = 0; kc < P; kc += t.KC) {
      const int kn = min(t.KC, P - kc);
      if (!single) {
        __syncthreads();                                          // every read of the previous run (and the staging above) is done
        stage_table(s_tab, tab, P, p0, pt, t.PTS, kc, kn);
        __syncthreads();
      }
      if (active) {
        const float* cw = s_tab + pl;
        const float* xk = xw + kc;
#pragma unroll 4
        for (int kk = 0; kk < kn; ++kk) {
          const float ck = cw[kk * t.PTS];
#pragma unroll
          for (int r = 0; r < kR; ++r) acc[r] = __builtin_fmaf(ck, xk[r * t.SEG + kk], acc[r]);
        }
      }
    }
    if (active) {
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const long m = (j0 + (long)r * t.G + jg) * n + p;
        if (m < L_out) orow[m] = acc[r];                          // blocks behind the row's last output do not count
      }
    }
  }
}

long gcdl(long a, long b) {
  while (b) { const long c = a % b; a = b; b = c; }
  return a;
}

bool shape_ok(int o, int n, int P) {
  return o >= 1 && n >= 1 && P >= kMinTaps && P <= kMaxTaps && (P & 1) == 0 && (long)n * P <= kMaxTable;
}

// ceil(L n / o), -1 where it does not fit
int64_t out_len(int64_t L, int64_t o, int64_t n) {
  const __int128 v = ((__int128)L * n + o - 1) / o;
  return v > ((__int128)1 << 44) ? -1 : (int64_t)v;
}

}  // namespace

extern "C" int p2phd_rateconv_plan(int in_rate, int out_rate, double passband, double atten_db, int* o, int* n, int* taps_per_phase, double* beta) {
  P2PHD_REQUIRE(in_rate >= 1 && out_rate >= 1, "rateconv_plan: rates must be >= 1 Hz, got %d and %d", in_rate, out_rate);
  P2PHD_REQUIRE(in_rate != out_rate, "rateconv_plan: nothing to convert: both rates are %d Hz", in_rate);
  P2PHD_REQUIRE(passband > 0.0 && passband < 1.0, "rateconv_plan: the passband must lie in (0, 1) of the lower Nyquist frequency, got %g", passband);
  P2PHD_REQUIRE(atten_db >= 40.0 && atten_db <= 160.0, "rateconv_plan: the attenuation must lie in [40, 160] dB, got %g", atten_db);
  P2PHD_REQUIRE(o && n && taps_per_phase && beta, "rateconv_plan: null output");
  const long g = gcdl(in_rate, out_rate);
  const double pi = 3.14159265358979323846;
  const double nyq = 0.5 * (double)std::min(in_rate, out_rate), fp = passband * nyq, fs = 2.0 * nyq - fp;
  const double half_taps = std::ceil((atten_db - 7.95) / (2.0 * 2.285 * (2.0 * pi * (fs - fp) / (double)in_rate)));
  P2PHD_REQUIRE(half_taps >= kMinTaps / 2 && half_taps <= kMaxTaps / 2,
                "rateconv_plan: %d -> %d Hz with the passband at %g and %g dB needs %.0f taps per phase, outside [%d, %d]: between these "
                "rates the filter is not built", in_rate, out_rate, passband, atten_db, 2.0 * half_taps, kMinTaps, kMaxTaps);
  const int P = 2 * (int)half_taps;
  const long nn = out_rate / g;
  P2PHD_REQUIRE(nn * P <= kMaxTable, "rateconv_plan: %d -> %d Hz needs a table of %ld phases x %d taps, more than %d coefficients: choose rates "
                "with a larger common divisor", in_rate, out_rate, nn, P, kMaxTable);
  *o = (int)(in_rate / g);
  *n = (int)nn;
  *taps_per_phase = P;
  *beta = 0.1102 * (atten_db - 8.7);
  return P2PHD_OK;
}

extern "C" int p2phd_rateconv_taps_fill(int o, int n, int taps_per_phase, double beta, double cutoff, float* out) {
  P2PHD_REQUIRE(shape_ok(o, n, taps_per_phase), "rateconv_taps_fill: need o, n >= 1, taps_per_phase even and in [%d, %d] and n * taps_per_phase <= %d, "
                "got o %d, n %d, taps_per_phase %d", kMinTaps, kMaxTaps, kMaxTable, o, n, taps_per_phase);
  P2PHD_REQUIRE(beta >= 0.0 && std::isfinite(beta), "rateconv_taps_fill: beta must be finite and >= 0, got %g", beta);
  P2PHD_REQUIRE(cutoff > 0.0 && cutoff <= 1.0, "rateconv_taps_fill: cutoff must lie in (0, 1] of the input's Nyquist frequency, got %g", cutoff);
  P2PHD_REQUIRE(out != nullptr, "rateconv_taps_fill: null output");
  const int P = taps_per_phase, half = P / 2 - 1;
  const double pi = 3.14159265358979323846, i0b = p2phd::bessel_i0(beta);
  std::vector<double> v((size_t)P);
  for (int p = 0; p < n; ++p) {
    const double frac = (double)(((long)p * o) % n) / (double)n;
    double sum = 0.0;
    for (int k = 0; k < P; ++k) {
      const double tau = (double)(k - half) - frac;
      const double y = pi * cutoff * tau, r = tau / (double)(P / 2);
      const double sinc = y == 0.0 ? 1.0 : std::sin(y) / y;
      v[(size_t)k] = cutoff * sinc * p2phd::bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
      sum += v[(size_t)k];
    }
    for (int k = 0; k < P; ++k) out[(size_t)p * P + k] = (float)(v[(size_t)k] / sum);
  }
  return P2PHD_OK;
}

extern "C" int64_t p2phd_rateconv_out_len(int64_t frames, int in_rate, int out_rate) {
  if (frames < 0 || frames > (int64_t(1) << 40) || in_rate < 1 || out_rate < 1) {
    p2phd::set_error("rateconv_out_len: need 0 <= frames <= 2^40 and rates >= 1 Hz (frames %lld, %d -> %d Hz)", (long long)frames, in_rate, out_rate);
    return -1;
  }
  const long g = gcdl(in_rate, out_rate);
  const int64_t v = out_len(frames, in_rate / g, out_rate / g);
  if (v < 0) p2phd::set_error("rateconv_out_len: %lld frames at %d -> %d Hz are too many", (long long)frames, in_rate, out_rate);
  return v;
}

extern "C" int64_t p2phd_rateconv_tile_len(int o, int n, int taps_per_phase) {
  if (!shape_ok(o, n, taps_per_phase)) {
    p2phd::set_error("rateconv_tile_len: bad o %d, n %d or taps_per_phase %d", o, n, taps_per_phase);
    return -1;
  }
  return (int64_t)tile_plan(o, n, taps_per_phase).G * kR * o;
}

extern "C" int p2phd_rateconv_fwd(const float* planar, int64_t frames, int channels, int64_t ld, const float* table_dev, int o, int n,
                                  int taps_per_phase, float* out, int64_t out_frames, int64_t out_ld, void* stream) {
  if (const int rc = p2phd::pcm_check_rows("rateconv_fwd", frames, channels, ld, P2PHD_PCM_F32, true)) return rc;
  P2PHD_REQUIRE(shape_ok(o, n, taps_per_phase), "rateconv_fwd: need o, n >= 1, taps_per_phase even and in [%d, %d] and n * taps_per_phase <= %d, got o %d, "
                "n %d, taps_per_phase %d", kMinTaps, kMaxTaps, kMaxTable, o, n, taps_per_phase);
  P2PHD_REQUIRE(o != n && gcdl(o, n) == 1, "rateconv_fwd: o and n must differ and share no divisor (in / gcd and out / gcd), got %d and %d", o, n);
  const int64_t want = out_len(frames, o, n);
  P2PHD_REQUIRE(want >= 0 && out_frames == want, "rateconv_fwd: %lld frames at %d -> %d give %lld outputs, out_frames is %lld", (long long)frames, o, n,
                (long long)want, (long long)out_frames);
  P2PHD_REQUIRE(out_ld >= out_frames && out_ld <= (int64_t(1) << 44), "rateconv_fwd: out_ld %lld is shorter than the %lld outputs of a row, or too large",
                (long long)out_ld, (long long)out_frames);
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(planar && table_dev && out, "rateconv_fwd: null pointer");
  P2PHD_REQUIRE(((reinterpret_cast<uintptr_t>(planar) | reinterpret_cast<uintptr_t>(table_dev) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
                "rateconv_fwd: a pointer is not aligned to a float");
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(planar), a1 = a0 + (uintptr_t)((channels - 1) * ld + frames) * sizeof(float);
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(out), b1 = b0 + (uintptr_t)((channels - 1) * out_ld + out_frames) * sizeof(float);
  P2PHD_REQUIRE(!(a0 < b1 && b0 < a1), "rateconv_fwd: out overlaps the input (the kernel reads a halo of other tiles: it cannot run in place)");
  const Tile t = tile_plan(o, n, taps_per_phase);
  const int64_t tiles = p2phd::cdiv(p2phd::cdiv(out_frames, (int64_t)n), (int64_t)t.G * kR);
  P2PHD_REQUIRE(tiles * t.chunks <= 0x7FFFFFFF, "rateconv_fwd: %lld workgroups per row are too many", (long long)(tiles * t.chunks));
  const size_t lds = tile_lds_bytes(t);
  static bool lds_set[64] = {};                                   // (the attribute is per device)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { p2phd::set_error("rateconv_fwd: no HIP device"); return P2PHD_ELAUNCH; }
  if (!lds_set[dev]) {
    const size_t most = ((size_t)kR * kSegMax + kTabFloats) * sizeof(float);      // above the 64 KiB a kernel gets unasked
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(rateconv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess) {
      (void)hipGetLastError();
      p2phd::set_error("rateconv_fwd: the device refuses %zu bytes of LDS per workgroup", most);
      return P2PHD_ELAUNCH;
    }
    lds_set[dev] = true;
  }
  const dim3 grid((unsigned)(tiles * t.chunks), (unsigned)channels);
  hipLaunchKernelGGL(rateconv_kernel, grid, dim3(kThreads), lds, (hipStream_t)stream, planar, (long)ld, (long)frames, table_dev, o, n, taps_per_phase, t,
                     out, (long)out_ld, (long)out_frames);
  ++p2phd::g_launch_count[p2phd::LC_RATECONV];
  return p2phd::check_launch("rateconv_fwd");
}
