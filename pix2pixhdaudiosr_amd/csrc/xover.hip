// Whole-file generation (pix2pixhdaudiosr_amd/generate/): the time-domain crossover behind the stitch.  Below the crossover
// frequency the written clip is the input, above it the generator's output:
//
//   out = sr + LP * (level * lr - sr)          LP: a centred (zero-delay) windowed-sinc low-pass of `taps` coefficients
//
//   taps_fill  (host) Kaiser-windowed sinc, float64, DC gain 1, rounded once to fp32.
//   fwd        d[j] = level * lr[j] - sr[j] inside [0, L), 0 outside (d is zero-extended, not the signals);
//              out[i] = sr[i] + sum_k h[k] d[i + c0 - k], c0 = (taps - 1) / 2.
//
// Arithmetic of an output, the same whatever the grid, the tile or the number of rows: d is one rounded product and one rounded
// subtraction (no contraction); the sum is one fp32 accumulator that starts at +0 and takes acc = fma(h[k], d, acc) for
// k = 0, 1, .., taps - 1 (the products ARE contracted: one rounding per tap); then one rounded addition sr[i] + acc.
//
// One workgroup per (tile of kTile outputs, row); a row is a channel, on blockIdx.y.  The tile's d with its taps - 1 halo is formed
// on load and staged in LDS in the padded layout of firwalk.h (256 threads, 8 CONSECUTIVE outputs a thread, one pad dword per 8
// staged: conflict-free reads).  A thread keeps the 8-wide window of d of its outputs in registers: tap k + 1 needs the window of
// tap k shifted by one sample, so a tap costs one LDS read and 8 fmas per thread; the taps are read uniformly (scalar loads).
// The sums go back through the same LDS region so that sr is read and out is written with consecutive lanes on
// consecutive floats, whatever the alignment of a row.  LDS: at most (2048 + 4094) * 9 / 8 floats = 27 KiB per workgroup.
// No atomics, no workspace.  Microseconds to a few milliseconds beside the generator: no roofline claim.
#include "common.h"
#include "convplan.h"
#include "firwalk.h"
#include "kaiser.h"
#include <cmath>
#include <cstdint>
#include <vector>

#pragma clang fp contract(off)      // d and the final addition are separately rounded; the tap products use fma explicitly

namespace {
constexpr int kThreads = 256;
constexpr int kOut = 8;                       // outputs per thread (firwalk.h)
constexpr int kTile = kThreads * kOut;        // outputs per workgroup
constexpr int kMaxTaps = 4095;

using p2phd::fir::lds_floats;
using p2phd::fir::pad8;
static_assert(kOut == 8, "pad8 is written for 8 outputs a thread");

__global__ __launch_bounds__(kThreads) void xover_kernel(const float* __restrict__ sr, long ld_sr, const float* __restrict__ lr, long ld_lr,
                                                         float level, const float* __restrict__ h, int taps, long L,
                                                         float* __restrict__ out, long ld_out) {
  extern __shared__ float s_d[];
  const int tid = threadIdx.x;
  const long tile0 = (long)blockIdx.x * kTile;
  sr += (long)blockIdx.y * ld_sr;
  lr += (long)blockIdx.y * ld_lr;
  out += (long)blockIdx.y * ld_out;
  const int len = (int)min((long)kTile, L - tile0);               // outputs of this tile, >= 1
  const int len8 = (len + kOut - 1) & ~(kOut - 1);                // ... up to whole threads: everything a thread reads is staged
  const int n = len8 + taps - 1;                                  // staged samples: position p holds d[tile0 - c0 + p]
  const long g0 = tile0 - (taps - 1) / 2;
  for (int p = tid; p < n; p += kThreads) {
    const long j = g0 + p;
    float d = 0.0f;
    if (j >= 0 && j < L) d = level * lr[j] - sr[j];
    s_d[pad8(p)] = d;
  }
  __syncthreads();
  float acc[kOut];
#pragma unroll
  for (int r = 0; r < kOut; ++r) acc[r] = 0.0f;
  const int base = tid * kOut;
  if (base < len) {
    // output r of this thread at tap k reads position base + r + (taps - 1 - k); w[r] is that sample at the current tap
    float w[kOut];
#pragma unroll
    for (int r = 0; r < kOut; ++r) w[r] = s_d[pad8(base + r + taps - 1)];
    int k = 0;
    for (; k + kOut <= taps; k += kOut) {
      // eight taps with the window rotating through the registers: at step u the sample of output r is w[(r - u) & 7]
#pragma unroll
      for (int u = 0; u < kOut; ++u) {
        const float hk = h[k + u];
#pragma unroll
        for (int r = 0; r < kOut; ++r) acc[r] = __builtin_fmaf(hk, w[(r - u) & (kOut - 1)], acc[r]);
        // the next tap: every output moves one sample down, output 0 takes a new one
        const int q = base + taps - 2 - (k + u);                  // >= base - 1 at the last tap: then it is not read
        w[(-u - 1) & (kOut - 1)] = s_d[pad8(max(q, 0))];
      }
    }
    for (; k < taps; ++k) {                                       // the last taps mod 8, with the window in place
      const float hk = h[k];
#pragma unroll
      for (int r = 0; r < kOut; ++r) acc[r] = __builtin_fmaf(hk, w[r], acc[r]);
#pragma unroll
      for (int r = kOut - 1; r > 0; --r) w[r] = w[r - 1];
      w[0] = s_d[pad8(max(base + taps - 2 - k, 0))];
    }
  }
  __syncthreads();                                                // every window read is done: the region takes the sums
#pragma unroll
  for (int r = 0; r < kOut; ++r) s_d[tid * (kOut + 1) + r] = acc[r];          // = pad8(base + r)
  __syncthreads();
  for (int p = tid; p < len; p += kThreads) out[tile0 + p] = sr[tile0 + p] + s_d[pad8(p)];
}

using p2phd::bessel_i0;

bool spans_overlap(const float* a, int64_t ld_a, const float* b, int64_t ld_b, int64_t C, int64_t L) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a1 = a0 + (uintptr_t)((C - 1) * ld_a + L) * sizeof(float), b1 = b0 + (uintptr_t)((C - 1) * ld_b + L) * sizeof(float);
  return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int p2phd_xover_tile_len(void) { return kTile; }

extern "C" int p2phd_xover_taps_fill(int taps, double cutoff, double beta, float* out) {
  P2PHD_REQUIRE(taps >= 1 && taps <= kMaxTaps && (taps & 1), "xover_taps_fill: taps must be odd and in [1, %d], got %d", kMaxTaps, taps);
  P2PHD_REQUIRE(cutoff > 0.0 && cutoff < 0.5, "xover_taps_fill: cutoff must be in (0, 0.5) cycles per sample, got %g", cutoff);
  P2PHD_REQUIRE(beta >= 0.0 && std::isfinite(beta), "xover_taps_fill: beta must be finite and >= 0, got %g", beta);
  P2PHD_REQUIRE(out != nullptr, "xover_taps_fill: null output");
  if (taps == 1) { out[0] = 1.0f; return P2PHD_OK; }
  const int c0 = (taps - 1) / 2;
  const double pi = 3.14159265358979323846, i0b = bessel_i0(beta);
  std::vector<double> h((size_t)taps);
  for (int k = 0; k <= c0; ++k) {
    const double n = (double)(k - c0);
    const double x = 2.0 * cutoff * n, y = pi * x;
    const double sinc = k == c0 ? 1.0 : std::sin(y) / y;
    const double r = 2.0 * n / (double)(taps - 1);
    const double v = 2.0 * cutoff * sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    h[(size_t)k] = v;
    h[(size_t)(taps - 1 - k)] = v;                                // symmetric bit for bit
  }
  double sum = 0.0;
  for (int k = 0; k < taps; ++k) sum += h[(size_t)k];
  for (int k = 0; k < taps; ++k) out[k] = (float)(h[(size_t)k] / sum);
  return P2PHD_OK;
}

extern "C" int p2phd_xover_fwd(const float* sr, int64_t ld_sr, const float* lr, int64_t ld_lr, float level, const float* taps_dev, int taps,
                               int64_t C, int64_t L, float* out, int64_t ld_out, void* stream) {
  P2PHD_REQUIRE(taps >= 1 && taps <= kMaxTaps && (taps & 1), "xover_fwd: taps must be odd and in [1, %d], got %d", kMaxTaps, taps);
  P2PHD_REQUIRE(C >= 0 && C <= 65535 && L >= 0 && L <= (int64_t(1) << 40), "xover_fwd: need 0 <= C <= 65535 and 0 <= L <= 2^40 (C %lld, L %lld)",
                (long long)C, (long long)L);
  P2PHD_REQUIRE(ld_sr >= L && ld_lr >= L && ld_out >= L, "xover_fwd: a row pitch is shorter than the %lld samples of a row (ld_sr %lld, ld_lr %lld, "
                "ld_out %lld)", (long long)L, (long long)ld_sr, (long long)ld_lr, (long long)ld_out);
  P2PHD_REQUIRE(std::max(ld_sr, std::max(ld_lr, ld_out)) <= (int64_t(1) << 44), "xover_fwd: a row pitch is too large");
  if (L == 0 || C == 0) return P2PHD_OK;
  P2PHD_REQUIRE(sr && lr && taps_dev && out, "xover_fwd: null pointer");
  P2PHD_REQUIRE(((reinterpret_cast<uintptr_t>(sr) | reinterpret_cast<uintptr_t>(lr) | reinterpret_cast<uintptr_t>(taps_dev) |
                  reinterpret_cast<uintptr_t>(out)) & 3) == 0, "xover_fwd: a pointer is not aligned to a float");
  P2PHD_REQUIRE(!spans_overlap(out, ld_out, sr, ld_sr, C, L) && !spans_overlap(out, ld_out, lr, ld_lr, C, L),
                "xover_fwd: out overlaps sr or lr (the kernel reads a halo of other tiles: it cannot run in place)");
  const dim3 grid((unsigned)p2phd::cdiv(L, kTile), (unsigned)C);
  const size_t lds = lds_floats(kTile + taps - 1) * sizeof(float);
  hipLaunchKernelGGL(xover_kernel, grid, dim3(kThreads), lds, (hipStream_t)stream, sr, (long)ld_sr, lr, (long)ld_lr, level, taps_dev, taps, (long)L,
                     out, (long)ld_out);
  ++p2phd::g_launch_count[p2phd::LC_XOVER];
  return p2phd::check_launch("xover_fwd");
}
