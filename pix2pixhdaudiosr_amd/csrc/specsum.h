// The chunked float64 spectrum sum shared by ltas_kernel (bandwidth.hip) and xspec_kernel (stereo.hip), and the separation of two
// real transforms out of one complex one that stft_db_kernel (specimg.hip) takes too.
//
// Framing: the F frames that lie wholly inside a row are cut into chunks of kChunk consecutive frames; one workgroup of 256 threads
// per chunk runs the frames through n-point complex Stockham FFTs in LDS (fft_wave.h: fft_coop), two real signals per transform.
// Thread t owns the bins t, t + 256, .. (at most kOwn) and keeps their float64 sums in registers across the chunk: each summed from
// +0 in ascending frame order.  The workgroup stores its partial, takes a ticket (common.h: fold_arrive_last), and the last one to
// arrive adds the chunks' partials from +0 in ascending chunk order (fold_chunks): the sum does not depend on who finishes when.
#pragma once
#include <hip/hip_runtime.h>

namespace p2phd {
namespace spec {

constexpr int kThreads = 256;
constexpr int kChunk = 8;                       // frames per workgroup (even: a pair of frames never straddles two chunks)
constexpr int kFoldAhead = 8;                   // partials a thread of the folding workgroup loads per bin before it adds them
constexpr int kMinFft = 64, kMaxFft = 2048;
constexpr int kOwn = (kMaxFft / 2 + 1 + kThreads - 1) / kThreads;      // bins per thread at most
constexpr int kMaxBins = 4097;                  // p2phd_bandwidth, p2phd_stereo_bands: K float64 of a spectrum handed on

#ifdef __HIPCC__
__device__ __forceinline__ void part_store(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double part_load(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the 3 n / 4 twiddles the radix-4 stages reach (the largest index a stage forms is below that), from the caller's table.  No barrier.
__device__ __forceinline__ void stage_twiddles(float2* s_tw, const float* __restrict__ tables, int n, int tid) {
  for (int i = tid; i < 3 * (n >> 2); i += kThreads) s_tw[i] = reinterpret_cast<const float2*>(tables)[i];
}

// Z = the n-point transform of a + i b with a, b real: A[k] = (Z[k] + conj Z[-k]) / 2, B[k] = (Z[k] - conj Z[-k]) / 2i.
// Returns 2 A[k] = (ax, ay) and 2 B[k] = (bx, by): four additions, the halves are left to the caller's power-of-two scale.
struct TwoReal { float ax, ay, bx, by; };
__device__ __forceinline__ TwoReal separate(const float2* Z, int n, int k) {
  const float2 a = Z[k], m = Z[(n - k) & (n - 1)];
  return {a.x + m.x, a.y - m.y, a.y + m.y, m.x - a.x};
}

// The fold of one spectrum by the workgroup that arrived last: out[k] = the sum over c = 0 .. chunks - 1 of rows[c step + k], from
// +0 in ascending c, for the bins k < K of thread tid.  kFoldAhead chunks are loaded before they are added, so that a row of loads
// is in flight per thread instead of one (the order of the additions is the chunks' all the same).
__device__ __forceinline__ void fold_chunks(const double* rows, long step, long chunks, int K, int tid, double* out) {
  double s[kOwn];
#pragma unroll
  for (int i = 0; i < kOwn; ++i) s[i] = 0.0;
  long cc = 0;
  for (; cc + kFoldAhead <= chunks; cc += kFoldAhead) {
    double v[kOwn][kFoldAhead];
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int k = tid + i * kThreads;
      if (k < K) {
#pragma unroll
        for (int u = 0; u < kFoldAhead; ++u) v[i][u] = part_load(rows + (cc + u) * step + k);
      }
    }
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      if (tid + i * kThreads < K) {
#pragma unroll
        for (int u = 0; u < kFoldAhead; ++u) s[i] += v[i][u];
      }
    }
  }
  for (; cc < chunks; ++cc) {
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int k = tid + i * kThreads;
      if (k < K) s[i] += part_load(rows + cc * step + k);
    }
  }
#pragma unroll
  for (int i = 0; i < kOwn; ++i) {
    const int k = tid + i * kThreads;
    if (k < K) out[k] = s[i];
  }
}
#endif  // __HIPCC__

}  // namespace spec
}  // namespace p2phd
