// The padded LDS layout of the 8-outputs-a-thread FIR kernels (truepeak.hip, limiter.hip, xover.hip) and the polyphase walk that
// truepeak_kernel and limiter_envelope_kernel share, so that the y of one has the bits of the other by construction.  (The
// single-phase walks of xover_kernel and limiter_apply_kernel stay in their files: DESIGN.md, "Shared device contracts".)
//
// Layout: 256 threads a workgroup, a thread owns 8 CONSECUTIVE outputs and keeps their 8-wide sample window in registers, so a tap
// costs one LDS read and 8 fmas per thread and phase.  Lanes read 8 dwords apart; the staged array carries one pad dword per 8
// (position p lives at pad8(p) = p + p / 8), lane t reads 9 t + const, 9 is coprime to 32: conflict-free.  Taps: scalar loads.
// Arithmetic of a sum: one fp32 accumulator from +0 (handed in by the caller), acc = fma(tap[k], sample, acc) for k = 0, 1, ..
// Only integer and bit operations, compares, loads, stores and explicit __builtin_fmaf live here: the bits do not depend on the
// including file's `#pragma clang fp contract`; an expression whose rounding does stays in its own file.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace p2phd {
namespace fir {

constexpr int kWalkThreads = 256;             // threads of a workgroup: lds_max256 and stage_finite are written for it

// the polyphase table c[F][P] of p2phd_truepeak and p2phd_limiter_envelope: factor F, taps per phase P
constexpr int kMinTaps = 4, kMaxTaps = 64;
inline bool table_ok(int factor, int taps_per_phase) {
  return (factor == 1 || factor == 2 || factor == 4) && taps_per_phase >= kMinTaps && taps_per_phase <= kMaxTaps && (taps_per_phase & 1) == 0;
}

// floats of a padded array of n positions
constexpr size_t lds_floats(int n) { return (size_t)n + ((size_t)n >> 3) + 1; }

#ifdef __HIPCC__
__device__ __forceinline__ int pad8(int p) { return p + (p >> 3); }
__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// a workgroup's partial in the reduction scratch, read by the last workgroup to arrive (common.h: fold_arrive_last)
__device__ __forceinline__ void part_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t part_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// s[0] = the largest v of the 256 threads (a maximum does not depend on the order); ends behind a barrier
__device__ __forceinline__ void lds_max256(uint32_t* s, int tid, uint32_t v) {
  s[tid] = v;
  __syncthreads();
  for (int o = kWalkThreads / 2; o > 0; o >>= 1) {
    if (tid < o) s[tid] = max(s[tid], s[tid + o]);
    __syncthreads();
  }
}

// Position q of the padded s_x takes x~[g0 + q] for q = 0 .. n - 1: the row, 0 outside [0, L), a NaN or infinite sample taken as 0.
// No barrier.
__device__ __forceinline__ void stage_finite(float* s_x, const float* __restrict__ row, long g0, int n, long L, int tid) {
  for (int q = tid; q < n; q += kWalkThreads) {
    const long j = g0 + q;
    uint32_t bits = 0u;
    if (j >= 0 && j < L) {
      bits = __float_as_uint(row[j]);
      if ((bits & 0x7FFFFFFFu) >= 0x7F800000u) bits = 0u;         // NaN, +-inf: taken as 0
    }
    s_x[pad8(q)] = __uint_as_float(bits);
  }
}

// The window walks UP: acc[p][r] += sum_k tab[(p + 1) P + k] s_x[base + r + k], k = 0 .. P - 1, for the NP fractional phases of a
// table tab[NP + 1][P] and the kIn instants base .. base + kIn - 1 of a thread; all phases are formed from the one window.  The
// caller hands in acc = +0.  n = staged positions: the one read behind the last tap is clamped to n - 1 and not used.
template <int NP, int kIn>
__device__ __forceinline__ void polyphase_walk_up(const float* s_x, const float* __restrict__ tab, int P, int base, int n, float (&acc)[NP][kIn]) {
  static_assert(kIn == 8, "pad8 and the rotation are written for 8");
  // instant r of this thread at tap k reads position base + r + k; w holds those samples at the current tap
  float w[kIn];
#pragma unroll
  for (int r = 0; r < kIn; ++r) w[r] = s_x[pad8(base + r)];
  int k = 0;
  for (; k + kIn <= P; k += kIn) {
    // eight taps with the window rotating through the registers: at step u the sample of instant r is w[(r + u) & 7]
#pragma unroll
    for (int u = 0; u < kIn; ++u) {
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const float ck = tab[(p + 1) * P + k + u];
#pragma unroll
        for (int r = 0; r < kIn; ++r) acc[p][r] = __builtin_fmaf(ck, w[(r + u) & (kIn - 1)], acc[p][r]);
      }
      // the next tap: every instant moves one sample up, instant 7 takes a new one (not read behind the last tap)
      w[u & (kIn - 1)] = s_x[pad8(min(base + kIn + k + u, n - 1))];
    }
  }
  for (; k < P; ++k) {                                            // the last taps mod 8, with the window in place
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const float ck = tab[(p + 1) * P + k];
#pragma unroll
      for (int r = 0; r < kIn; ++r) acc[p][r] = __builtin_fmaf(ck, w[r], acc[p][r]);
    }
#pragma unroll
    for (int r = 0; r + 1 < kIn; ++r) w[r] = w[r + 1];
    w[kIn - 1] = s_x[pad8(min(base + kIn + k, n - 1))];
  }
}
#endif  // __HIPCC__

}  // namespace fir
}  // namespace p2phd
