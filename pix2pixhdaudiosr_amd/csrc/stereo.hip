// Whole-file generation (pix2pixhdaudiosr_amd/generate): the stereo image of a two-channel clip -- how the two written channels
// relate below and above the low rate's Nyquist frequency -- and the mid/side matrix of SuperResolver(stereo='ms').  Launch family
// "stereo".
//
//   xspec    xs[g][q][k] = sum_f Q_q[f][k] over the F = 1 + (L - n) / hop frames that lie wholly inside the clip (p2phd_ltas's
//            framing, window, tables and (4 / n)^2 scale), with A, B the Hann-windowed transforms of rows 2 g and 2 g + 1 and
//            Q_0 = |A|^2, Q_1 = |B|^2, Q_2 = Re(A conj B), Q_3 = Im(A conj B), each formed in fp32 and widened exactly.  The sum is
//            float64 in ltas's fixed order: chunks of kChunk consecutive frames, each summed from +0 ascending, the chunks' sums
//            added from +0 ascending.
//   bands    res[g] = the float64 sums of the four rows over the bins [0, k_split) and [k_split, K), in the order include/p2phd.h
//            writes down, nothing contracted: a numpy restatement returns the same bits.
//   matrix   out0 = a (x0 + s), out1 = a (x0 - s), s = x1 (with guard_side: +0 where x1 is not finite); plain fp32.
//
// xspec has the geometry of ltas_kernel (bandwidth.hip; the constants, the separation and the fold are specsum.h's): one workgroup
// of 256 threads per (chunk of 8 frames, pair), one n-point complex Stockham FFT in LDS per frame (fft_wave.h). The two slots of
// the complex transform carry the two CHANNELS of one frame, z = w x_L + i w x_R, separated with stft_db's expressions, so the
// cross term costs four more multiplies per bin and no more transforms; a chunk is eight transforms where ltas's is four. Thread t
// owns the bins t, t + 256, .. (at most 5) and keeps their four float64 sums in registers across the chunk (20 doubles). LDS as
// ltas: 22 n bytes, 44 KiB at n = 2048, three workgroups to a CU. Partials [chunk][4][K] go to the caller's workspace; the last
// workgroup of a pair to arrive folds them in chunk order, ONE quantity at a time with ltas's look-ahead of eight partials per bin
// (kOwn x kFoldAhead doubles in flight, as there: four quantities at once would not fit three workgroups to a CU). The arrival
// tickets are FOLD_LTAS's, the tickets-only region of p2phd_ltas: the two kernels never run inside one another's launch, and
// fold_scratch orders launches of one region that arrive on different streams, so an ltas and an xspec on two streams are ordered
// like two ltas calls are. No float atomics.
//
// bands: one workgroup per pair, 256 lanes, a tree in LDS.  matrix: grid-stride, float4 where both pitches and pointers allow.
#include "common.h"
#include "convplan.h"
#include "streamgrid.h"
#include "fft_wave.h"
#include "specsum.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {
using namespace p2phd_fft;
using namespace p2phd::spec;       // kThreads, kChunk, kOwn, .. and the helpers of the chunked sum: p2phd_ltas's, by construction

constexpr int kQuant = 4;                       // |A|^2, |B|^2, Re(A conj B), Im(A conj B)

// grid (chunks, G).  ticket[g / ppt] counts the workgroups of pairs [t ppt, min(G, (t + 1) ppt)): ppt = 1 unless G exceeds the tickets
__global__ __launch_bounds__(kThreads, 3) void xspec_kernel(const float* __restrict__ x, long ld, int n, int hop, long F,
                                                            const float* __restrict__ tables, float pscale, double* __restrict__ part,
                                                            unsigned* __restrict__ ticket, int ppt, int G, double* __restrict__ xs) {
  extern __shared__ float4 smem_raw[];
  float2* buf0 = reinterpret_cast<float2*>(smem_raw);
  float2* buf1 = buf0 + n;
  float2* s_tw = buf1 + n;                                        // 3 n / 4 of them: the largest index a stage forms is below that
  const int tid = threadIdx.x;
  const int K = (n >> 1) + 1;
  const long chunks = gridDim.x, c = blockIdx.x, g = blockIdx.y;
  const float* left = x + 2 * g * ld;
  const float* right = left + ld;
  const float* win = tables + 2 * n;
  stage_twiddles(s_tw, tables, n, tid);
  double acc[kQuant][kOwn];
#pragma unroll
  for (int q = 0; q < kQuant; ++q)
#pragma unroll
    for (int i = 0; i < kOwn; ++i) acc[q][i] = 0.0;
  const long f_lo = c * kChunk, f_hi = min(F, f_lo + kChunk);
  __syncthreads();
  for (long f = f_lo; f < f_hi; ++f) {
    const float* pa = left + f * hop;                             // frame f lies inside both rows
    const float* pb = right + f * hop;
    for (int j = tid; j < n; j += kThreads) {
      const float w = win[j];
      buf0[j] = make_float2(w * pa[j], w * pb[j]);
    }
    __syncthreads();
    const float2* Z = fft_coop(buf0, buf1, s_tw, n, tid, kThreads);
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int k = tid + i * kThreads;
      if (k < K) {
        const TwoReal z = separate(Z, n, k);
        acc[0][i] += (double)((z.ax * z.ax + z.ay * z.ay) * pscale);
        acc[1][i] += (double)((z.bx * z.bx + z.by * z.by) * pscale);
        acc[2][i] += (double)((z.ax * z.bx + z.ay * z.by) * pscale);      // A conj B = (ax bx + ay by) + i (ay bx - ax by)
        acc[3][i] += (double)((z.ay * z.bx - z.ax * z.by) * pscale);
      }
    }
    __syncthreads();                                              // Z is read: the next frame may overwrite either buffer
  }
  double* mine = part + (g * chunks + c) * (long)(kQuant * K);
#pragma unroll
  for (int q = 0; q < kQuant; ++q)
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      const int k = tid + i * kThreads;
      if (k < K) part_store(mine + q * K + k, acc[q][i]);
    }
  const int t = (int)(g / ppt);
  const int g_lo = t * ppt, g_hi = min(G, g_lo + ppt);
  if (!p2phd::fold_arrive_last(ticket + t, (unsigned)((g_hi - g_lo) * chunks))) return;
  // the fold (specsum.h), one quantity of one pair at a time: a thread adds its own bins' partials in chunk order
  const long step = (long)kQuant * K;                             // from one chunk's partial to the next
  for (long gg = g_lo; gg < g_hi; ++gg)
    for (int q = 0; q < kQuant; ++q) fold_chunks(part + gg * chunks * step + (long)q * K, step, chunks, K, tid, xs + (gg * kQuant + q) * K);
}

// grid (G).  The order of include/p2phd.h: per (band, row) lane t adds v[lo + t], v[lo + t + 256], .. to +0 in ascending order,
// then the 256 lanes fold as a tree, s[t] += s[t + o] for o = 128, 64, .. 1.
__global__ __launch_bounds__(kThreads) void stereo_bands_kernel(const double* __restrict__ xs, int K, int k_split, double* __restrict__ res) {
#pragma clang fp contract(off)
  __shared__ double s_lane[kThreads];
  const int tid = threadIdx.x;
  const double* base = xs + (long)blockIdx.x * kQuant * K;
  for (int b = 0; b < 2; ++b) {
    const int lo = b ? k_split : 0, hi = b ? K : k_split;
    for (int q = 0; q < kQuant; ++q) {
      const double* v = base + (long)q * K;
      double s = 0.0;
      for (int k = lo + tid; k < hi; k += kThreads) s += v[k];
      s_lane[tid] = s;
      __syncthreads();
      for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) s_lane[tid] += s_lane[tid + o];
        __syncthreads();
      }
      if (tid == 0) res[(long)blockIdx.x * 8 + b * kQuant + q] = s_lane[0];
      __syncthreads();                                            // s_lane[0] is read: the next sum may overwrite it
    }
  }
}

__device__ __forceinline__ float side_of(float s, int guard) { return guard && !(fabsf(s) <= 3.402823466e+38f) ? 0.0f : s; }

// `vec`: both pitches are multiples of 4 floats and all pointers are aligned to 16 bytes, so a float4 never straddles a row's end
__global__ __launch_bounds__(kThreads) void stereo_matrix_kernel(const float* x, long ld, long L, float a, int guard, float* out, long ld_out,
                                                                 int vec) {      // (no __restrict__: out may be x)
#pragma clang fp contract(off)
  const long stride = (long)gridDim.x * kThreads;
  long i = (long)blockIdx.x * kThreads + threadIdx.x;
  long done = 0;
  if (vec) {
    const long L4 = L >> 2;
    for (long j = i; j < L4; j += stride) {
      const float4 m = reinterpret_cast<const float4*>(x)[j];
      float4 s = reinterpret_cast<const float4*>(x + ld)[j];
      s.x = side_of(s.x, guard), s.y = side_of(s.y, guard), s.z = side_of(s.z, guard), s.w = side_of(s.w, guard);
      reinterpret_cast<float4*>(out)[j] = make_float4(a * (m.x + s.x), a * (m.y + s.y), a * (m.z + s.z), a * (m.w + s.w));
      reinterpret_cast<float4*>(out + ld_out)[j] = make_float4(a * (m.x - s.x), a * (m.y - s.y), a * (m.z - s.z), a * (m.w - s.w));
    }
    done = L4 << 2;
  }
  for (long j = done + i; j < L; j += stride) {
    const float m = x[j], s = side_of(x[ld + j], guard);
    out[j] = a * (m + s);
    out[ld_out + j] = a * (m - s);
  }
}

int check_xspec(int64_t G, int64_t L, int n_fft, int hop, const char* who) {
  P2PHD_REQUIRE(p2phd::is_pow2(n_fft) && n_fft >= kMinFft && n_fft <= kMaxFft, "%s: n_fft must be a power of two in [%d, %d], got %d", who,
                kMinFft, kMaxFft, n_fft);
  P2PHD_REQUIRE(hop >= 1 && hop <= n_fft, "%s: hop must be in [1, n_fft = %d], got %d", who, n_fft, hop);
  P2PHD_REQUIRE(G >= 0 && G <= 32767 && L >= 0 && L <= (int64_t(1) << 40), "%s: need 0 <= G <= 32767 and 0 <= L <= 2^40 (G %lld, L %lld)", who,
                (long long)G, (long long)L);
  const int64_t F = L >= n_fft ? 1 + (L - n_fft) / hop : 0;
  P2PHD_REQUIRE(F <= (int64_t(1) << 30), "%s: %lld frames are more than 2^30: use a longer hop", who, (long long)F);
  return P2PHD_OK;
}

inline int64_t frames_of(int64_t L, int n_fft, int hop) { return L >= n_fft ? 1 + (L - n_fft) / hop : 0; }

}  // namespace

extern "C" size_t p2phd_xspec_workspace_bytes(int64_t G, int64_t L, int n_fft, int hop) {
  if (check_xspec(G, L, n_fft, hop, "xspec_workspace_bytes") != P2PHD_OK) return 0;
  const int64_t chunks = p2phd::cdiv(frames_of(L, n_fft, hop), kChunk);
  return (size_t)G * (size_t)chunks * (size_t)kQuant * (size_t)(n_fft / 2 + 1) * sizeof(double);
}

extern "C" int p2phd_xspec(const float* x, int64_t ld, int64_t G, int64_t L, int n_fft, int hop, const float* tables, double* xs,
                           void* workspace, void* stream) {
  if (int rc = check_xspec(G, L, n_fft, hop, "xspec")) return rc;
  P2PHD_REQUIRE(ld >= L && ld <= (int64_t(1) << 44), "xspec: the row pitch %lld is shorter than the %lld samples of a row, or too large",
                (long long)ld, (long long)L);
  if (G == 0) return P2PHD_OK;
  P2PHD_REQUIRE(xs != nullptr && (reinterpret_cast<uintptr_t>(xs) & 7) == 0, "xspec: xs is null or not aligned to 8 bytes");
  hipStream_t st = (hipStream_t)stream;
  const int K = n_fft / 2 + 1;
  const int64_t F = frames_of(L, n_fft, hop);
  if (F == 0) {
    if (hipMemsetAsync(xs, 0, (size_t)G * kQuant * K * sizeof(double), st) != hipSuccess) {
      p2phd::set_error("xspec: memset failed");
      return P2PHD_ELAUNCH;
    }
    return P2PHD_OK;
  }
  P2PHD_REQUIRE(x && tables && workspace, "xspec: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && ((reinterpret_cast<uintptr_t>(tables) | reinterpret_cast<uintptr_t>(workspace)) & 7) == 0,
                "xspec: a pointer is not aligned (x: a float; tables, workspace: 8 bytes)");
  const p2phd::FoldScratch fs = p2phd::fold_scratch(p2phd::FOLD_LTAS, st);
  if (fs.ticket == nullptr) return P2PHD_EINVAL;                  // (refused: error text set by fold_scratch)
  const int ppt = (int)p2phd::cdiv(G, fs.tickets);               // pairs per ticket: 1 up to 1024 pairs
  const int64_t chunks = p2phd::cdiv(F, kChunk);
  const size_t lds = (size_t)n_fft * 2 * sizeof(float2) + (size_t)(3 * (n_fft / 4)) * sizeof(float2);
  const float pscale = 4.0f / ((float)n_fft * (float)n_fft);      // (4 / n)^2 / 4, the halves of the separation: a power of two
  hipLaunchKernelGGL(xspec_kernel, dim3((unsigned)chunks, (unsigned)G), dim3(kThreads), lds, st, x, (long)ld, n_fft, hop, (long)F, tables, pscale,
                     static_cast<double*>(workspace), fs.ticket, ppt, (int)G, xs);
  ++p2phd::g_launch_count[p2phd::LC_STEREO];
  return p2phd::check_launch("xspec");
}

extern "C" int p2phd_stereo_bands(const double* xs, int64_t G, int K, int k_split, double* res, void* stream) {
  P2PHD_REQUIRE(K >= 2 && K <= kMaxBins, "stereo_bands: need 2 <= K <= %d bins, got %d", kMaxBins, K);
  P2PHD_REQUIRE(k_split >= 1 && k_split <= K - 1, "stereo_bands: k_split must be in [1, K - 1 = %d], got %d", K - 1, k_split);
  P2PHD_REQUIRE(G >= 0 && G <= 2147483647LL / 4, "stereo_bands: need 0 <= G <= (2^31 - 1) / 4, got %lld", (long long)G);
  if (G == 0) return P2PHD_OK;
  P2PHD_REQUIRE(xs && res, "stereo_bands: null pointer");
  P2PHD_REQUIRE(((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(res)) & 7) == 0, "stereo_bands: a pointer is not aligned to 8 bytes");
  hipLaunchKernelGGL(stereo_bands_kernel, dim3((unsigned)G), dim3(kThreads), 0, (hipStream_t)stream, xs, K, k_split, res);
  ++p2phd::g_launch_count[p2phd::LC_STEREO];
  return p2phd::check_launch("stereo_bands");
}

extern "C" int p2phd_stereo_matrix(const float* x, int64_t ld, int64_t L, float a, int guard_side, float* out, int64_t ld_out, void* stream) {
  P2PHD_REQUIRE(L >= 0 && L <= (int64_t(1) << 40), "stereo_matrix: need 0 <= L <= 2^40, got %lld", (long long)L);
  P2PHD_REQUIRE(ld >= L && ld_out >= L && ld <= (int64_t(1) << 44) && ld_out <= (int64_t(1) << 44),
                "stereo_matrix: a row pitch (%lld, %lld) is shorter than the %lld samples of a row, or too large", (long long)ld, (long long)ld_out,
                (long long)L);
  P2PHD_REQUIRE(a == a && fabsf(a) <= 3.402823466e+38f, "stereo_matrix: the factor a must be finite");
  if (L == 0) return P2PHD_OK;
  P2PHD_REQUIRE(x && out, "stereo_matrix: null pointer");
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
  P2PHD_REQUIRE(((xa | oa) & 3) == 0, "stereo_matrix: a pointer is not aligned to a float");
  // in place is allowed as out == x with one pitch (a thread reads both its samples before it writes either); any other overlap is not
  const uintptr_t xe = xa + (size_t)(ld + L) * sizeof(float), oe = oa + (size_t)(ld_out + L) * sizeof(float);
  P2PHD_REQUIRE((xa == oa && ld == ld_out) || xe <= oa || oe <= xa, "stereo_matrix: out overlaps x without being x at the same row pitch");
  const int vec = ((xa | oa) & 15) == 0 && ((ld | ld_out) & 3) == 0;
  const int blocks = p2phd::stream_grid_of(vec ? p2phd::SG_STEREO_VEC : p2phd::SG_STEREO_SCALAR, P2PHD_F32, L, 2).used;     // (streamgrid.h)
  hipLaunchKernelGGL(stereo_matrix_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, x, (long)ld, (long)L, a, guard_side != 0,
                     out, (long)ld_out, vec);
  ++p2phd::g_launch_count[p2phd::LC_STEREO];
  return p2phd::check_launch("stereo_matrix");
}
