// Time-domain discriminator plumbing (--use_time_D, reference pix2pixHD_model.py:251-258, 314-320, 375-387): everything
// between the generated spectrogram and the first conv of time_D that is not a conv.
//
//   pack    (lr_frames, other_frames)[N,F,win] f32 -> NHWC [N,F,win,Cp] in the compute dtype, channel 0 = lr, 1 = other,
//           the other channels zero; mode dB: 20 log10(max(|x|, min_value)) - 20 = amplitude_to_DB(|x|, 20, min_value, 1)
//           (discriminate_time_D, :314-320), mode raw: the values themselves (:386).  One launch instead of abs, clamp,
//           log10, scale, cat, layout change and cast.
//   frames  sr_result[B,2,N,F] -> s * window[i] * IDCT_2N_native(decode(sr_result))[b,f,i]   (to_frames :251-258 and :376),
//           decode = (A0 - A1) / (2 alpha - 1), A_c = 10 * 10^((|x_c| (max - min) + min) / 20) - min_value;
//           and its adjoint: the gradient of those frames back to sr_result.
//
// The frame kernels follow dct.hip: one workgroup owns a tile of frames of one sample, each wavefront runs one N-point
// Stockham FFT per frame in its own LDS buffers.  The spectrogram is bins-major ([N bins][F frames]) and a frame is a
// column of it, so the tile is staged through LDS both ways: global accesses walk the frame axis of a row (f_tile
// consecutive floats), the per-frame transforms walk the bin axis in LDS ([f_tile][N + 1]: the + 1 keeps the transposed
// accesses off one bank).  All three kernels are streaming kernels: one pass over their operands, no reuse to exploit.
#include "common.h"
#include "convplan.h"
#include "convdev.h"
#include "streamgrid.h"
#include "fft_wave.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {
using namespace p2phd_fft;

constexpr int kThreads = 256;
constexpr int kWaves = 4;

__device__ __forceinline__ float to_db(float v, float min_value) { return 20.f * log10f(fmaxf(fabsf(v), min_value)) - 20.f; }

template <typename T> struct Px;                                // one NHWC pixel of 8 channels: (c0, c1, 0, ..., 0)
template <> struct Px<float> {
  static __device__ __forceinline__ void store(float* dst, float a, float b) {
    reinterpret_cast<float4*>(dst)[0] = make_float4(a, b, 0.f, 0.f);
    reinterpret_cast<float4*>(dst)[1] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
};
template <> struct Px<bf16_t> {
  static __device__ __forceinline__ void store(bf16_t* dst, float a, float b) {
    const unsigned lo = (unsigned)__builtin_bit_cast(unsigned short, (bf16_t)a);
    const unsigned hi = (unsigned)__builtin_bit_cast(unsigned short, (bf16_t)b);
    *reinterpret_cast<uint4*>(dst) = make_uint4(lo | (hi << 16), 0u, 0u, 0u);
  }
};

// Four pixels per thread where the quad is whole and the sources are 16-byte aligned (one float4 load per source, 64 /
// 128 contiguous bytes stored); element by element otherwise.
template <typename T, bool kDb>
__global__ __launch_bounds__(kThreads) void pack_pair_kernel(const float* __restrict__ lr, const float* __restrict__ other,
                                                             T* __restrict__ dst, long total, int vec4, float min_value) {
  const long quads = (total + 3) >> 2;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
    const long e0 = q << 2;
    float a[4], b[4];
    const int n = (int)min(4l, total - e0);
    if (vec4 && n == 4) {
      const float4 va = *reinterpret_cast<const float4*>(lr + e0), vb = *reinterpret_cast<const float4*>(other + e0);
      a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
      b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
    } else {
      for (int i = 0; i < 4; ++i) {
        a[i] = i < n ? lr[e0 + i] : 0.f;
        b[i] = i < n ? other[e0 + i] : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < n) Px<T>::store(dst + (e0 + i) * 8, kDb ? to_db(a[i], min_value) : a[i], kDb ? to_db(b[i], min_value) : b[i]);
    }
  }
}

struct FramesLds {
  float* s_x;        // [f_tile][N + 1]
  float* s_win;      // [N], already times the frame scale
  float2* s_ftw;     // exp(-2 pi i j / N)
  float2* s_rot;     // exp(-i pi k / 2N)
  float2* buf0;      // this wave's FFT buffers
  float2* buf1;
};

__device__ __forceinline__ FramesLds frames_lds(float* smem, int N, int x_cap, int wave) {
  FramesLds l;
  l.s_x = smem;
  l.s_win = smem + x_cap;
  l.s_ftw = reinterpret_cast<float2*>(l.s_win + N);
  l.s_rot = l.s_ftw + N;
  l.buf0 = l.s_rot + N + (size_t)wave * 2 * N;
  l.buf1 = l.buf0 + N;
  return l;
}

__device__ __forceinline__ float amp_of(float x, float mn, float range) { return 10.f * exp10f((fabsf(x) * range + mn) * 0.05f); }

// sr_result [B,2,N,F] -> frames [B,F,N]
__global__ __launch_bounds__(kThreads) void frames_fwd_kernel(
    const float* __restrict__ sr, const float* __restrict__ norm2, long F, int N, const float* __restrict__ window,
    const float* __restrict__ tables, float alpha, float min_value, float scale, float* __restrict__ out, int f_tile, int n_tiles,
    int x_cap, int fft_waves) {
  extern __shared__ float4 smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x / n_tiles;
  const long t0 = (long)(blockIdx.x % n_tiles) * f_tile;
  const int nf = (int)min((long)f_tile, F - t0);
  const FramesLds l = frames_lds(reinterpret_cast<float*>(smem_raw), N, x_cap, wave);

  for (int i = tid; i < N; i += kThreads) l.s_win[i] = window[i] * scale;
  const float2* tb = reinterpret_cast<const float2*>(tables);
  for (int i = tid; i < 2 * N; i += kThreads) l.s_ftw[i] = tb[i];
  const float mn = norm2[0], range = norm2[1] - norm2[0];
  const float inv = 1.f / (2.f * alpha - 1.f);
  const float* s0 = sr + (size_t)b * 2 * N * F;
  for (int idx = tid; idx < N * f_tile; idx += kThreads) {       // f_tile is a power of two
    const int j = idx & (f_tile - 1), k = idx / f_tile;
    float v = 0.f;
    if (j < nf) {
      const size_t o = (size_t)k * F + t0 + j;
      v = ((amp_of(s0[o], mn, range) - min_value) - (amp_of(s0[o + (size_t)N * F], mn, range) - min_value)) * inv;
    }
    l.s_x[j * (N + 1) + k] = v;
  }
  __syncthreads();

  for (int f0 = 0; f0 < nf; f0 += fft_waves) {
    const int f = f0 + wave;
    const bool active = wave < fft_waves && f < nf;
    if (active) {
      // conj(V_k) = (X'_k + i X'_{N-k}) * exp(-i pi k / 2N), X'_N = 0;  v = Re(FFT(conj V)) (dct.hip, imdct2_fwd_kernel)
      const float* X = l.s_x + f * (N + 1);
      for (int k = lane; k < N; k += 64) l.buf0[k] = cmul(make_float2(X[k], k == 0 ? 0.f : X[N - k]), l.s_rot[k]);
    }
    __syncthreads();
    float2* res = fft_wave(l.buf0, l.buf1, l.s_ftw, N, lane, active);
    float* stage = reinterpret_cast<float*>(res == l.buf0 ? l.buf1 : l.buf0);
    if (active) {
      for (int n = lane; n < (N >> 1); n += 64) {
        stage[2 * n] = res[n].x * l.s_win[2 * n];
        stage[2 * n + 1] = res[N - 1 - n].x * l.s_win[2 * n + 1];
      }
    }
    __syncthreads();
    if (active) {
      float4* o4 = reinterpret_cast<float4*>(out + (b * F + t0 + f) * (long)N);
      const float4* s4 = reinterpret_cast<const float4*>(stage);
      for (int i = lane; i < (N >> 2); i += 64) o4[i] = s4[i];
    }
    __syncthreads();
  }
}

// g [B,F,N] (gradient of the frames) -> g_sr [B,2,N,F]
__global__ __launch_bounds__(kThreads) void frames_bwd_kernel(
    const float* __restrict__ g, const float* __restrict__ sr, const float* __restrict__ norm2, long F, int N,
    const float* __restrict__ window, const float* __restrict__ tables, float alpha, float scale, float* __restrict__ g_sr,
    int f_tile, int n_tiles, int x_cap, int fft_waves) {
  extern __shared__ float4 smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x / n_tiles;
  const long t0 = (long)(blockIdx.x % n_tiles) * f_tile;
  const int nf = (int)min((long)f_tile, F - t0);
  const FramesLds l = frames_lds(reinterpret_cast<float*>(smem_raw), N, x_cap, wave);

  for (int i = tid; i < N; i += kThreads) l.s_win[i] = window[i] * scale;
  const float2* tb = reinterpret_cast<const float2*>(tables);
  for (int i = tid; i < 2 * N; i += kThreads) l.s_ftw[i] = tb[i];
  __syncthreads();

  for (int f0 = 0; f0 < nf; f0 += fft_waves) {
    const int f = f0 + wave;
    const bool active = wave < fft_waves && f < nf;
    if (active) {
      // adjoint of y = X_0 + 2 sum_k X_k cos(.): gX_0 = sum_i gy_i, gX_k = 2 sum_i gy_i cos(.) -- the DCT-II of dct.hip's
      // forward kernel (Makhoul reordering) with scale N and k0 1/2
      const float2* g2 = reinterpret_cast<const float2*>(g + (b * F + t0 + f) * (long)N);
      for (int n = lane; n < (N >> 1); n += 64) {
        const float2 v = g2[n];
        l.buf0[n] = make_float2(v.x * l.s_win[2 * n], 0.f);
        l.buf0[N - 1 - n] = make_float2(v.y * l.s_win[2 * n + 1], 0.f);
      }
    }
    __syncthreads();
    float2* res = fft_wave(l.buf0, l.buf1, l.s_ftw, N, lane, active);
    if (active) {
      float* X = l.s_x + f * (N + 1);
      for (int k = lane; k < N; k += 64) X[k] = cmul(res[k], l.s_rot[k]).x * (k == 0 ? 1.f : 2.f);
    }
    __syncthreads();
  }

  const float mn = norm2[0], range = norm2[1] - norm2[0];
  const float inv = 1.f / (2.f * alpha - 1.f);
  const float dk = 0.05f * 2.302585092994046f * range;          // d/dx of 10^((|x| range + min)/20), without the sign
  const size_t base = (size_t)b * 2 * N * F;
  for (int idx = tid; idx < N * f_tile; idx += kThreads) {
    const int j = idx & (f_tile - 1), k = idx / f_tile;
    if (j < nf) {
      const size_t o = base + (size_t)k * F + t0 + j;
      const float gs = l.s_x[j * (N + 1) + k] * inv;
      const float x0 = sr[o], x1 = sr[o + (size_t)N * F];
      const float sg0 = x0 > 0.f ? 1.f : (x0 < 0.f ? -1.f : 0.f), sg1 = x1 > 0.f ? 1.f : (x1 < 0.f ? -1.f : 0.f);
      g_sr[o] = gs * amp_of(x0, mn, range) * dk * sg0;
      g_sr[o + (size_t)N * F] = -gs * amp_of(x1, mn, range) * dk * sg1;
    }
  }
}

int frames_tile(int N) { return N <= 512 ? 16 : (N <= 1024 ? 8 : 4); }
int frames_fft_waves(int N) { return N <= 1024 ? kWaves : 2; }

struct FramesPlan { int f_tile, fw, x_cap; int64_t n_tiles; size_t lds; };

int frames_plan(const char* what, int64_t B, int64_t F, int n_fft, FramesPlan* p) {
  P2PHD_REQUIRE(p2phd::is_pow2(n_fft) && n_fft >= 16 && n_fft <= 2048, "%s: n_fft must be a power of two in [16, 2048], got %d", what, n_fft);
  P2PHD_REQUIRE(B >= 0 && F >= 0, "%s: negative size", what);
  p->f_tile = frames_tile(n_fft);
  p->fw = frames_fft_waves(n_fft);
  p->x_cap = (p->f_tile * (n_fft + 1) + 3) & ~3;
  p->n_tiles = p2phd::cdiv(F, p->f_tile);
  P2PHD_REQUIRE(B * p->n_tiles < (1ll << 31), "%s: grid too large", what);
  p->lds = sizeof(float) * ((size_t)p->x_cap + n_fft + 4 * (size_t)n_fft + (size_t)p->fw * 4 * n_fft);
  P2PHD_REQUIRE(p->lds <= 160 * 1024, "%s: n_fft %d needs %zu B of LDS", what, n_fft, p->lds);
  return P2PHD_OK;
}

}  // namespace

extern "C" int p2phd_timed_pack_pair(int dtype, const float* lr_frames, const float* other_frames, int64_t n_pixels, int mode_db,
                                     float min_value, void* dst, void* stream) {
  P2PHD_REQUIRE(n_pixels >= 0, "timed_pack_pair: negative size");
  if (n_pixels == 0) return P2PHD_OK;
  P2PHD_REQUIRE(lr_frames && other_frames && dst, "timed_pack_pair: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 15) == 0, "timed_pack_pair: the output must be 16-byte aligned");
  P2PHD_REQUIRE(dtype == P2PHD_BF16 || dtype == P2PHD_F32, "timed_pack_pair: unsupported dtype %d", dtype);
  P2PHD_REQUIRE(!mode_db || min_value > 0.f, "timed_pack_pair: min_value must be positive in dB mode");
  const int vec4 = ((reinterpret_cast<uintptr_t>(lr_frames) | reinterpret_cast<uintptr_t>(other_frames)) & 15) == 0;
  const int grid = p2phd::stream_grid_of(p2phd::SG_PACK_PAIR, dtype, n_pixels, 1).used;      // (streamgrid.h)
  hipStream_t st = (hipStream_t)stream;
#define P2PHD_PACK(T, DB) \
  hipLaunchKernelGGL((pack_pair_kernel<T, DB>), dim3(grid), dim3(kThreads), 0, st, lr_frames, other_frames, (T*)dst, (long)n_pixels, vec4, min_value)
  if (dtype == P2PHD_BF16) { if (mode_db) P2PHD_PACK(bf16_t, true); else P2PHD_PACK(bf16_t, false); }
  else { if (mode_db) P2PHD_PACK(float, true); else P2PHD_PACK(float, false); }
#undef P2PHD_PACK
  ++p2phd::g_launch_count[p2phd::LC_TIMED_PACK];
  return p2phd::check_launch("timed_pack_pair");
}

extern "C" int p2phd_timed_frames_fwd(const float* sr, const float* minmax, int64_t B, int64_t n_frames, int n_fft,
                                      const float* window, const float* tables, float alpha, float min_value, float scale,
                                      float* out, void* stream) {
  FramesPlan p;
  if (int rc = frames_plan("timed_frames_fwd", B, n_frames, n_fft, &p)) return rc;
  if (B == 0 || n_frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(sr && minmax && window && tables && out, "timed_frames_fwd: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "timed_frames_fwd: the output must be 16-byte aligned");
  P2PHD_REQUIRE(2.f * alpha != 1.f, "timed_frames_fwd: alpha = 0.5 has no decode");
  if (p.lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(frames_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL(frames_fwd_kernel, dim3((unsigned)(B * p.n_tiles)), dim3(kThreads), p.lds, (hipStream_t)stream, sr, minmax,
                     (long)n_frames, n_fft, window, tables, alpha, min_value, scale, out, p.f_tile, (int)p.n_tiles, p.x_cap, p.fw);
  ++p2phd::g_launch_count[p2phd::LC_TIMED_FRAMES];
  return p2phd::check_launch("timed_frames_fwd");
}

extern "C" int p2phd_timed_frames_bwd(const float* g_frames, const float* sr, const float* minmax, int64_t B, int64_t n_frames,
                                      int n_fft, const float* window, const float* tables, float alpha, float scale, float* g_sr,
                                      void* stream) {
  FramesPlan p;
  if (int rc = frames_plan("timed_frames_bwd", B, n_frames, n_fft, &p)) return rc;
  if (B == 0 || n_frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(g_frames && sr && minmax && window && tables && g_sr, "timed_frames_bwd: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(g_frames) & 7) == 0, "timed_frames_bwd: the frame gradient must be 8-byte aligned");
  P2PHD_REQUIRE(2.f * alpha != 1.f, "timed_frames_bwd: alpha = 0.5 has no decode");
  if (p.lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(frames_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL(frames_bwd_kernel, dim3((unsigned)(B * p.n_tiles)), dim3(kThreads), p.lds, (hipStream_t)stream, g_frames, sr,
                     minmax, (long)n_frames, n_fft, window, tables, alpha, scale, g_sr, p.f_tile, (int)p.n_tiles, p.x_cap, p.fw);
  ++p2phd::g_launch_count[p2phd::LC_TIMED_FRAMES];
  return p2phd::check_launch("timed_frames_bwd");
}
