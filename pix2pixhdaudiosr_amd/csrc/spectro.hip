// Spectrogram codec around the MDCT: Pix2PixHDModel.to_spectro / denormalize / to_audio
// (models/pix2pixHD_model.py:142-249): the explicit two-channel encoding of the published runs and the single-channel
// magnitude encoding, every mask_mode.
//
// encode: spec[B,F,M] (frames x bins, MDCT4 output) -> log_spectro[B,2,M,F] in [0,1], pha[B,1,M,F]
//   pass 1  transposes through a 32x32 LDS tile (reads coalesced along bins, writes coalesced along frames),
//           applies the neg/pos split (:150-151) and amplitude_to_DB(., 20, min_value, 1) (:154-155), and leaves
//           per-block (min, max, sum, sumsq) partials -- the global min/max of :167-168 without a host sync;
//   finalize reduces the partials to (min, max, mean, std) on the device;
//   pass 2  normalises in place (:193) and overwrites the top mask rows with min-max-scaled noise (:196-226).
// decode: log_spectro[B,2,M,F] -> spec[B,F,M] = (A0 - A1)/(2 alpha - 1), A = DB_to_amplitude(|x|(max-min)+min, 10, .5) - min_value
#include "common.h"
#include "convplan.h"
#include "streamgrid.h"
#include <algorithm>
#include <cstdint>

namespace {

__device__ __forceinline__ void block_reduce4(float mn, float mx, float s1, float s2, float* out4) {
  __shared__ float red[4][4];
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o));
    s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o);
  }
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  const int w = tid >> 6;
  if ((tid & 63) == 0) { red[w][0] = mn; red[w][1] = mx; red[w][2] = s1; red[w][3] = s2; }
  __syncthreads();
  if (tid == 0) {
    const int nw = (blockDim.x * blockDim.y + 63) / 64;
    for (int i = 1; i < nw; ++i) { mn = fminf(mn, red[i][0]); mx = fmaxf(mx, red[i][1]); s1 += red[i][2]; s2 += red[i][3]; }
    out4[0] = mn; out4[1] = mx; out4[2] = s1; out4[3] = s2;
  }
}

__global__ __launch_bounds__(256) void encode_pass1_kernel(const float* __restrict__ spec, float* __restrict__ db,
                                                           float* __restrict__ pha, float* __restrict__ partials, int F,
                                                           int M, float alpha, float min_value, int channels) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, m0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;
  for (int i = 0; i < 4; ++i) {
    const int f = f0 + ty + 8 * i, m = m0 + tx;
    tile[ty + 8 * i][tx] = (f < F && m < M) ? spec[((size_t)b * F + f) * M + m] : 0.f;
  }
  __syncthreads();
  float mn = INFINITY, mx = -INFINITY, s1 = 0.f, s2 = 0.f;
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 8 * i, f = f0 + tx;
    if (m < M && f < F) {
      const float s = tile[tx][ty + 8 * i];
      pha[((size_t)b * M + m) * F + f] = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
      if (channels == 2) {                                       // explicit encoding (:149-158)
        const float neg = 0.5f * (fabsf(s) - s);
        const float pos = s + neg;
        const float d0 = 20.f * log10f(fmaxf(alpha * pos + (1.f - alpha) * neg, min_value)) - 20.f;
        const float d1 = 20.f * log10f(fmaxf((1.f - alpha) * pos + alpha * neg, min_value)) - 20.f;
        const size_t o = ((size_t)b * 2 * M + m) * F + f;
        db[o] = d0;
        db[o + (size_t)M * F] = d1;
        mn = fminf(mn, fminf(d0, d1)); mx = fmaxf(mx, fmaxf(d0, d1));
        s1 += d0 + d1; s2 += d0 * d0 + d1 * d1;
      } else {                                                   // magnitude only (:159-162); the sign travels in pha
        const float d0 = 20.f * log10f(fmaxf(fabsf(s) + min_value, min_value)) - 20.f;
        db[((size_t)b * M + m) * F + f] = d0;
        mn = fminf(mn, d0); mx = fmaxf(mx, d0);
        s1 += d0; s2 += d0 * d0;
      }
    }
  }
  const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  block_reduce4(mn, mx, s1, s2, partials + 4 * blk);
}

__global__ __launch_bounds__(256) void stats4_kernel(const float* __restrict__ x, long n, float* __restrict__ partials) {
  float mn = INFINITY, mx = -INFINITY, s1 = 0.f, s2 = 0.f;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const float v = x[e];
    mn = fminf(mn, v); mx = fmaxf(mx, v); s1 += v; s2 += v * v;
  }
  block_reduce4(mn, mx, s1, s2, partials + 4 * blockIdx.x);
}

// out4 = (min, max, mean, unbiased std) over `count` values described by nblk partials
__global__ __launch_bounds__(256) void finalize4_kernel(const float* __restrict__ partials, int nblk, double count, float* __restrict__ out4) {
  __shared__ double rs[256], rq[256];
  __shared__ float rmn[256], rmx[256];
  float mn = INFINITY, mx = -INFINITY;
  double s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
    mn = fminf(mn, partials[4 * i]); mx = fmaxf(mx, partials[4 * i + 1]);
    s1 += partials[4 * i + 2]; s2 += partials[4 * i + 3];
  }
  rmn[threadIdx.x] = mn; rmx[threadIdx.x] = mx; rs[threadIdx.x] = s1; rq[threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 256; ++i) { mn = fminf(mn, rmn[i]); mx = fmaxf(mx, rmx[i]); s1 += rs[i]; s2 += rq[i]; }
    const double mean = s1 / count;
    const double var = count > 1 ? (s2 - count * mean * mean) / (count - 1) : 0.0;
    out4[0] = mn; out4[1] = mx; out4[2] = (float)mean; out4[3] = (float)sqrt(var > 0 ? var : 0.0);
  }
}

// mask_mode (:207-221): 0 = noise / (max - min) (single peak at 0), 1 = min-max scaled noise times a random sign,
// 2 = min-max scaled noise; no noise pointer = zeros (mask_mode None)
__global__ __launch_bounds__(256) void encode_pass2_kernel(float* __restrict__ db, const float* __restrict__ norm4,
                                                           const float* __restrict__ noise, const float* __restrict__ nnorm4,
                                                           int M, int F, int mask_rows, long total, int mask_mode,
                                                           const float* __restrict__ noise_sign) {
  const float mn = norm4[0], scale = 1.f / (norm4[1] - norm4[0]);
  float nmn = 0.f, nscale = 0.f;
  if (noise != nullptr) { nmn = mask_mode == 0 ? 0.f : nnorm4[0]; nscale = 1.f / (nnorm4[1] - nnorm4[0]); }
  const int keep = M - mask_rows;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int f = (int)(e % F);
    const long r = e / F;
    const int m = (int)(r % M);
    const long bc = r / M;                                     // b*2 + channel
    float v;
    if (m < keep) v = (db[e] - mn) * scale;
    else if (noise != nullptr) {
      const long q = (bc * mask_rows + (m - keep)) * F + f;
      v = (noise[q] - nmn) * nscale;
      if (mask_mode == 1) v *= noise_sign[q];
    } else v = 0.f;
    db[e] = v;
  }
}

__global__ __launch_bounds__(256) void decode_kernel(const float* __restrict__ x, const float* __restrict__ norm2,
                                                     float* __restrict__ spec, int F, int M, float alpha, float min_value) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, m0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const float mn = norm2[0], range = norm2[1] - norm2[0];
  const float inv = 1.f / (2.f * alpha - 1.f);
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 8 * i, f = f0 + tx;
    float v = 0.f;
    if (m < M && f < F) {
      const size_t o = ((size_t)b * 2 * M + m) * F + f;
      const float a0 = 10.f * exp10f((fabsf(x[o]) * range + mn) * 0.05f) - min_value;
      const float a1 = 10.f * exp10f((fabsf(x[o + (size_t)M * F]) * range + mn) * 0.05f) - min_value;
      v = (a0 - a1) * inv;
    }
    tile[ty + 8 * i][tx] = v;
  }
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int f = f0 + ty + 8 * i, m = m0 + tx;
    if (f < F && m < M) spec[((size_t)b * F + f) * M + m] = tile[tx][ty + 8 * i];
  }
}

// util.imdct's decode (util/util.py:104-126): amplitude = sum of the channels, sign = pha below `keep` rows and
// sign(ch0 - ch1) above (explicit encoding); single channel: sign = pha everywhere (the caller draws the random signs).
__global__ __launch_bounds__(256) void decode_signed_kernel(const float* __restrict__ x, const float* __restrict__ pha,
                                                            const float* __restrict__ norm2, float* __restrict__ spec, int F, int M,
                                                            int channels, int keep, float min_value, float scale, int norm_stride) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, m0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;
  norm2 += (size_t)b * norm_stride;                               // 0: one range for all rows; 8: row b's own (norm_rows)
  const float mn = norm2[0], range = norm2[1] - norm2[0];
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 8 * i, f = f0 + tx;
    float v = 0.f;
    if (m < M && f < F) {
      const size_t o = ((size_t)b * channels * M + m) * F + f;
      const float a0 = 10.f * exp10f((fabsf(x[o]) * range + mn) * 0.05f) - min_value;
      float sgn = pha[((size_t)b * M + m) * F + f];
      float amp = a0;
      if (channels == 2) {
        const float a1 = 10.f * exp10f((fabsf(x[o + (size_t)M * F]) * range + mn) * 0.05f) - min_value;
        amp = a0 + a1;
        if (m >= keep) sgn = a0 > a1 ? 1.f : (a0 < a1 ? -1.f : 0.f);
      }
      v = amp * sgn * scale;
    }
    tile[ty + 8 * i][tx] = v;
  }
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int f = f0 + ty + 8 * i, m = m0 + tx;
    if (f < F && m < M) spec[((size_t)b * F + f) * M + m] = tile[tx][ty + 8 * i];
  }
}

// One element of decode_signed_kernel for tensor x: the same expressions in the same order, so a row decoded here carries
// the bits that kernel writes for it.  `sgn` is the pha value (not read where the channels give the sign).
__device__ __forceinline__ float decode_signed_at(const float* __restrict__ x, size_t o, size_t plane, float sgn, int channels,
                                                  bool sign_from_channels, float mn, float range, float min_value, float scale) {
  const float a0 = 10.f * exp10f((fabsf(x[o]) * range + mn) * 0.05f) - min_value;
  float amp = a0;
  if (channels == 2) {
    const float a1 = 10.f * exp10f((fabsf(x[o + plane]) * range + mn) * 0.05f) - min_value;
    amp = a0 + a1;
    if (sign_from_channels) sgn = a0 > a1 ? 1.f : (a0 < a1 ? -1.f : 0.f);
  }
  return amp * sgn * scale;
}

// s + w (l - s) from rounded operands, one rounding per operation: no contraction across the decode, so that l == s gives s.
__device__ __forceinline__ float splice_blend(float s, float l, float w) {
#pragma clang fp contract(off)
  const float d = l - s;
  const float wd = w * d;
  return s + wd;
}

// decode_signed_kernel with the low band taken from the input's own spectrogram: rows below keep - fade decode `lr`, rows
// from keep decode `sr`, the fade rows between cross-fade the two decoded values with the input's weight
// w = cos^2(pi (j + 1/2) / (2 fade)) = (1 + cos(pi (2 j + 1) / (2 fade))) / 2, j = m - (keep - fade).  A row loads only
// the tensors it decodes (and pha only where it gives the sign).  Same tile, grid and block as decode_signed_kernel.
__global__ __launch_bounds__(256) void decode_spliced_kernel(const float* __restrict__ sr, const float* __restrict__ lr,
                                                             const float* __restrict__ pha, const float* __restrict__ norm2,
                                                             float* __restrict__ spec, int F, int M, int channels, int keep,
                                                             int fade, float min_value, float scale, int norm_stride) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, m0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;
  norm2 += (size_t)b * norm_stride;                               // as in decode_signed_kernel
  const float mn = norm2[0], range = norm2[1] - norm2[0];
  const size_t plane = (size_t)M * F;
  const int lo = keep - fade;                                     // first fade row
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 8 * i, f = f0 + tx;
    float v = 0.f;
    if (m < M && f < F) {
      const size_t o = ((size_t)b * channels * M + m) * F + f;
      const bool from_channels = channels == 2 && m >= keep;
      const float sgn = from_channels ? 0.f : pha[((size_t)b * M + m) * F + f];
      if (m >= keep) {
        v = decode_signed_at(sr, o, plane, sgn, channels, from_channels, mn, range, min_value, scale);
      } else if (m < lo) {
        v = decode_signed_at(lr, o, plane, sgn, channels, false, mn, range, min_value, scale);
      } else {
        const float s = decode_signed_at(sr, o, plane, sgn, channels, false, mn, range, min_value, scale);
        const float l = decode_signed_at(lr, o, plane, sgn, channels, false, mn, range, min_value, scale);
        const float w = 0.5f + 0.5f * cospif((float)(2 * (m - lo) + 1) / (float)(2 * fade));
        v = splice_blend(s, l, w);
      }
    }
    tile[ty + 8 * i][tx] = v;
  }
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int f = f0 + ty + 8 * i, m = m0 + tx;
    if (f < F && m < M) spec[((size_t)b * F + f) * M + m] = tile[tx][ty + 8 * i];
  }
}

// ---- one normalisation range for many encodes (whole-file generation, norm_scope='clip') ------------------------------------
// The range is found in a pass in front of the encodes (range_kernel + range_fold_kernel, accumulated in two floats on the
// device), then every encode reads it (encode_given_kernel) instead of reducing its own tensor.

// What encode_pass1_kernel (CH = 2, 1: its dB values for the spectrum value s, the same expressions in the same order) or
// stats4_kernel (CH = 0: the value itself) folds into its min and max.
template <int CH>
__device__ __forceinline__ void fold_minmax(float s, float alpha, float min_value, float& mn, float& mx) {
  if (CH == 2) {
    const float neg = 0.5f * (fabsf(s) - s);
    const float pos = s + neg;
    const float d0 = 20.f * log10f(fmaxf(alpha * pos + (1.f - alpha) * neg, min_value)) - 20.f;
    const float d1 = 20.f * log10f(fmaxf((1.f - alpha) * pos + alpha * neg, min_value)) - 20.f;
    mn = fminf(mn, fminf(d0, d1)); mx = fmaxf(mx, fmaxf(d0, d1));
  } else if (CH == 1) {
    const float d0 = 20.f * log10f(fmaxf(fabsf(s) + min_value, min_value)) - 20.f;
    mn = fminf(mn, d0); mx = fmaxf(mx, d0);
  } else {
    mn = fminf(mn, s); mx = fmaxf(mx, s);
  }
}

// (mn, mx) of a block of 256 threads; thread 0 holds the result
__device__ __forceinline__ void block_minmax(float& mn, float& mx) {
  __shared__ float red[4][2];
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[w][0] = mn; red[w][1] = mx; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < 4; ++i) { mn = fminf(mn, red[i][0]); mx = fmaxf(mx, red[i][1]); }
}

// A streaming read of x[0, n): the first 4 * n4 floats as float4 (n4 = 0 where x is not 16-byte aligned), the rest one by one;
// min and max do not depend on the order, so the tile walk of pass 1 is not repeated.  partials[2 * block] = (min, max).
template <int CH>
__global__ __launch_bounds__(256) void range_kernel(const float* __restrict__ x, long n, long n4, float alpha, float min_value,
                                                    float* __restrict__ partials) {
  float mn = INFINITY, mx = -INFINITY;
  const long stride = (long)gridDim.x * 256;
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += stride) {
    const float4 v = x4[e];
    fold_minmax<CH>(v.x, alpha, min_value, mn, mx); fold_minmax<CH>(v.y, alpha, min_value, mn, mx);
    fold_minmax<CH>(v.z, alpha, min_value, mn, mx); fold_minmax<CH>(v.w, alpha, min_value, mn, mx);
  }
  for (long e = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) fold_minmax<CH>(x[e], alpha, min_value, mn, mx);
  block_minmax(mn, mx);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = mn; partials[2 * blockIdx.x + 1] = mx; }
}

// minmax_io = (fminf(minmax_io[0], min of the partials), fmaxf(minmax_io[1], max of the partials)): one block, plain stores
__global__ __launch_bounds__(256) void range_fold_kernel(const float* __restrict__ partials, int nblk, float* __restrict__ minmax_io) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < nblk; i += 256) { mn = fminf(mn, partials[2 * i]); mx = fmaxf(mx, partials[2 * i + 1]); }
  block_minmax(mn, mx);
  if (threadIdx.x == 0) { minmax_io[0] = fminf(minmax_io[0], mn); minmax_io[1] = fmaxf(minmax_io[1], mx); }
}

template <int CH>
int launch_range(const float* x, long n, float alpha, float min_value, float* minmax_io, float* partials, hipStream_t st) {
  const long n4 = ((uintptr_t)x & 15) == 0 ? n / 4 : 0;
  // (streamgrid.h: n4 + (n - 4 * n4) items, at most 1024 workgroups) 2 * 1024 floats: inside the 4 * 1024 every caller's workspace has
  const int nb = p2phd::stream_grid_of(n4 ? p2phd::SG_RANGE_VEC : p2phd::SG_RANGE_SCALAR, P2PHD_F32, n, 1).used;
  hipLaunchKernelGGL(range_kernel<CH>, dim3(nb), dim3(256), 0, st, x, n, n4, alpha, min_value, partials);
  hipLaunchKernelGGL(range_fold_kernel, dim3(1), dim3(256), 0, st, partials, nb, minmax_io);
  return nb;
}

// encode_pass1_kernel and encode_pass2_kernel in one pass over the tile, the statistics read from norm8 = (min, max, -, -,
// noise_min, noise_max, -, -): the dB values of the kept rows by pass 1's expressions, normalised by pass 2's; the mask rows
// by pass 2's, their dB values never formed.  A range of zero gives the scale 0 where pass 2 divides by it.
__global__ __launch_bounds__(256) void encode_given_kernel(const float* __restrict__ spec, const float* __restrict__ norm8,
                                                           const float* __restrict__ noise, const float* __restrict__ noise_sign,
                                                           float* __restrict__ out, float* __restrict__ pha, int F, int M,
                                                           float alpha, float min_value, int channels, int mask_rows, int mask_mode,
                                                           int norm_stride) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, m0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;
  for (int i = 0; i < 4; ++i) {
    const int f = f0 + ty + 8 * i, m = m0 + tx;
    tile[ty + 8 * i][tx] = (f < F && m < M) ? spec[((size_t)b * F + f) * M + m] : 0.f;
  }
  norm8 += (size_t)b * norm_stride;                               // 0: one norm8 for all rows; 8: row b's own (norm_rows)
  const float mn = norm8[0], range = norm8[1] - norm8[0];
  const float scale = range == 0.f ? 0.f : 1.f / range;
  float nmn = 0.f, nscale = 0.f;
  if (noise != nullptr) {
    const float nrange = norm8[5] - norm8[4];
    nmn = mask_mode == 0 ? 0.f : norm8[4];
    nscale = nrange == 0.f ? 0.f : 1.f / nrange;
  }
  const int keep = M - mask_rows;
  const size_t plane = (size_t)M * F;
  __syncthreads();
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + ty + 8 * i, f = f0 + tx;
    if (m < M && f < F) {
      const float s = tile[tx][ty + 8 * i];
      pha[((size_t)b * M + m) * F + f] = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
      const size_t o = ((size_t)b * channels * M + m) * F + f;
      if (m < keep) {
        if (channels == 2) {
          const float neg = 0.5f * (fabsf(s) - s);
          const float pos = s + neg;
          const float d0 = 20.f * log10f(fmaxf(alpha * pos + (1.f - alpha) * neg, min_value)) - 20.f;
          const float d1 = 20.f * log10f(fmaxf((1.f - alpha) * pos + alpha * neg, min_value)) - 20.f;
          out[o] = (d0 - mn) * scale;
          out[o + plane] = (d1 - mn) * scale;
        } else {
          const float d0 = 20.f * log10f(fmaxf(fabsf(s) + min_value, min_value)) - 20.f;
          out[o] = (d0 - mn) * scale;
        }
      } else {
        for (int c = 0; c < channels; ++c) {
          float v = 0.f;
          if (noise != nullptr) {
            const size_t q = (((size_t)b * channels + c) * mask_rows + (m - keep)) * F + f;
            v = (noise[q] - nmn) * nscale;
            if (mask_mode == 1) v *= noise_sign[q];
          }
          out[o + c * plane] = v;
        }
      }
    }
  }
}

// ---- one normalisation range per row (whole-file generation, segment_norm) ---------------------------------------------------
// rows_stats_kernel leaves (min, max, noise min, noise max) of a chunk of every row, rows_fold_kernel folds a row's chunks into
// its norm8 (plain stores, no atomics: min and max do not depend on the order), and encode_given_kernel / the decodes read row
// b's statistics at norm_rows + 8 b.

// fold_minmax over x[0, n), this workgroup's share of `chunks`: float4 reads where this base is 16-byte aligned, else one by one
template <int CH>
__device__ __forceinline__ void fold_stream(const float* __restrict__ x, long n, int chunk, int chunks, float alpha, float min_value,
                                            float& mn, float& mx) {
  const long n4 = ((uintptr_t)x & 15) == 0 ? n / 4 : 0;
  const long stride = (long)chunks * 256;
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
  for (long e = (long)chunk * 256 + threadIdx.x; e < n4; e += stride) {
    const float4 v = x4[e];
    fold_minmax<CH>(v.x, alpha, min_value, mn, mx); fold_minmax<CH>(v.y, alpha, min_value, mn, mx);
    fold_minmax<CH>(v.z, alpha, min_value, mn, mx); fold_minmax<CH>(v.w, alpha, min_value, mn, mx);
  }
  for (long e = 4 * n4 + (long)chunk * 256 + threadIdx.x; e < n; e += stride) fold_minmax<CH>(x[e], alpha, min_value, mn, mx);
}

// grid (chunks, B): partials[4 (b chunks + chunk)] = (min, max) of the dB values of the chunk's share of row b's n = F M spectrum
// values, then those of its share of row b's nn noise values ((+inf, -inf) without noise).  The alignment is that of each row's
// own base: with n or nn no multiple of 4 the rows behind the first start off a 16-byte boundary.
template <int CH>
__global__ __launch_bounds__(256) void rows_stats_kernel(const float* __restrict__ spec, long n, const float* __restrict__ noise,
                                                         long nn, float alpha, float min_value, float* __restrict__ partials) {
  const int b = blockIdx.y;
  float mn = INFINITY, mx = -INFINITY, nmn = INFINITY, nmx = -INFINITY;
  fold_stream<CH>(spec + (size_t)b * n, n, blockIdx.x, gridDim.x, alpha, min_value, mn, mx);
  if (noise != nullptr) fold_stream<0>(noise + (size_t)b * nn, nn, blockIdx.x, gridDim.x, 0.f, 0.f, nmn, nmx);
  block_minmax(mn, mx);
  __syncthreads();                                                // block_minmax's LDS words are read by thread 0 until here
  block_minmax(nmn, nmx);
  if (threadIdx.x == 0) {
    float* p = partials + 4 * ((size_t)b * gridDim.x + blockIdx.x);
    p[0] = mn; p[1] = mx; p[2] = nmn; p[3] = nmx;
  }
}

// grid B, one wave: norm_rows[8 b] = (min, max, 0, 0, noise min, noise max, 0, 0) of row b's `chunks` partials
__global__ __launch_bounds__(64) void rows_fold_kernel(const float* __restrict__ partials, int chunks, float* __restrict__ norm_rows) {
  const int b = blockIdx.x;
  float mn = INFINITY, mx = -INFINITY, nmn = INFINITY, nmx = -INFINITY;
  for (int i = threadIdx.x; i < chunks; i += 64) {
    const float* p = partials + 4 * ((size_t)b * chunks + i);
    mn = fminf(mn, p[0]); mx = fmaxf(mx, p[1]); nmn = fminf(nmn, p[2]); nmx = fmaxf(nmx, p[3]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o));
    nmn = fminf(nmn, __shfl_xor(nmn, o)); nmx = fmaxf(nmx, __shfl_xor(nmx, o));
  }
  if (threadIdx.x == 0) {
    float* q = norm_rows + 8 * (size_t)b;
    q[0] = mn; q[1] = mx; q[2] = 0.f; q[3] = 0.f; q[4] = nmn; q[5] = nmx; q[6] = 0.f; q[7] = 0.f;
  }
}

// workgroups per row of rows_stats_kernel
inline int rows_chunks(int64_t F, int64_t M) { return p2phd::stream_grid_of(p2phd::SG_SPECTRO_ROWS, P2PHD_F32, F * M, 1).used; }

}  // namespace

extern "C" int64_t p2phd_spectro_partials_floats(int64_t B, int64_t F, int64_t M) {
  return 4 * B * ((F + 31) / 32) * ((M + 31) / 32) + 4 * 1024;   // encode blocks + noise-statistics blocks
}

extern "C" int p2phd_spectro_encode_ex(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha,
                                       float min_value, int mask_rows, int mask_mode, const float* noise,
                                       const float* noise_sign, float* log_spectro, float* pha, float* norm4, float* partials,
                                       void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1 && mask_rows >= 0 && mask_rows <= M, "spectro_encode: bad geometry");
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_encode: channels must be 2 (explicit encoding) or 1");
  P2PHD_REQUIRE(mask_mode >= 0 && mask_mode <= 2, "spectro_encode: mask_mode must be 0, 1 or 2");
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(spec && log_spectro && pha && norm4 && partials, "spectro_encode: null pointer");
  P2PHD_REQUIRE(!(mask_mode == 1 && noise != nullptr && mask_rows > 0 && noise_sign == nullptr), "spectro_encode: mask mode1 needs the sign tensor");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_encode: grid too large");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  const int nblk = (int)(grid.x * grid.y * grid.z);
  hipLaunchKernelGGL(encode_pass1_kernel, grid, dim3(32, 8), 0, st, spec, log_spectro, pha, partials, (int)F, (int)M, alpha, min_value, channels);
  hipLaunchKernelGGL(finalize4_kernel, dim3(1), dim3(256), 0, st, partials, nblk, (double)(channels * B * F * M), norm4);
  float* npart = partials + 4 * (size_t)nblk;
  float* nnorm = norm4 + 4;
  if (noise != nullptr && mask_rows > 0) {
    const long n = channels * B * mask_rows * F;
    const int nb = p2phd::stream_grid_of(p2phd::SG_SPECTRO_STATS, P2PHD_F32, n, 1).used;
    hipLaunchKernelGGL(stats4_kernel, dim3(nb), dim3(256), 0, st, noise, n, npart);
    hipLaunchKernelGGL(finalize4_kernel, dim3(1), dim3(256), 0, st, npart, nb, (double)n, nnorm);
  }
  const long total = channels * B * M * F;
  const int blocks = p2phd::stream_grid_of(p2phd::SG_SPECTRO_ENCODE, P2PHD_F32, total, 1).used;
  hipLaunchKernelGGL(encode_pass2_kernel, dim3(blocks), dim3(256), 0, st, log_spectro, norm4, mask_rows > 0 ? noise : nullptr,
                     nnorm, (int)M, (int)F, mask_rows, total, mask_mode, noise_sign);
  return p2phd::check_launch("spectro_encode");
}

extern "C" int p2phd_spectro_encode(const float* spec, int64_t B, int64_t F, int64_t M, float alpha, float min_value,
                                    int mask_rows, const float* noise, float* log_spectro, float* pha, float* norm4,
                                    float* partials, void* stream) {
  return p2phd_spectro_encode_ex(spec, B, F, M, 2, alpha, min_value, mask_rows, 2, noise, nullptr, log_spectro, pha, norm4,
                                 partials, stream);
}

extern "C" int p2phd_spectro_decode(const float* log_spectro, const float* norm_min_max, int64_t B, int64_t F, int64_t M,
                                    float alpha, float min_value, float* spec, void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_decode: bad geometry");
  P2PHD_REQUIRE(alpha != 0.5f, "spectro_decode: alpha = 0.5 makes the explicit encoding singular");
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(log_spectro && norm_min_max && spec, "spectro_decode: null pointer");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_decode: grid too large");
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(decode_kernel, grid, dim3(32, 8), 0, (hipStream_t)stream, log_spectro, norm_min_max, spec, (int)F, (int)M, alpha, min_value);
  return p2phd::check_launch("spectro_decode");
}

extern "C" int p2phd_spectro_decode_signed(const float* log_spectro, const float* pha, const float* norm_min_max, int64_t B,
                                           int64_t F, int64_t M, int channels, int keep_rows, float min_value, float scale,
                                           float* spec, void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_decode_signed: bad geometry");
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_decode_signed: channels must be 1 or 2, got %d", channels);
  P2PHD_REQUIRE(keep_rows >= 0 && keep_rows <= M, "spectro_decode_signed: keep_rows %d outside [0, %lld]", keep_rows, (long long)M);
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(log_spectro && pha && norm_min_max && spec, "spectro_decode_signed: null pointer");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_decode_signed: grid too large");
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(decode_signed_kernel, grid, dim3(32, 8), 0, (hipStream_t)stream, log_spectro, pha, norm_min_max, spec, (int)F,
                     (int)M, channels, keep_rows, min_value, scale, 0);
  return p2phd::check_launch("spectro_decode_signed");
}

extern "C" int p2phd_spectro_decode_spliced(const float* sr_log_spectro, const float* lr_log_spectro, const float* pha,
                                            const float* norm_min_max, int64_t B, int64_t F, int64_t M, int channels,
                                            int keep_rows, int fade_rows, float min_value, float scale, float* spec,
                                            void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_decode_spliced: bad geometry");
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_decode_spliced: channels must be 1 or 2, got %d", channels);
  P2PHD_REQUIRE(keep_rows >= 0 && keep_rows <= M, "spectro_decode_spliced: keep_rows %d outside [0, %lld]", keep_rows, (long long)M);
  P2PHD_REQUIRE(fade_rows >= 0 && fade_rows <= keep_rows, "spectro_decode_spliced: fade_rows %d outside [0, keep_rows = %d]",
                fade_rows, keep_rows);
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(sr_log_spectro && lr_log_spectro && pha && norm_min_max && spec, "spectro_decode_spliced: null pointer");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_decode_spliced: grid too large");
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(decode_spliced_kernel, grid, dim3(32, 8), 0, (hipStream_t)stream, sr_log_spectro, lr_log_spectro, pha,
                     norm_min_max, spec, (int)F, (int)M, channels, keep_rows, fade_rows, min_value, scale, 0);
  return p2phd::check_launch("spectro_decode_spliced");
}

extern "C" int p2phd_spectro_range(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha, float min_value,
                                   float* minmax_io, float* partials, void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_range: bad geometry");
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_range: channels must be 2 (explicit encoding) or 1, got %d", channels);
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(spec && minmax_io && partials, "spectro_range: null pointer");
  const long n = (long)(B * F * M);
  if (channels == 2) launch_range<2>(spec, n, alpha, min_value, minmax_io, partials, (hipStream_t)stream);
  else launch_range<1>(spec, n, alpha, min_value, minmax_io, partials, (hipStream_t)stream);
  ++p2phd::g_launch_count[p2phd::LC_NORMSCOPE];
  return p2phd::check_launch("spectro_range");
}

extern "C" int p2phd_range_fold(const float* x, int64_t n, float* minmax_io, float* partials, void* stream) {
  P2PHD_REQUIRE(n >= 0, "range_fold: bad length %lld", (long long)n);
  if (n == 0) return P2PHD_OK;
  P2PHD_REQUIRE(x && minmax_io && partials, "range_fold: null pointer");
  launch_range<0>(x, (long)n, 0.f, 0.f, minmax_io, partials, (hipStream_t)stream);
  ++p2phd::g_launch_count[p2phd::LC_NORMSCOPE];
  return p2phd::check_launch("range_fold");
}

extern "C" int p2phd_spectro_encode_given(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha,
                                          float min_value, int mask_rows, int mask_mode, const float* noise,
                                          const float* noise_sign, const float* norm8, float* log_spectro, float* pha,
                                          void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_encode_given: bad geometry");
  P2PHD_REQUIRE(mask_rows >= 0 && mask_rows <= M, "spectro_encode_given: mask_rows %d outside [0, %lld]", mask_rows, (long long)M);
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_encode_given: channels must be 2 (explicit encoding) or 1, got %d", channels);
  P2PHD_REQUIRE(mask_mode >= 0 && mask_mode <= 2, "spectro_encode_given: mask_mode must be 0, 1 or 2, got %d", mask_mode);
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(spec && log_spectro && pha && norm8, "spectro_encode_given: null pointer");
  P2PHD_REQUIRE(!(mask_mode == 1 && noise != nullptr && mask_rows > 0 && noise_sign == nullptr),
                "spectro_encode_given: mask mode1 needs the sign tensor");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_encode_given: grid too large");
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(encode_given_kernel, grid, dim3(32, 8), 0, (hipStream_t)stream, spec, norm8, mask_rows > 0 ? noise : nullptr,
                     noise_sign, log_spectro, pha, (int)F, (int)M, alpha, min_value, channels, mask_rows, mask_mode, 0);
  ++p2phd::g_launch_count[p2phd::LC_NORMSCOPE];
  return p2phd::check_launch("spectro_encode_given");
}

extern "C" int64_t p2phd_spectro_rows_partials_floats(int64_t B, int64_t F, int64_t M) {
  if (B < 0 || F < 1 || M < 1) return 0;
  return 4 * B * rows_chunks(F, M);
}

extern "C" int p2phd_spectro_encode_rows(const float* spec, int64_t B, int64_t F, int64_t M, int channels, float alpha,
                                         float min_value, int mask_rows, int mask_mode, const float* noise,
                                         const float* noise_sign, float* norm_rows, float* log_spectro, float* pha,
                                         float* workspace, void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_encode_rows: bad geometry");
  P2PHD_REQUIRE(mask_rows >= 0 && mask_rows <= M, "spectro_encode_rows: mask_rows %d outside [0, %lld]", mask_rows, (long long)M);
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_encode_rows: channels must be 2 (explicit encoding) or 1, got %d", channels);
  P2PHD_REQUIRE(mask_mode >= 0 && mask_mode <= 2, "spectro_encode_rows: mask_mode must be 0, 1 or 2, got %d", mask_mode);
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(spec && norm_rows && log_spectro && pha && workspace, "spectro_encode_rows: null pointer");
  P2PHD_REQUIRE(!(mask_mode == 1 && noise != nullptr && mask_rows > 0 && noise_sign == nullptr),
                "spectro_encode_rows: mask mode1 needs the sign tensor");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_encode_rows: grid too large");
  hipStream_t st = (hipStream_t)stream;
  if (mask_rows == 0) noise = nullptr;
  const int chunks = rows_chunks(F, M);
  const long n = (long)(F * M), nn = (long)channels * mask_rows * F;
  if (channels == 2)
    hipLaunchKernelGGL(rows_stats_kernel<2>, dim3(chunks, (unsigned)B), dim3(256), 0, st, spec, n, noise, nn, alpha, min_value, workspace);
  else
    hipLaunchKernelGGL(rows_stats_kernel<1>, dim3(chunks, (unsigned)B), dim3(256), 0, st, spec, n, noise, nn, alpha, min_value, workspace);
  hipLaunchKernelGGL(rows_fold_kernel, dim3((unsigned)B), dim3(64), 0, st, workspace, chunks, norm_rows);
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(encode_given_kernel, grid, dim3(32, 8), 0, st, spec, norm_rows, noise, noise_sign, log_spectro, pha, (int)F, (int)M,
                     alpha, min_value, channels, mask_rows, mask_mode, 8);
  ++p2phd::g_launch_count[p2phd::LC_NORMROWS];
  return p2phd::check_launch("spectro_encode_rows");
}

extern "C" int p2phd_spectro_decode_signed_rows(const float* log_spectro, const float* pha, const float* norm_rows, int64_t B,
                                                int64_t F, int64_t M, int channels, int keep_rows, float min_value, float scale,
                                                float* spec, void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_decode_signed_rows: bad geometry");
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_decode_signed_rows: channels must be 1 or 2, got %d", channels);
  P2PHD_REQUIRE(keep_rows >= 0 && keep_rows <= M, "spectro_decode_signed_rows: keep_rows %d outside [0, %lld]", keep_rows, (long long)M);
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(log_spectro && pha && norm_rows && spec, "spectro_decode_signed_rows: null pointer");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_decode_signed_rows: grid too large");
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(decode_signed_kernel, grid, dim3(32, 8), 0, (hipStream_t)stream, log_spectro, pha, norm_rows, spec, (int)F,
                     (int)M, channels, keep_rows, min_value, scale, 8);
  ++p2phd::g_launch_count[p2phd::LC_NORMROWS];
  return p2phd::check_launch("spectro_decode_signed_rows");
}

extern "C" int p2phd_spectro_decode_spliced_rows(const float* sr_log_spectro, const float* lr_log_spectro, const float* pha,
                                                 const float* norm_rows, int64_t B, int64_t F, int64_t M, int channels,
                                                 int keep_rows, int fade_rows, float min_value, float scale, float* spec,
                                                 void* stream) {
  P2PHD_REQUIRE(B >= 0 && F >= 1 && M >= 1, "spectro_decode_spliced_rows: bad geometry");
  P2PHD_REQUIRE(channels == 1 || channels == 2, "spectro_decode_spliced_rows: channels must be 1 or 2, got %d", channels);
  P2PHD_REQUIRE(keep_rows >= 0 && keep_rows <= M, "spectro_decode_spliced_rows: keep_rows %d outside [0, %lld]", keep_rows, (long long)M);
  P2PHD_REQUIRE(fade_rows >= 0 && fade_rows <= keep_rows, "spectro_decode_spliced_rows: fade_rows %d outside [0, keep_rows = %d]",
                fade_rows, keep_rows);
  if (B == 0) return P2PHD_OK;
  P2PHD_REQUIRE(sr_log_spectro && lr_log_spectro && pha && norm_rows && spec, "spectro_decode_spliced_rows: null pointer");
  P2PHD_REQUIRE(B < 65536 && (F + 31) / 32 < 65536, "spectro_decode_spliced_rows: grid too large");
  dim3 grid((unsigned)((M + 31) / 32), (unsigned)((F + 31) / 32), (unsigned)B);
  hipLaunchKernelGGL(decode_spliced_kernel, grid, dim3(32, 8), 0, (hipStream_t)stream, sr_log_spectro, lr_log_spectro, pha,
                     norm_rows, spec, (int)F, (int)M, channels, keep_rows, fade_rows, min_value, scale, 8);
  ++p2phd::g_launch_count[p2phd::LC_NORMROWS];
  return p2phd::check_launch("spectro_decode_spliced_rows");
}
