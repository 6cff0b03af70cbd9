// Evaluation metrics of the generation tail: compute_matrics (util/util.py:133-184, caller generate_audio.py:47-49).
//
//   sr' = (sr - mean(sr)) / std(sr) * std(hr) + mean(hr)     per row, unbiased std            (:139-140)
//   mse = mean((sr' - hr)^2);  snr_x = mean_rows 10 log10(sum hr^2 / sum (x - hr)^2)            (:148-152)
//   lsd = mean_{rows,frames} sqrt(mean_bins (log10(P_hr + 1e-6) - log10(P_sr' + 1e-6))^2)       (:178-182)
// with P = |STFT|^2 of n_fft2 = 2 n_fft, hop2 = 2 hop, a KBD window of 2 win, reflect-centred frames.
//
// Five launches, no host synchronisation, deterministic (per-block partials in fp64, summed by one block):
//   moments -> row constants -> match (+ error partials) -> STFT/LSD -> finalize.
// The STFT transforms hr and sr' together: z = hr + i sr' through ONE n_fft2-point complex Stockham FFT in LDS run by
// the whole workgroup, separated by H[k] = (Z[k] + conj Z[-k]) / 2, S[k] = (Z[k] - conj Z[-k]) / 2i.
//
// The per-row entry (p2phd_audio_metrics_rows) gives the same four figures for every row on its own -- no mean over rows --
// and four more:
//   lsd_lf / lsd_hf: the LSD above with mean_bins taken over k < cut_bin / k >= cut_bin only (same frames, same FFT);
//   ssnr_x = mean_frames clamp(10 log10(Es / (En + eps) + eps), -10, 35),  Es = sum (w hr)^2,  En = sum (w hr - w x)^2,
//            w[i] = 0.5 (1 - cos(2 pi (i + 1) / (W + 1))), frames of W = seg_win samples at f * seg_hop, f < (T - W) / seg_hop,
//            eps = 2^-52, x = sr' (ssnr_sr) or lr (ssnr_lr); NaN when the row holds no frame.
// Seven launches whatever B is: moments -> row constants -> match (the three kernels above) -> STFT/LSD with band
// accumulators -> segment window table -> segmental SNR (one wavefront per frame) -> per-row finalize.  Every partial sum is
// chunked by the row's own length only, so a row's figures do not depend on the rows beside it.
#include "common.h"
#include "convplan.h"
#include "fft_wave.h"
#include <cmath>

namespace {
using namespace p2phd_fft;

constexpr int kThreads = 256;
constexpr int kMaxChunks = 64;

__device__ __forceinline__ double block_sum(double v, double* s_red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// P1[b][chunk][5] = sum sr, sum sr^2, sum hr, sum hr^2, sum (lr - hr)^2
__global__ __launch_bounds__(kThreads) void moments_kernel(const float* __restrict__ hr, const float* __restrict__ lr,
                                                           const float* __restrict__ sr, long T, int chunks, double* __restrict__ P1) {
  __shared__ double s_red[4];
  const long b = blockIdx.y;
  const long per = (T + chunks - 1) / chunks;
  const long lo = blockIdx.x * per, hi = min(T, lo + per);
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
  for (long i = lo + threadIdx.x; i < hi; i += kThreads) {
    const float s = sr[b * T + i], h = hr[b * T + i], d = lr[b * T + i] - h;
    a0 += s; a1 += (double)s * s; a2 += h; a3 += (double)h * h; a4 += (double)d * d;
  }
  double* o = P1 + (b * chunks + blockIdx.x) * 5;
  a0 = block_sum(a0, s_red); a1 = block_sum(a1, s_red); a2 = block_sum(a2, s_red);
  a3 = block_sum(a3, s_red); a4 = block_sum(a4, s_red);
  if (threadIdx.x == 0) { o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3; o[4] = a4; }
}

// ROW[b][6] = mean_sr, std_sr, mean_hr, std_hr, sum hr^2, sum (lr - hr)^2
__global__ __launch_bounds__(64) void row_consts_kernel(const double* __restrict__ P1, long B, long T, int chunks, double* __restrict__ ROW) {
  const long b = (long)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double a[5] = {0, 0, 0, 0, 0};
  for (int c = 0; c < chunks; ++c)
    for (int j = 0; j < 5; ++j) a[j] += P1[(b * chunks + c) * 5 + j];
  const double n = (double)T;
  const double ms = a[0] / n, mh = a[2] / n;
  const double vs = (a[1] - n * ms * ms) / (n - 1.0), vh = (a[3] - n * mh * mh) / (n - 1.0);
  double* o = ROW + b * 6;
  o[0] = ms; o[1] = sqrt(fmax(vs, 0.0)); o[2] = mh; o[3] = sqrt(fmax(vh, 0.0)); o[4] = a[3]; o[5] = a[4];
}

__global__ __launch_bounds__(kThreads) void match_kernel(const float* __restrict__ hr, const float* __restrict__ sr,
                                                         const double* __restrict__ ROW, long T, int chunks,
                                                         float* __restrict__ out, double* __restrict__ P3) {
  __shared__ double s_red[4];
  const long b = blockIdx.y;
  const float ms = (float)ROW[b * 6 + 0], ss = (float)ROW[b * 6 + 1], mh = (float)ROW[b * 6 + 2], sh = (float)ROW[b * 6 + 3];
  const long per = (T + chunks - 1) / chunks;
  const long lo = blockIdx.x * per, hi = min(T, lo + per);
  double acc = 0;
  for (long i = lo + threadIdx.x; i < hi; i += kThreads) {
    const float v = (sr[b * T + i] - ms) / ss * sh + mh;
    out[b * T + i] = v;
    const float d = v - hr[b * T + i];
    acc += (double)d * d;
  }
  acc = block_sum(acc, s_red);
  if (threadIdx.x == 0) P3[b * chunks + blockIdx.x] = acc;
}

// kBands: P4[b][chunk][3] = sum over the chunk's frames of d_all, d_lo (k < cut_bin), d_hi (k >= cut_bin); else P4[b][chunk] = d_all
template <bool kBands>
__global__ __launch_bounds__(kThreads) void lsd_kernel(const float* __restrict__ hr, const float* __restrict__ sr, long T, int n2,
                                                       int hop2, int win2, const float* __restrict__ window2,
                                                       const float* __restrict__ tables, int pad, long frames, int fchunks,
                                                       int cut_bin, double* __restrict__ P4) {
  extern __shared__ float4 smem_raw[];
  __shared__ double s_red[4];
  float2* buf0 = reinterpret_cast<float2*>(smem_raw);
  float2* buf1 = buf0 + n2;
  float2* s_tw = buf1 + n2;
  float* s_win = reinterpret_cast<float*>(s_tw + n2);
  const int tid = threadIdx.x;
  const long b = blockIdx.y;
  const int left = (n2 - win2) >> 1;
  for (int i = tid; i < n2; i += kThreads) {
    s_tw[i] = reinterpret_cast<const float2*>(tables)[i];
    s_win[i] = (i >= left && i < left + win2) ? window2[i - left] : 0.f;
  }
  const long per = (frames + fchunks - 1) / fchunks;
  const long f_lo = blockIdx.x * per, f_hi = min(frames, f_lo + per);
  const float* h = hr + b * T;
  const float* s = sr + b * T;
  const int nbins = (n2 >> 1) + 1;
  double total = 0, total_lo = 0, total_hi = 0;
  __syncthreads();
  for (long f = f_lo; f < f_hi; ++f) {
    for (int n = tid; n < n2; n += kThreads) {
      long i = f * hop2 - pad + n;
      if (i < 0) i = -i;
      if (i >= T) i = 2 * (T - 1) - i;
      const float w = s_win[n];
      buf0[n] = make_float2(w * h[i], w * s[i]);
    }
    __syncthreads();
    const float2* Z = fft_coop(buf0, buf1, s_tw, n2, tid, kThreads);
    double acc = 0, acc_hi = 0;
    for (int k = tid; k < nbins; k += kThreads) {
      const float2 a = Z[k], m = Z[(n2 - k) & (n2 - 1)];
      const float hx = 0.5f * (a.x + m.x), hy = 0.5f * (a.y - m.y);
      const float sx = 0.5f * (a.y + m.y), sy = 0.5f * (m.x - a.x);
      const float d = log10f(hx * hx + hy * hy + 1e-6f) - log10f(sx * sx + sy * sy + 1e-6f);
      if (kBands && k >= cut_bin) acc_hi += (double)d * d;
      else acc += (double)d * d;
    }
    acc = block_sum(acc, s_red);           // also fences Z before the next frame overwrites buf0
    if (kBands) {                          // acc holds the low band here: 1 <= cut_bin <= n2 / 2 leaves neither band empty
      acc_hi = block_sum(acc_hi, s_red);
      total_lo += sqrt(acc / cut_bin);
      total_hi += sqrt(acc_hi / (nbins - cut_bin));
      acc += acc_hi;
    }
    total += sqrt(acc / nbins);
    __syncthreads();
  }
  if (kBands) {
    if (tid == 0) {
      double* o = P4 + (b * fchunks + blockIdx.x) * 3;
      o[0] = total; o[1] = total_lo; o[2] = total_hi;
    }
  } else {
    if (tid == 0) P4[b * fchunks + blockIdx.x] = total;
  }
}

// WIN[i] = 0.5 (1 - cos(2 pi (i + 1) / (W + 1))): the segment window of the segmental SNR, once per call
__global__ __launch_bounds__(kThreads) void seg_window_kernel(int W, double* __restrict__ WIN) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < W) WIN[i] = 0.5 * (1.0 - cos(2.0 * 3.14159265358979323846264338327950288 * (double)(i + 1) / (double)(W + 1)));
}

// One wavefront per frame of W samples at f * H; the four waves of a workgroup take frames f_lo + wave, + 4, ... of chunk
// blockIdx.x.  Es / En in fp64: En -> 0 (x == hr) must reach the upper clamp, not a rounding residue.
// P5[b][chunk][2] = sum over the chunk's frames of the clamped dB value for x = sr', x = lr.
__global__ __launch_bounds__(kThreads) void ssnr_kernel(const float* __restrict__ hr, const float* __restrict__ lr,
                                                        const float* __restrict__ sr, const double* __restrict__ WIN, long T, int W,
                                                        int H, long F, int schunks, double* __restrict__ P5) {
  __shared__ double s_part[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long b = blockIdx.y;
  const float* h = hr + b * T;
  const float* l = lr + b * T;
  const float* s = sr + b * T;
  const long per = (F + schunks - 1) / schunks;
  const long f_lo = blockIdx.x * per, f_hi = min(F, f_lo + per);
  const double eps = 2.220446049250313e-16;                     // 2^-52
  double tot_s = 0, tot_l = 0;
  for (long f = f_lo + wave; f < f_hi; f += 4) {
    const long base = f * H;                                    // base + W <= T by the frame count
    double es = 0, en_s = 0, en_l = 0;
    for (int i = lane; i < W; i += 64) {
      const double w = WIN[i];
      const double wh = w * (double)h[base + i];
      const double ds = wh - w * (double)s[base + i], dl = wh - w * (double)l[base + i];
      es += wh * wh; en_s += ds * ds; en_l += dl * dl;
    }
    for (int o = 32; o > 0; o >>= 1) {
      es += __shfl_down(es, o, 64); en_s += __shfl_down(en_s, o, 64); en_l += __shfl_down(en_l, o, 64);
    }
    if (lane == 0) {
      tot_s += fmin(fmax(10.0 * log10(es / (en_s + eps) + eps), -10.0), 35.0);
      tot_l += fmin(fmax(10.0 * log10(es / (en_l + eps) + eps), -10.0), 35.0);
    }
  }
  if (lane == 0) { s_part[wave][0] = tot_s; s_part[wave][1] = tot_l; }
  __syncthreads();
  if (threadIdx.x < 2)
    P5[(b * schunks + blockIdx.x) * 2 + threadIdx.x] =
        s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

// rows_out[b][8] = mse, snr_sr, snr_lr, lsd, lsd_lf, lsd_hf, ssnr_sr, ssnr_lr; one workgroup per row
__global__ __launch_bounds__(kThreads) void finalize_rows_kernel(const double* __restrict__ ROW, const double* __restrict__ P3,
                                                                 const double* __restrict__ P4, const double* __restrict__ P5,
                                                                 long T, int chunks, long frames, int fchunks, long F, int schunks,
                                                                 float* __restrict__ rows_out) {
  __shared__ double s_red[4];
  const long b = blockIdx.x;
  double e = 0, d[3] = {0, 0, 0}, v[2] = {0, 0};
  for (int c = threadIdx.x; c < chunks; c += kThreads) e += P3[b * chunks + c];
  for (int c = threadIdx.x; c < fchunks; c += kThreads)
    for (int j = 0; j < 3; ++j) d[j] += P4[(b * fchunks + c) * 3 + j];
  for (int c = threadIdx.x; c < schunks; c += kThreads)
    for (int j = 0; j < 2; ++j) v[j] += P5[(b * schunks + c) * 2 + j];
  e = block_sum(e, s_red);
  for (int j = 0; j < 3; ++j) d[j] = block_sum(d[j], s_red);
  for (int j = 0; j < 2; ++j) v[j] = block_sum(v[j], s_red);
  if (threadIdx.x == 0) {
    float* o = rows_out + b * 8;
    o[0] = (float)(e / (double)T);
    o[1] = (float)(10.0 * log10(ROW[b * 6 + 4] / e));
    o[2] = (float)(10.0 * log10(ROW[b * 6 + 4] / ROW[b * 6 + 5]));
    for (int j = 0; j < 3; ++j) o[3 + j] = (float)(d[j] / (double)frames);
    for (int j = 0; j < 2; ++j) o[6 + j] = F >= 1 ? (float)(v[j] / (double)F) : __builtin_nanf("");
  }
}

__global__ __launch_bounds__(kThreads) void finalize_kernel(const double* __restrict__ ROW, const double* __restrict__ P3,
                                                            const double* __restrict__ P4, long B, long T, int chunks, long frames,
                                                            int fchunks, float* __restrict__ result) {
  __shared__ double s_red[4];
  double err_all = 0, snr_s = 0, snr_l = 0, lsd = 0;
  for (long b = threadIdx.x; b < B; b += kThreads) {
    double e = 0;
    for (int c = 0; c < chunks; ++c) e += P3[b * chunks + c];
    err_all += e;
    snr_s += 10.0 * log10(ROW[b * 6 + 4] / e);
    snr_l += 10.0 * log10(ROW[b * 6 + 4] / ROW[b * 6 + 5]);
    for (int c = 0; c < fchunks; ++c) lsd += P4[b * fchunks + c];
  }
  err_all = block_sum(err_all, s_red); snr_s = block_sum(snr_s, s_red);
  snr_l = block_sum(snr_l, s_red); lsd = block_sum(lsd, s_red);
  if (threadIdx.x == 0) {
    result[0] = (float)(err_all / ((double)B * (double)T));
    result[1] = (float)(snr_s / (double)B);
    result[2] = (float)(snr_l / (double)B);
    result[3] = (float)(lsd / ((double)B * (double)frames));
  }
}

struct Plan { int chunks, fchunks; long frames; int pad; };

int make_plan(int64_t B, int64_t T, int n2, int hop2, int win2, int center, Plan* p) {
  P2PHD_REQUIRE(p2phd::is_pow2(n2) && n2 >= 16 && n2 <= 4096, "metrics: STFT length must be a power of two in [16, 4096], got %d", n2);
  P2PHD_REQUIRE(win2 >= 1 && win2 <= n2 && hop2 >= 1, "metrics: bad STFT window %d / hop %d for n_fft %d", win2, hop2, n2);
  P2PHD_REQUIRE(B >= 1 && T >= 2, "metrics: need at least one row of two samples");
  p->pad = center ? n2 / 2 : 0;
  P2PHD_REQUIRE(!center || T > p->pad, "metrics: reflect padding %d needs a longer signal than %lld", p->pad, (long long)T);
  P2PHD_REQUIRE(T + 2 * p->pad >= n2, "metrics: signal of %lld samples shorter than one STFT frame (%d)", (long long)T, n2);
  p->frames = 1 + (T + 2 * p->pad - n2) / hop2;
  p->chunks = (int)std::min<int64_t>(kMaxChunks, p2phd::cdiv(T, 4096));
  int64_t fc = std::max<int64_t>(1, std::min<int64_t>(p->frames, 2048 / std::max<int64_t>(B, 1)));
  p->fchunks = (int)std::min<int64_t>(fc, 1024);
  P2PHD_REQUIRE(B < 65536, "metrics: too many rows");
  return P2PHD_OK;
}

// The per-row entry: the chunk counts follow the row's length alone (never B), so a row's partial sums group the same way
// whatever is beside it.
struct RowsPlan { Plan p; long F; int schunks; };

int make_rows_plan(int64_t B, int64_t T, int n2, int hop2, int win2, int center, int cut_bin, int seg_win, int seg_hop, RowsPlan* r) {
  if (int rc = make_plan(B, T, n2, hop2, win2, center, &r->p)) return rc;
  P2PHD_REQUIRE(cut_bin >= 1 && cut_bin <= n2 / 2, "metrics rows: cut_bin %d outside [1, %d]", cut_bin, n2 / 2);
  P2PHD_REQUIRE(seg_win >= 1 && seg_hop >= 1, "metrics rows: segment window %d / hop %d must be positive", seg_win, seg_hop);
  P2PHD_REQUIRE(seg_win <= (1 << 24), "metrics rows: segment window %d too long", seg_win);
  r->p.fchunks = (int)std::min<int64_t>(r->p.frames, 512);
  r->F = T >= seg_win ? (long)((T - seg_win) / seg_hop) : 0;      // a row shorter than one frame + one hop: NaN, not an error
  r->schunks = (int)std::max<int64_t>(1, std::min<int64_t>(p2phd::cdiv(r->F, 4), 512));
  return P2PHD_OK;
}

template <bool kBands>
void launch_lsd(const Plan& p, int64_t B, int64_t T, int n_fft2, int hop2, int win2, const float* window2, const float* tables,
                const float* hr, const float* sr_matched, int cut_bin, double* P4, hipStream_t st) {
  const size_t lds = (size_t)n_fft2 * (3 * sizeof(float2) + sizeof(float));
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lsd_kernel<kBands>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(lsd_kernel<kBands>, dim3(p.fchunks, (unsigned)B), dim3(kThreads), lds, st, hr, sr_matched, (long)T, n_fft2, hop2,
                     win2, window2, tables, p.pad, p.frames, p.fchunks, cut_bin, P4);
}

}  // namespace

extern "C" size_t p2phd_stft_tables_floats(int n_fft2) { return 2 * (size_t)n_fft2; }

extern "C" int p2phd_stft_tables_fill(int n_fft2, float* host_out) {
  P2PHD_REQUIRE(p2phd::is_pow2(n_fft2) && n_fft2 >= 16 && n_fft2 <= 4096, "stft tables: bad n_fft %d", n_fft2);
  P2PHD_REQUIRE(host_out != nullptr, "stft tables: null output");
  const double pi = 3.14159265358979323846264338327950288;
  for (int j = 0; j < n_fft2; ++j) {
    const double a = -2.0 * pi * j / n_fft2;
    host_out[2 * j] = (float)std::cos(a);
    host_out[2 * j + 1] = (float)std::sin(a);
  }
  return P2PHD_OK;
}

extern "C" size_t p2phd_metrics_workspace_bytes(int64_t B, int64_t T, int n_fft2, int hop2, int win2, int center) {
  Plan p;
  if (make_plan(B, T, n_fft2, hop2, win2, center, &p) != P2PHD_OK) return 0;
  return sizeof(double) * (size_t)B * ((size_t)p.chunks * 6 + 6 + (size_t)p.fchunks);
}

extern "C" int p2phd_audio_metrics(const float* hr, const float* lr, const float* sr, int64_t B, int64_t T, int n_fft2, int hop2,
                                   int win2, const float* window2, const float* tables, int center, float* sr_matched,
                                   float* result4, void* workspace, void* stream) {
  Plan p;
  if (int rc = make_plan(B, T, n_fft2, hop2, win2, center, &p)) return rc;
  P2PHD_REQUIRE(hr && lr && sr && window2 && tables && sr_matched && result4 && workspace, "audio_metrics: null pointer");
  hipStream_t st = (hipStream_t)stream;
  double* P1 = reinterpret_cast<double*>(workspace);
  double* ROW = P1 + (size_t)B * p.chunks * 5;
  double* P3 = ROW + (size_t)B * 6;
  double* P4 = P3 + (size_t)B * p.chunks;
  hipLaunchKernelGGL(moments_kernel, dim3(p.chunks, (unsigned)B), dim3(kThreads), 0, st, hr, lr, sr, (long)T, p.chunks, P1);
  hipLaunchKernelGGL(row_consts_kernel, dim3((unsigned)p2phd::cdiv(B, 64)), dim3(64), 0, st, P1, (long)B, (long)T, p.chunks, ROW);
  hipLaunchKernelGGL(match_kernel, dim3(p.chunks, (unsigned)B), dim3(kThreads), 0, st, hr, sr, ROW, (long)T, p.chunks, sr_matched, P3);
  launch_lsd<false>(p, B, T, n_fft2, hop2, win2, window2, tables, hr, sr_matched, 0, P4, st);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kThreads), 0, st, ROW, P3, P4, (long)B, (long)T, p.chunks, p.frames, p.fchunks, result4);
  return p2phd::check_launch("audio_metrics");
}

extern "C" size_t p2phd_metrics_rows_workspace_bytes(int64_t B, int64_t T, int n_fft2, int hop2, int win2, int center, int cut_bin,
                                                     int seg_win, int seg_hop) {
  RowsPlan r;
  if (make_rows_plan(B, T, n_fft2, hop2, win2, center, cut_bin, seg_win, seg_hop, &r) != P2PHD_OK) return 0;
  return sizeof(double) * ((size_t)B * ((size_t)r.p.chunks * 6 + 6 + (size_t)r.p.fchunks * 3 + (size_t)r.schunks * 2) + (size_t)seg_win);
}

extern "C" int p2phd_audio_metrics_rows(const float* hr, const float* lr, const float* sr, int64_t B, int64_t T, int n_fft2, int hop2,
                                        int win2, const float* window2, const float* tables, int center, int cut_bin, int seg_win,
                                        int seg_hop, float* matched_out, float* rows_out, void* workspace, void* stream) {
  RowsPlan r;
  if (int rc = make_rows_plan(B, T, n_fft2, hop2, win2, center, cut_bin, seg_win, seg_hop, &r)) return rc;
  P2PHD_REQUIRE(hr && lr && sr && window2 && tables && matched_out && rows_out && workspace, "audio_metrics_rows: null pointer");
  const Plan& p = r.p;
  hipStream_t st = (hipStream_t)stream;
  double* P1 = reinterpret_cast<double*>(workspace);
  double* ROW = P1 + (size_t)B * p.chunks * 5;
  double* P3 = ROW + (size_t)B * 6;
  double* P4 = P3 + (size_t)B * p.chunks;
  double* P5 = P4 + (size_t)B * p.fchunks * 3;
  double* WIN = P5 + (size_t)B * r.schunks * 2;
  hipLaunchKernelGGL(moments_kernel, dim3(p.chunks, (unsigned)B), dim3(kThreads), 0, st, hr, lr, sr, (long)T, p.chunks, P1);
  hipLaunchKernelGGL(row_consts_kernel, dim3((unsigned)p2phd::cdiv(B, 64)), dim3(64), 0, st, P1, (long)B, (long)T, p.chunks, ROW);
  hipLaunchKernelGGL(match_kernel, dim3(p.chunks, (unsigned)B), dim3(kThreads), 0, st, hr, sr, ROW, (long)T, p.chunks, matched_out, P3);
  launch_lsd<true>(p, B, T, n_fft2, hop2, win2, window2, tables, hr, matched_out, cut_bin, P4, st);
  hipLaunchKernelGGL(seg_window_kernel, dim3((unsigned)p2phd::cdiv(seg_win, kThreads)), dim3(kThreads), 0, st, seg_win, WIN);
  hipLaunchKernelGGL(ssnr_kernel, dim3(r.schunks, (unsigned)B), dim3(kThreads), 0, st, hr, lr, matched_out, WIN, (long)T, seg_win,
                     seg_hop, r.F, r.schunks, P5);
  hipLaunchKernelGGL(finalize_rows_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, ROW, P3, P4, P5, (long)T, p.chunks, p.frames,
                     p.fchunks, r.F, r.schunks, rows_out);
  p2phd::g_launch_count[p2phd::LC_METRICS_ROWS] += 7;
  return p2phd::check_launch("audio_metrics_rows");
}
