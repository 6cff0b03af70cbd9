// Whole-file generation (pix2pixhdaudiosr_amd/generate/): the two ends of the waveform -> segments -> generator -> segments ->
// waveform path that are not a transform or a conv.
//
//   gather  audio[L] -> seg[S,T], seg[s,i] = audio[s * stride + i], zero beyond L.  stride = T is the reference's
//           seg_pad_audio (data/audio_dataset.py:124-135); stride < T makes neighbouring segments share V = T - stride samples.
//   stitch  seg[S,T] -> out[L_out]: each sample from the one or two segments that cover it.  Inside an overlap the later
//           segment fades in with w = sin^2(pi (i + 1/2) / (2 V)) and the earlier one fades out with 1 - w; V = 0 is the
//           reference's torch.cat(...).view(1, -1) times `gain`.
//
// The `_planar` entries run the same two kernels over C rows in one launch each (blockIdx.y = row): audio[C][ld] -> seg[C*S][T],
// channel-major, and seg[C*S][T] -> out[C][ld].  A row goes through the code of the single-row entries, which are the C = 1 case.
//
// Both are streaming kernels (one pass, no reuse, no atomics): one thread per four consecutive outputs, 16-byte accesses
// where the addresses allow.  The cross-fade is evaluated in double and rounded once, so an output is the correctly rounded
// value of the formula whatever the two operands' signs (a float evaluation loses bits where they cancel); the fp64 sine
// runs on at most half of the samples of a kernel that is a few microseconds long.
#include "common.h"
#include "convplan.h"
#include "streamgrid.h"
#include <algorithm>
#include <cstdint>

namespace {
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void segments_gather_kernel(const float* __restrict__ audio, long L, long T, long stride,
                                                                   long total, float* __restrict__ out, int vec4, long ld) {
  audio += (long)blockIdx.y * ld;                                 // row of a planar clip; its segments follow the previous row's
  out += (long)blockIdx.y * total;
  const long quads = (total + 3) >> 2;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
    const long e0 = q << 2;
    if (vec4) {                                                   // T, stride multiples of 4: a quad stays in one row, 16-byte aligned
      const long s = e0 / T, src = s * stride + (e0 - s * T);
      float4 v;
      if (src + 4 <= L) {
        v = *reinterpret_cast<const float4*>(audio + src);
      } else {
        v.x = src < L ? audio[src] : 0.f;
        v.y = src + 1 < L ? audio[src + 1] : 0.f;
        v.z = src + 2 < L ? audio[src + 2] : 0.f;
        v.w = 0.f;
      }
      *reinterpret_cast<float4*>(out + e0) = v;
    } else {
      const long n = min(4l, total - e0);
      for (long j = 0; j < n; ++j) {
        const long e = e0 + j, s = e / T, src = s * stride + (e - s * T);
        out[e] = src < L ? audio[src] : 0.f;
      }
    }
  }
}

__device__ __forceinline__ float stitch_one(const float* __restrict__ seg, long n, long S, long T, long stride, long V, double gain,
                                            double step) {
  const long a = min(n / stride, S - 1);                          // the latest segment that covers n
  const long i = n - a * stride;
  const double cur = (double)seg[a * T + i];
  if (a == 0 || i >= V) return (float)(gain * cur);
  const double sn = sin(((double)i + 0.5) * step);
  const double w = sn * sn;
  return (float)(gain * (w * cur + (1.0 - w) * (double)seg[(a - 1) * T + i + stride]));
}

__global__ __launch_bounds__(kThreads) void segments_stitch_kernel(const float* __restrict__ seg, long S, long T, long stride, long V,
                                                                   float gain, float* __restrict__ out, long L_out, int vec4, long ld) {
  seg += (long)blockIdx.y * S * T;
  out += (long)blockIdx.y * ld;
  const long quads = (L_out + 3) >> 2;
  const double step = V > 0 ? 3.14159265358979323846 / (2.0 * (double)V) : 0.0;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
    const long n0 = q << 2;
    if (vec4 && n0 + 4 <= L_out) {
      const long a = min(n0 / stride, S - 1), i0 = n0 - a * stride;
      const long src = a * T + i0;
      float4 v;
      if ((a == 0 || i0 >= V) && a == min((n0 + 3) / stride, S - 1) && (src & 3) == 0) {     // plain run of one segment
        v = *reinterpret_cast<const float4*>(seg + src);
        v.x *= gain; v.y *= gain; v.z *= gain; v.w *= gain;
      } else {
        v.x = stitch_one(seg, n0, S, T, stride, V, gain, step);
        v.y = stitch_one(seg, n0 + 1, S, T, stride, V, gain, step);
        v.z = stitch_one(seg, n0 + 2, S, T, stride, V, gain, step);
        v.w = stitch_one(seg, n0 + 3, S, T, stride, V, gain, step);
      }
      *reinterpret_cast<float4*>(out + n0) = v;
    } else {
      for (long n = n0; n < min(n0 + 4, L_out); ++n) out[n] = stitch_one(seg, n, S, T, stride, V, gain, step);
    }
  }
}

int stream_grid(int64_t elems) { return p2phd::stream_grid_of(p2phd::SG_STITCH, P2PHD_F32, elems, 1).used; }     // (streamgrid.h)

// every row's first element must be 16-byte aligned for the float4 paths: the bases, and the row pitches when C > 1
bool rows_aligned(const void* a, const void* b, int64_t C, int64_t pitch_a, int64_t pitch_b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 && (C == 1 || ((pitch_a | pitch_b) & 3) == 0);
}

int gather_rows(const char* what, const float* audio, int64_t C, int64_t ld, int64_t L, int64_t T, int64_t stride, int64_t S, float* out,
                void* stream) {
  P2PHD_REQUIRE(L >= 0 && T >= 1 && S >= 1, "%s: need L >= 0, T >= 1, S >= 1 (L %lld, T %lld, S %lld)", what, (long long)L, (long long)T,
                (long long)S);
  P2PHD_REQUIRE(stride >= 1 && stride <= T, "%s: stride must be in [1, T], got %lld (T %lld)", what, (long long)stride, (long long)T);
  P2PHD_REQUIRE(C >= 1 && C <= 65535 && ld >= L, "%s: need 1 <= C <= 65535 and ld >= L (C %lld, ld %lld, L %lld)", what, (long long)C,
                (long long)ld, (long long)L);
  P2PHD_REQUIRE(S <= (int64_t(1) << 40) / T / C, "%s: C * S * T too large", what);
  P2PHD_REQUIRE(out && (audio || L == 0), "%s: null pointer", what);
  const int vec4 = (T & 3) == 0 && (stride & 3) == 0 && rows_aligned(audio, out, C, ld, S * T);
  hipLaunchKernelGGL(segments_gather_kernel, dim3(stream_grid(S * T), (unsigned)C), dim3(kThreads), 0, (hipStream_t)stream, audio, (long)L,
                     (long)T, (long)stride, (long)(S * T), out, vec4, (long)ld);
  ++p2phd::g_launch_count[p2phd::LC_STITCH];
  return p2phd::check_launch(what);
}

int stitch_rows(const char* what, const float* seg, int64_t C, int64_t S, int64_t T, int64_t stride, float gain, float* out, int64_t ld,
                int64_t L_out, void* stream) {
  P2PHD_REQUIRE(S >= 1 && T >= 1, "%s: need S >= 1 and T >= 1 (S %lld, T %lld)", what, (long long)S, (long long)T);
  const int64_t V = T - stride;
  P2PHD_REQUIRE(V >= 0 && V <= T / 2, "%s: the overlap T - stride must be in [0, T/2], got %lld (T %lld)", what, (long long)V, (long long)T);
  P2PHD_REQUIRE(C >= 1 && C <= 65535, "%s: need 1 <= C <= 65535, got %lld", what, (long long)C);
  P2PHD_REQUIRE(S <= (int64_t(1) << 40) / T / C, "%s: C * S * T too large", what);
  P2PHD_REQUIRE(L_out >= 0 && L_out <= (S - 1) * stride + T, "%s: L_out %lld is beyond the %lld samples the segments span", what,
                (long long)L_out, (long long)((S - 1) * stride + T));
  P2PHD_REQUIRE(ld >= L_out, "%s: ld %lld is shorter than L_out %lld", what, (long long)ld, (long long)L_out);
  if (L_out == 0) return P2PHD_OK;
  P2PHD_REQUIRE(seg && out, "%s: null pointer", what);
  const int vec4 = rows_aligned(seg, out, C, S * T, ld);
  hipLaunchKernelGGL(segments_stitch_kernel, dim3(stream_grid(L_out), (unsigned)C), dim3(kThreads), 0, (hipStream_t)stream, seg, (long)S,
                     (long)T, (long)stride, (long)V, gain, out, (long)L_out, vec4, (long)ld);
  ++p2phd::g_launch_count[p2phd::LC_STITCH];
  return p2phd::check_launch(what);
}

}  // namespace

extern "C" int p2phd_segments_gather(const float* audio, int64_t L, int64_t T, int64_t stride, int64_t S, float* out, void* stream) {
  return gather_rows("segments_gather", audio, 1, L, L, T, stride, S, out, stream);
}

extern "C" int p2phd_segments_stitch(const float* seg, int64_t S, int64_t T, int64_t stride, float gain, float* out, int64_t L_out,
                                     void* stream) {
  return stitch_rows("segments_stitch", seg, 1, S, T, stride, gain, out, L_out, L_out, stream);
}

extern "C" int p2phd_segments_gather_planar(const float* audio, int64_t C, int64_t ld, int64_t L, int64_t T, int64_t stride, int64_t S,
                                            float* out, void* stream) {
  return gather_rows("segments_gather_planar", audio, C, ld, L, T, stride, S, out, stream);
}

extern "C" int p2phd_segments_stitch_planar(const float* seg, int64_t C, int64_t S, int64_t T, int64_t stride, float gain, float* out,
                                            int64_t ld, int64_t L_out, void* stream) {
  return stitch_rows("segments_stitch_planar", seg, C, S, T, stride, gain, out, ld, L_out, stream);
}
