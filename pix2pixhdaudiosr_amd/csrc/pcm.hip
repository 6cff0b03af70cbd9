// Whole-file generation (pix2pixhdaudiosr_amd/generate.py): the PCM codec at the two ends of the file path, so that a file
// costs one copy of its payload to the device and one copy of the encoded payload back, with no per-sample host work.
//
//   decode  little-endian interleaved payload of a RIFF data chunk -> planar fp32 out[c * ld + n].  One int -> float
//           conversion and an exact power-of-two scale (data/wavio.py load), so the result is the bits wavio.load returns.
//   encode  planar fp32 -> interleaved payload: PCM16 / PCM24 (clamp, scale, round half to even; NaN -> 0) or a float32 bit copy.
//
// Streaming kernels, one thread per sample of the interleaved stream: the payload side is contiguous across a wave, the
// planar side is `channels` contiguous runs.  The payload pointer has byte alignment only (24-bit samples, a data chunk
// at any file offset): typed loads / stores where the pointer is aligned to the sample size, byte accesses otherwise.
#include "common.h"
#include "convplan.h"
#include <algorithm>
#include <cstdint>

namespace {
constexpr int kThreads = 256;

template <int BYTES> __device__ __forceinline__ uint64_t load_le(const uint8_t* __restrict__ p, int aligned) {
  if (BYTES == 1) return p[0];
  if (aligned) {
    if (BYTES == 2) return *reinterpret_cast<const uint16_t*>(p);
    if (BYTES == 4) return *reinterpret_cast<const uint32_t*>(p);
    if (BYTES == 8) return *reinterpret_cast<const uint64_t*>(p);
  }
  uint64_t v = 0;
#pragma unroll
  for (int b = 0; b < BYTES; ++b) v |= (uint64_t)p[b] << (8 * b);
  return v;
}

template <int BYTES> __device__ __forceinline__ void store_le(uint8_t* __restrict__ p, uint32_t v, int aligned) {
  if (aligned && BYTES == 2) { *reinterpret_cast<uint16_t*>(p) = (uint16_t)v; return; }
  if (aligned && BYTES == 4) { *reinterpret_cast<uint32_t*>(p) = v; return; }
#pragma unroll
  for (int b = 0; b < BYTES; ++b) p[b] = (uint8_t)(v >> (8 * b));
}

// FORMAT: the P2PHD_PCM_* codes of include/p2phd.h
template <int FORMAT> __device__ __forceinline__ uint32_t decode_one(const uint8_t* __restrict__ p, int aligned) {
  if (FORMAT == P2PHD_PCM_U8) return __float_as_uint(((float)(int)load_le<1>(p, 1) - 128.0f) * (1.0f / 128.0f));
  if (FORMAT == P2PHD_PCM_S16) return __float_as_uint((float)(int16_t)load_le<2>(p, aligned) * (1.0f / 32768.0f));
  if (FORMAT == P2PHD_PCM_S24) return __float_as_uint((float)((int32_t)((uint32_t)load_le<3>(p, 0) << 8) >> 8) * (1.0f / 8388608.0f));
  if (FORMAT == P2PHD_PCM_S32) return __float_as_uint((float)(int32_t)load_le<4>(p, aligned) * (1.0f / 2147483648.0f));
  if (FORMAT == P2PHD_PCM_F32) return (uint32_t)load_le<4>(p, aligned);                    // bit copy: a NaN keeps its payload
  return __float_as_uint((float)__longlong_as_double((long long)load_le<8>(p, aligned)));  // round to nearest even
}

template <int FORMAT, int BYTES>
__global__ __launch_bounds__(kThreads) void pcm_decode_kernel(const uint8_t* __restrict__ src, long frames, long channels, long ld,
                                                              uint32_t* __restrict__ out, int aligned) {
  const long total = frames * channels;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long n = e / channels, c = e - n * channels;
    out[c * ld + n] = decode_one<FORMAT>(src + e * BYTES, aligned);
  }
}

// clamp to [-1, (2^(bits-1) - 1) / 2^(bits-1)], times 2^(bits-1) (exact), round half to even; NaN -> 0
template <int BITS> __device__ __forceinline__ uint32_t quantise(float x) {
  constexpr float scale = (float)(1u << (BITS - 1));
  constexpr float hi = (scale - 1.0f) / scale;
  if (x != x) return 0u;
  x = fminf(fmaxf(x, -1.0f), hi);
  return (uint32_t)(int32_t)rintf(x * scale);
}

template <int FORMAT, int BYTES>
__global__ __launch_bounds__(kThreads) void pcm_encode_kernel(const uint32_t* __restrict__ planar, long frames, long channels, long ld,
                                                              uint8_t* __restrict__ out, int aligned) {
  const long total = frames * channels;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long n = e / channels, c = e - n * channels;
    const uint32_t bits = planar[c * ld + n];
    uint32_t v;
    if (FORMAT == P2PHD_PCM_S16) v = quantise<16>(__uint_as_float(bits));
    else if (FORMAT == P2PHD_PCM_S24) v = quantise<24>(__uint_as_float(bits));
    else v = bits;
    store_le<BYTES>(out + e * BYTES, v, aligned);
  }
}

int sample_grid(int64_t samples) { return (int)std::max<int64_t>(1, std::min<int64_t>(p2phd::cdiv(samples, kThreads), 16384)); }

template <int FORMAT, int BYTES>
void launch_decode(const void* bytes, int64_t frames, int channels, float* out, int64_t ld, hipStream_t st) {
  const int aligned = (reinterpret_cast<uintptr_t>(bytes) & (BYTES - 1)) == 0 && (BYTES & (BYTES - 1)) == 0;
  hipLaunchKernelGGL((pcm_decode_kernel<FORMAT, BYTES>), dim3(sample_grid(frames * channels)), dim3(kThreads), 0, st,
                     static_cast<const uint8_t*>(bytes), (long)frames, (long)channels, (long)ld, reinterpret_cast<uint32_t*>(out), aligned);
}

template <int FORMAT, int BYTES>
void launch_encode(const float* planar, int64_t frames, int channels, int64_t ld, void* out, hipStream_t st) {
  const int aligned = (reinterpret_cast<uintptr_t>(out) & (BYTES - 1)) == 0 && (BYTES & (BYTES - 1)) == 0;
  hipLaunchKernelGGL((pcm_encode_kernel<FORMAT, BYTES>), dim3(sample_grid(frames * channels)), dim3(kThreads), 0, st,
                     reinterpret_cast<const uint32_t*>(planar), (long)frames, (long)channels, (long)ld, static_cast<uint8_t*>(out), aligned);
}

}  // namespace

extern "C" int p2phd_pcm_decode(const void* bytes, int64_t frames, int channels, int format, float* out, int64_t ld, void* stream) {
  P2PHD_REQUIRE(frames >= 0 && channels >= 1 && channels <= 65535, "pcm_decode: need frames >= 0 and 1 <= channels <= 65535 (frames %lld, channels %d)",
                (long long)frames, channels);
  P2PHD_REQUIRE(format >= P2PHD_PCM_U8 && format <= P2PHD_PCM_F64, "pcm_decode: unknown format %d", format);
  P2PHD_REQUIRE(ld >= frames, "pcm_decode: ld %lld is shorter than the %lld frames of a row", (long long)ld, (long long)frames);
  P2PHD_REQUIRE(frames <= (int64_t(1) << 40) / channels, "pcm_decode: frames * channels too large");
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes && out, "pcm_decode: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "pcm_decode: out is not aligned to a float");
  hipStream_t st = (hipStream_t)stream;
  switch (format) {
    case P2PHD_PCM_U8:  launch_decode<P2PHD_PCM_U8, 1>(bytes, frames, channels, out, ld, st); break;
    case P2PHD_PCM_S16: launch_decode<P2PHD_PCM_S16, 2>(bytes, frames, channels, out, ld, st); break;
    case P2PHD_PCM_S24: launch_decode<P2PHD_PCM_S24, 3>(bytes, frames, channels, out, ld, st); break;
    case P2PHD_PCM_S32: launch_decode<P2PHD_PCM_S32, 4>(bytes, frames, channels, out, ld, st); break;
    case P2PHD_PCM_F32: launch_decode<P2PHD_PCM_F32, 4>(bytes, frames, channels, out, ld, st); break;
    default:            launch_decode<P2PHD_PCM_F64, 8>(bytes, frames, channels, out, ld, st); break;
  }
  ++p2phd::g_launch_count[p2phd::LC_PCM];
  return p2phd::check_launch("pcm_decode");
}

extern "C" int p2phd_pcm_encode(const float* planar, int64_t frames, int channels, int64_t ld, int format, void* out, void* stream) {
  P2PHD_REQUIRE(frames >= 0 && channels >= 1 && channels <= 65535, "pcm_encode: need frames >= 0 and 1 <= channels <= 65535 (frames %lld, channels %d)",
                (long long)frames, channels);
  P2PHD_REQUIRE(format == P2PHD_PCM_S16 || format == P2PHD_PCM_S24 || format == P2PHD_PCM_F32,
                "pcm_encode: format %d is not one of PCM16, PCM24, float32", format);
  P2PHD_REQUIRE(ld >= frames, "pcm_encode: ld %lld is shorter than the %lld frames of a row", (long long)ld, (long long)frames);
  P2PHD_REQUIRE(frames <= (int64_t(1) << 40) / channels, "pcm_encode: frames * channels too large");
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(planar && out, "pcm_encode: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(planar) & 3) == 0, "pcm_encode: planar is not aligned to a float");
  hipStream_t st = (hipStream_t)stream;
  switch (format) {
    case P2PHD_PCM_S16: launch_encode<P2PHD_PCM_S16, 2>(planar, frames, channels, ld, out, st); break;
    case P2PHD_PCM_S24: launch_encode<P2PHD_PCM_S24, 3>(planar, frames, channels, ld, out, st); break;
    default:            launch_encode<P2PHD_PCM_F32, 4>(planar, frames, channels, ld, out, st); break;
  }
  ++p2phd::g_launch_count[p2phd::LC_PCM];
  return p2phd::check_launch("pcm_encode");
}
