// Whole-file generation (pix2pixhdaudiosr_amd/generate/): the PCM codec at the two ends of the file path, so that a file
// costs one copy of its payload to the device and one copy of the encoded payload back, with no per-sample host work.
//
//   decode  little-endian interleaved payload of a RIFF data chunk -> planar fp32 out[c * ld + n].  One int -> float
//           conversion and an exact power-of-two scale (data/wavio.py load), so the result is the bits wavio.load returns.
//           p2phd_pcm_decode_ex: the same for the payloads of AIFF, AU and NIST SPHERE files -- big-endian samples (a byte swap
//           behind the load) and signed 8-bit ones -- which decode to the bits of their WAV twin.
//   encode  planar fp32 -> interleaved payload, one kernel behind both entries: y = x * gain[0] (read from device memory: the
//           peak launch in front needs no host round trip; no gain: y = x), v = y * 2^(bits-1) [+ d], r = rint(v) clamped to
//           the integer range, NaN -> 0; float32 writes y, without gain as a bit copy.  d: TPDF dither of +-1 LSB for PCM16, a
//           counter-based hash of (seed, index of the interleaved sample) -- a payload encoded in pieces, or twice, gets the same
//           bytes.  p2phd_pcm_encode is p2phd_pcm_encode_ex without gain and dither: the bytes wavio.save writes, which clamps
//           in front of the rounding -- the same integer for every float (tests/test_pcm_host.py holds both orders together).
//
// and the output stage in front of the encoder, for a file that must not clip silently (opt-in):
//
//   peak       per channel max |x| over the finite samples, the number of samples the encoder of the format would clamp and
//              the number of NaN / inf samples; one gain for all channels, gain = m > ceiling ? ceiling / m : 1 with m the
//              largest channel peak.  A maximum of bit patterns and integer counts: the same bits on every run.  Workgroup
//              partials are stored and folded by the last workgroup (common.h: fold_arrive_last), so nothing is zeroed before
//              the launch and there is no float atomic.  HBM-bound: 16-byte pieces, four in flight per thread.
//
// Streaming kernels, one thread per sample of the interleaved stream: the payload side is contiguous across a wave, the
// planar side is `channels` contiguous runs.  The payload pointer has byte alignment only (24-bit samples, a data chunk
// at any file offset): typed loads / stores where the pointer is aligned to the sample size, byte accesses otherwise.
#include "common.h"
#include "convplan.h"
#include "dither.h"
#include "streamgrid.h"
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

// ---- big-endian containers (AIFF, AU, NIST SPHERE: data/containers.py) ---------------------------------------------------
// The sample at p as the little-endian load of its WAV twin would return it.  BE: the bytes stand in the other order -- a typed
// load and a byte swap where the payload is aligned to the sample size, byte-wise otherwise (24-bit always), load_le's rule.
template <int BYTES, bool BE> __device__ __forceinline__ uint64_t load_any(const uint8_t* __restrict__ p, int aligned) {
  if (!BE || BYTES == 1) return load_le<BYTES>(p, aligned);
  if (aligned) {
    if (BYTES == 2) return __builtin_bswap16(*reinterpret_cast<const uint16_t*>(p));
    if (BYTES == 4) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(p));
    if (BYTES == 8) return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(p));
  }
  uint64_t v = 0;
#pragma unroll
  for (int b = 0; b < BYTES; ++b) v = (v << 8) | p[b];
  return v;
}

// decode_one's conversions on a loaded sample.  SIGNED8 (U8 only): the byte is s, its twin holds s + 128: s / 128.
template <int FORMAT, bool SIGNED8> __device__ __forceinline__ uint32_t convert_one(uint64_t v) {
  if (FORMAT == P2PHD_PCM_U8) return __float_as_uint((SIGNED8 ? (float)(int8_t)v : (float)(int)v - 128.0f) * (1.0f / 128.0f));
  if (FORMAT == P2PHD_PCM_S16) return __float_as_uint((float)(int16_t)v * (1.0f / 32768.0f));
  if (FORMAT == P2PHD_PCM_S24) return __float_as_uint((float)((int32_t)((uint32_t)v << 8) >> 8) * (1.0f / 8388608.0f));
  if (FORMAT == P2PHD_PCM_S32) return __float_as_uint((float)(int32_t)v * (1.0f / 2147483648.0f));
  if (FORMAT == P2PHD_PCM_F32) return (uint32_t)v;                                         // bit copy: a NaN keeps its payload
  return __float_as_uint((float)__longlong_as_double((long long)v));                      // round to nearest even
}

constexpr int pcm_bytes(int format) {
  return format == P2PHD_PCM_U8 ? 1 : format == P2PHD_PCM_S16 ? 2 : format == P2PHD_PCM_S24 ? 3 : format == P2PHD_PCM_F64 ? 8 : 4;
}

// The grid-stride walk with the payload's alignment known at compile time, two samples of a thread loaded before either is converted.
// pcm_decode_kernel gets both from the compiler (the test of `aligned` moved out of its loop, the loop unrolled by two with the loads in
// front); with the byte swap behind the load it gives neither, and the decoder runs at two thirds of the little-endian rate on an hour.
template <int FORMAT, bool BE, bool SIGNED8, bool ALIGNED>
__device__ __forceinline__ void decode_ex_walk(const uint8_t* __restrict__ src, long total, long channels, long ld, uint32_t* __restrict__ out) {
  constexpr int BYTES = pcm_bytes(FORMAT);
  const long stride = (long)gridDim.x * blockDim.x;
  long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; e + stride < total; e += 2 * stride) {
    const long f = e + stride;
    const uint64_t a = load_any<BYTES, BE>(src + e * BYTES, ALIGNED), b = load_any<BYTES, BE>(src + f * BYTES, ALIGNED);
    const long n = e / channels, c = e - n * channels, m = f / channels, d = f - m * channels;
    out[c * ld + n] = convert_one<FORMAT, SIGNED8>(a);
    out[d * ld + m] = convert_one<FORMAT, SIGNED8>(b);
  }
  if (e < total) {
    const long n = e / channels, c = e - n * channels;
    out[c * ld + n] = convert_one<FORMAT, SIGNED8>(load_any<BYTES, BE>(src + e * BYTES, ALIGNED));
  }
}

// pcm_decode_kernel's walk and layout, templated on (format, byte order, signedness)
template <int FORMAT, bool BE, bool SIGNED8>
__global__ __launch_bounds__(kThreads) void pcm_decode_ex_kernel(const uint8_t* __restrict__ src, long frames, long channels, long ld,
                                                                 uint32_t* __restrict__ out, int aligned) {
  if (aligned) decode_ex_walk<FORMAT, BE, SIGNED8, true>(src, frames * channels, channels, ld, out);
  else decode_ex_walk<FORMAT, BE, SIGNED8, false>(src, frames * channels, channels, ld, out);
}

using p2phd::tpdf;                  // dither.h: the TPDF dither of an interleaved sample, shared with shaper.hip

// y * 2^(bits-1) (exact) [+ d], round half to even, clamp to the integer range; NaN -> 0
template <int BITS, bool DITHER> __device__ __forceinline__ uint32_t quantise(float y, float d) {
  constexpr float scale = (float)(1u << (BITS - 1));
  float v = y * scale;
  if (DITHER) v = v + d;
  if (v != v) return 0u;
  return (uint32_t)(int32_t)fminf(fmaxf(rintf(v), -scale), scale - 1.0f);
}

template <int FORMAT, int BYTES, bool GAIN, bool DITHER>
__global__ __launch_bounds__(kThreads) void pcm_encode_kernel(const uint32_t* __restrict__ planar, long frames, long channels, long ld,
                                                              const float* __restrict__ gain, uint64_t seed, uint64_t first_index,
                                                              uint8_t* __restrict__ out, int aligned) {
  const long total = frames * channels;
  const float g = GAIN ? *gain : 1.0f;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long n = e / channels, c = e - n * channels;
    const uint32_t bits = planar[c * ld + n];
    const float y = GAIN ? __uint_as_float(bits) * g : __uint_as_float(bits);
    const float d = DITHER ? tpdf(seed, first_index + (uint64_t)e) : 0.0f;
    uint32_t v;
    if (FORMAT == P2PHD_PCM_S16) v = quantise<16, DITHER>(y, d);
    else if (FORMAT == P2PHD_PCM_S24) v = quantise<24, false>(y, d);
    else v = GAIN ? __float_as_uint(y) : bits;                 // no gain: a bit copy, a NaN keeps its payload
    store_le<BYTES>(out + e * BYTES, v, aligned);
  }
}

// ---- output stage: peak report and the gain of the clip guard ------------------------------------------------------------
// Peak statistics of one sample (the rare path: a piece that holds a sample above the format's limit or a non-finite one)
template <int FORMAT> __device__ __forceinline__ void peak_tally(uint32_t bits, uint32_t& pk, unsigned long long& ov, unsigned long long& nf) {
  const uint32_t a = bits & 0x7FFFFFFFu;
  const float x = __uint_as_float(bits);
  if (a < 0x7F800000u) pk = max(pk, a); else ++nf;
  if (FORMAT == P2PHD_PCM_F32) ov += fabsf(x) > 1.0f;                                        // (false for NaN, true for +-inf)
  else {
    constexpr float scale = FORMAT == P2PHD_PCM_S16 ? 32768.0f : 8388608.0f;
    ov += (x > (scale - 1.0f) / scale) || (x < -1.0f);
  }
}

constexpr int kPeakWords = 5;      // a workgroup's partial: peak bits, clamped count lo / hi, non-finite count lo / hi
constexpr int kPeakU = 4;          // 16-byte pieces in flight per thread

__device__ __forceinline__ void peak_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t peak_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// grid (gx, channels): workgroup (b, c) walks its share of row c.  A row starts at any float (ld is the caller's): the samples in
// front of the first 16-byte boundary and behind the last whole piece are read one by one by workgroup b = 0.
template <int FORMAT>
__global__ __launch_bounds__(kThreads) void pcm_peak_kernel(const float* __restrict__ planar, long frames, long ld, float ceiling,
                                                            uint32_t* __restrict__ part, unsigned* __restrict__ ticket,
                                                            float* __restrict__ peak, long long* __restrict__ over,
                                                            long long* __restrict__ nonfinite, float* __restrict__ gain) {
  // at or below `limit` (bit pattern of |x|) a sample is finite and inside the format's range: only the maximum is kept
  constexpr uint32_t limit = FORMAT == P2PHD_PCM_S16 ? 0x3F7FFE00u : FORMAT == P2PHD_PCM_S24 ? 0x3F7FFFFEu : 0x3F800000u;
  static_assert(__builtin_bit_cast(uint32_t, 32767.0f / 32768.0f) == 0x3F7FFE00u && __builtin_bit_cast(uint32_t, 8388607.0f / 8388608.0f) == 0x3F7FFFFEu &&
                __builtin_bit_cast(uint32_t, 1.0f) == 0x3F800000u, "limit: the bit patterns of hi and 1");
  __shared__ uint32_t s_pk[kThreads];
  __shared__ unsigned long long s_ov[kThreads], s_nf[kThreads];
  const int tid = threadIdx.x, c = blockIdx.y, gx = gridDim.x, C = gridDim.y;
  const float* row = planar + (long)c * ld;
  const long head = min(frames, (long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2));
  const long pieces = (frames - head) >> 2;
  const long tail0 = head + (pieces << 2);
  const uint4* body = reinterpret_cast<const uint4*>(row + head);
  uint32_t pk = 0u;
  unsigned long long ov = 0ull, nf = 0ull;
  const long stride = (long)gx * kThreads;
  for (long e0 = (long)blockIdx.x * kThreads + tid; e0 < pieces; e0 += kPeakU * stride) {
    uint4 q[kPeakU];
#pragma unroll
    for (int u = 0; u < kPeakU; ++u) q[u] = body[min(e0 + u * stride, pieces - 1)];          // unconditional, clamped
    __builtin_amdgcn_sched_barrier(0);                            // all four requests go out before the first piece is looked at
#pragma unroll
    for (int u = 0; u < kPeakU; ++u) {
      if (e0 + u * stride >= pieces) continue;
      const uint32_t a0 = q[u].x & 0x7FFFFFFFu, a1 = q[u].y & 0x7FFFFFFFu, a2 = q[u].z & 0x7FFFFFFFu, a3 = q[u].w & 0x7FFFFFFFu;
      const uint32_t m = max(max(a0, a1), max(a2, a3));
      if (m <= limit) pk = max(pk, m);
      else {
        peak_tally<FORMAT>(q[u].x, pk, ov, nf); peak_tally<FORMAT>(q[u].y, pk, ov, nf);
        peak_tally<FORMAT>(q[u].z, pk, ov, nf); peak_tally<FORMAT>(q[u].w, pk, ov, nf);
      }
    }
  }
  if (blockIdx.x == 0) {
    if (tid < head) peak_tally<FORMAT>(__float_as_uint(row[tid]), pk, ov, nf);
    if (tid < frames - tail0) peak_tally<FORMAT>(__float_as_uint(row[tail0 + tid]), pk, ov, nf);
  }
  s_pk[tid] = pk; s_ov[tid] = ov; s_nf[tid] = nf;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) { s_pk[tid] = max(s_pk[tid], s_pk[tid + o]); s_ov[tid] += s_ov[tid + o]; s_nf[tid] += s_nf[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    uint32_t* w = part + ((size_t)c * gx + blockIdx.x) * kPeakWords;
    peak_store(w + 0, s_pk[0]);
    peak_store(w + 1, (uint32_t)s_ov[0]); peak_store(w + 2, (uint32_t)(s_ov[0] >> 32));
    peak_store(w + 3, (uint32_t)s_nf[0]); peak_store(w + 4, (uint32_t)(s_nf[0] >> 32));
  }
  if (!p2phd::fold_arrive_last(ticket, (unsigned)(gx * C))) return;
  // the last workgroup: wave w folds channels w, w + 4, ...; a maximum and integer sums do not depend on the order
  __shared__ uint32_t s_max[kThreads / 64];
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t top = 0u;
  for (int ch = wave; ch < C; ch += kThreads / 64) {
    uint32_t p = 0u;
    unsigned long long o = 0ull, f = 0ull;
    for (int b = lane; b < gx; b += 64) {
      const uint32_t* w = part + ((size_t)ch * gx + b) * kPeakWords;
      p = max(p, peak_load(w + 0));
      o += (unsigned long long)peak_load(w + 1) | ((unsigned long long)peak_load(w + 2) << 32);
      f += (unsigned long long)peak_load(w + 3) | ((unsigned long long)peak_load(w + 4) << 32);
    }
    for (int s = 32; s > 0; s >>= 1) {
      p = max(p, (uint32_t)__shfl_xor((int)p, s));
      o += (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)o, s) | ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(o >> 32), s) << 32);
      f += (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)f, s) | ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(f >> 32), s) << 32);
    }
    if (lane == 0) { peak[ch] = __uint_as_float(p); over[ch] = (long long)o; nonfinite[ch] = (long long)f; }
    top = max(top, p);
  }
  if (lane == 0) s_max[wave] = top;
  __syncthreads();
  if (tid == 0) {
    constexpr float own = FORMAT == P2PHD_PCM_S16 ? 32767.0f / 32768.0f : FORMAT == P2PHD_PCM_S24 ? 8388607.0f / 8388608.0f : 1.0f;
    const float m = __uint_as_float(max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
    const float cl = ceiling <= 0.0f ? own : ceiling;
    *gain = m > cl ? cl / m : 1.0f;
  }
}

int sample_grid(int64_t samples) { return p2phd::stream_grid_of(p2phd::SG_PCM, P2PHD_F32, samples, 1).used; }       // (streamgrid.h)

template <int FORMAT, int BYTES>
void launch_decode(const void* bytes, int64_t frames, int channels, float* out, int64_t ld, hipStream_t st) {
  const int aligned = (reinterpret_cast<uintptr_t>(bytes) & (BYTES - 1)) == 0 && (BYTES & (BYTES - 1)) == 0;
  hipLaunchKernelGGL((pcm_decode_kernel<FORMAT, BYTES>), dim3(sample_grid(frames * channels)), dim3(kThreads), 0, st,
                     static_cast<const uint8_t*>(bytes), (long)frames, (long)channels, (long)ld, reinterpret_cast<uint32_t*>(out), aligned);
}

template <int FORMAT, bool BE, bool SIGNED8>
void launch_decode_ex(const void* bytes, int64_t frames, int channels, float* out, int64_t ld, hipStream_t st) {
  constexpr int BYTES = pcm_bytes(FORMAT);
  const int aligned = (reinterpret_cast<uintptr_t>(bytes) & (BYTES - 1)) == 0 && (BYTES & (BYTES - 1)) == 0;
  hipLaunchKernelGGL((pcm_decode_ex_kernel<FORMAT, BE, SIGNED8>), dim3(sample_grid(frames * channels)), dim3(kThreads), 0, st,
                     static_cast<const uint8_t*>(bytes), (long)frames, (long)channels, (long)ld, reinterpret_cast<uint32_t*>(out), aligned);
}

template <int FORMAT>
void launch_decode_order(bool be, const void* bytes, int64_t frames, int channels, float* out, int64_t ld, hipStream_t st) {
  (be ? launch_decode_ex<FORMAT, true, false> : launch_decode_ex<FORMAT, false, false>)(bytes, frames, channels, out, ld, st);
}

template <int FORMAT, int BYTES, bool DITHER>
void launch_encode(const float* planar, int64_t frames, int channels, int64_t ld, const float* gain, uint64_t seed, uint64_t first_index,
                   void* out, hipStream_t st) {
  const int aligned = (reinterpret_cast<uintptr_t>(out) & (BYTES - 1)) == 0 && (BYTES & (BYTES - 1)) == 0;
  const auto kernel = gain ? pcm_encode_kernel<FORMAT, BYTES, true, DITHER> : pcm_encode_kernel<FORMAT, BYTES, false, DITHER>;
  hipLaunchKernelGGL(kernel, dim3(sample_grid(frames * channels)), dim3(kThreads), 0, st, reinterpret_cast<const uint32_t*>(planar),
                     (long)frames, (long)channels, (long)ld, gain, seed, first_index, static_cast<uint8_t*>(out), aligned);
}

// workgroups per row (streamgrid.h, which holds kThreads, kPeakU and kPeakWords as numbers)
static_assert(kThreads == 256 && kPeakU == 4 && kPeakWords == 5, "streamgrid.h, SG_PCM_PEAK");
int peak_grid(int64_t frames, int channels) { return p2phd::stream_grid_of(p2phd::SG_PCM_PEAK, P2PHD_F32, frames, channels).used; }

// The checks every entry shares: the shape of the planar side and the format -- one a data chunk can hold (decode), or one
// of the three an output is written in (`encodable`)
int check_rows(const char* what, int64_t frames, int channels, int64_t ld, int format, bool encodable) {
  P2PHD_REQUIRE(frames >= 0 && channels >= 1 && channels <= 65535, "%s: need frames >= 0 and 1 <= channels <= 65535 (frames %lld, channels %d)", what,
                (long long)frames, channels);
  if (encodable)
    P2PHD_REQUIRE(format == P2PHD_PCM_S16 || format == P2PHD_PCM_S24 || format == P2PHD_PCM_F32, "%s: format %d is not one of PCM16, PCM24, float32",
                  what, format);
  else
    P2PHD_REQUIRE(format >= P2PHD_PCM_U8 && format <= P2PHD_PCM_F64, "%s: unknown format %d", what, format);
  P2PHD_REQUIRE(ld >= frames, "%s: ld %lld is shorter than the %lld frames of a row", what, (long long)ld, (long long)frames);
  P2PHD_REQUIRE(frames <= (int64_t(1) << 40) / channels, "%s: frames * channels too large", what);
  return P2PHD_OK;
}

int encode_rows(const char* what, const float* planar, int64_t frames, int channels, int64_t ld, int format, const float* gain, int dither,
                uint64_t seed, int64_t first_index, void* out, void* stream) {
  if (const int rc = check_rows(what, frames, channels, ld, format, true)) return rc;
  P2PHD_REQUIRE(dither == 0 || (dither == 1 && format == P2PHD_PCM_S16), "%s: dither must be 0, or 1 (TPDF) with PCM16 (dither %d, format %d)", what,
                dither, format);
  P2PHD_REQUIRE(first_index >= 0, "%s: first_index %lld is negative", what, (long long)first_index);
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(planar && out, "%s: null pointer", what);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(planar) & 3) == 0, "%s: planar is not aligned to a float", what);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(gain) & 3) == 0, "%s: planar or gain is not aligned to a float", what);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t first = (uint64_t)first_index;
  switch (format) {
    case P2PHD_PCM_S16: (dither ? launch_encode<P2PHD_PCM_S16, 2, true> : launch_encode<P2PHD_PCM_S16, 2, false>)(planar, frames, channels, ld, gain, seed, first, out, st); break;
    case P2PHD_PCM_S24: launch_encode<P2PHD_PCM_S24, 3, false>(planar, frames, channels, ld, gain, seed, first, out, st); break;
    default:            launch_encode<P2PHD_PCM_F32, 4, false>(planar, frames, channels, ld, gain, seed, first, out, st); break;
  }
  ++p2phd::g_launch_count[p2phd::LC_PCM];
  return p2phd::check_launch(what);
}

}  // namespace

int p2phd::pcm_check_rows(const char* what, int64_t frames, int channels, int64_t ld, int format, bool encodable) {
  return check_rows(what, frames, channels, ld, format, encodable);
}

extern "C" int p2phd_pcm_decode(const void* bytes, int64_t frames, int channels, int format, float* out, int64_t ld, void* stream) {
  if (const int rc = check_rows("pcm_decode", frames, channels, ld, format, false)) return rc;
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

extern "C" int p2phd_pcm_decode_ex(const void* bytes, int64_t frames, int channels, int format, int flags, float* out, int64_t ld,
                                   void* stream) {
  if (const int rc = check_rows("pcm_decode_ex", frames, channels, ld, format, false)) return rc;
  P2PHD_REQUIRE((flags & ~(P2PHD_PCM_BIG_ENDIAN | P2PHD_PCM_SIGNED8)) == 0, "pcm_decode_ex: unknown flag bits in %d", flags);
  P2PHD_REQUIRE(!(flags & P2PHD_PCM_SIGNED8) || format == P2PHD_PCM_U8, "pcm_decode_ex: P2PHD_PCM_SIGNED8 goes with P2PHD_PCM_U8 only (format %d)",
                format);
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes && out, "pcm_decode_ex: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "pcm_decode_ex: out is not aligned to a float");
  hipStream_t st = (hipStream_t)stream;
  const bool be = (flags & P2PHD_PCM_BIG_ENDIAN) != 0;
  switch (format) {
    case P2PHD_PCM_U8:                                            // a byte has no order
      (flags & P2PHD_PCM_SIGNED8 ? launch_decode_ex<P2PHD_PCM_U8, false, true> : launch_decode_ex<P2PHD_PCM_U8, false, false>)(bytes, frames, channels, out, ld, st);
      break;
    case P2PHD_PCM_S16: launch_decode_order<P2PHD_PCM_S16>(be, bytes, frames, channels, out, ld, st); break;
    case P2PHD_PCM_S24: launch_decode_order<P2PHD_PCM_S24>(be, bytes, frames, channels, out, ld, st); break;
    case P2PHD_PCM_S32: launch_decode_order<P2PHD_PCM_S32>(be, bytes, frames, channels, out, ld, st); break;
    case P2PHD_PCM_F32: launch_decode_order<P2PHD_PCM_F32>(be, bytes, frames, channels, out, ld, st); break;
    default:            launch_decode_order<P2PHD_PCM_F64>(be, bytes, frames, channels, out, ld, st); break;
  }
  ++p2phd::g_launch_count[p2phd::LC_PCM];
  return p2phd::check_launch("pcm_decode_ex");
}

extern "C" int p2phd_pcm_encode(const float* planar, int64_t frames, int channels, int64_t ld, int format, void* out, void* stream) {
  return encode_rows("pcm_encode", planar, frames, channels, ld, format, nullptr, 0, 0, 0, out, stream);
}

extern "C" int p2phd_pcm_encode_ex(const float* planar, int64_t frames, int channels, int64_t ld, int format, const float* gain, int dither,
                                   uint64_t seed, int64_t first_index, void* out, void* stream) {
  return encode_rows("pcm_encode_ex", planar, frames, channels, ld, format, gain, dither, seed, first_index, out, stream);
}

extern "C" int p2phd_pcm_peak(const float* planar, int64_t frames, int channels, int64_t ld, int format, float ceiling, float* peak,
                              int64_t* over, int64_t* nonfinite, float* gain, void* stream) {
  if (const int rc = check_rows("pcm_peak", frames, channels, ld, format, true)) return rc;
  P2PHD_REQUIRE(peak && over && nonfinite && gain, "pcm_peak: null output pointer");
  P2PHD_REQUIRE(frames == 0 || planar, "pcm_peak: null pointer");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(planar) & 3) == 0, "pcm_peak: planar is not aligned to a float");
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(over) & 7) == 0 && (reinterpret_cast<uintptr_t>(nonfinite) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(peak) & 3) == 0 && (reinterpret_cast<uintptr_t>(gain) & 3) == 0, "pcm_peak: an output is not aligned to its type");
  hipStream_t st = (hipStream_t)stream;
  const p2phd::FoldScratch fs = p2phd::fold_scratch(p2phd::FOLD_PCM, st);
  if (fs.part == nullptr) return P2PHD_EINVAL;                   // (refused: error text set by fold_scratch)
  P2PHD_REQUIRE(fs.floats >= (size_t)kPeakWords * channels, "pcm_peak: reduction scratch too small for %d channels", channels);
  // frames = 0 launches too: the outputs (zeros, gain 1) are valid after every call
  const dim3 grid(peak_grid(frames, channels), channels);
  uint32_t* part = reinterpret_cast<uint32_t*>(fs.part);
  long long* ov = reinterpret_cast<long long*>(over);
  long long* nf = reinterpret_cast<long long*>(nonfinite);
  switch (format) {
    case P2PHD_PCM_S16: hipLaunchKernelGGL(pcm_peak_kernel<P2PHD_PCM_S16>, grid, dim3(kThreads), 0, st, planar, (long)frames, (long)ld, ceiling, part, fs.ticket, peak, ov, nf, gain); break;
    case P2PHD_PCM_S24: hipLaunchKernelGGL(pcm_peak_kernel<P2PHD_PCM_S24>, grid, dim3(kThreads), 0, st, planar, (long)frames, (long)ld, ceiling, part, fs.ticket, peak, ov, nf, gain); break;
    default:            hipLaunchKernelGGL(pcm_peak_kernel<P2PHD_PCM_F32>, grid, dim3(kThreads), 0, st, planar, (long)frames, (long)ld, ceiling, part, fs.ticket, peak, ov, nf, gain); break;
  }
  ++p2phd::g_launch_count[p2phd::LC_PCM];
  return p2phd::check_launch("pcm_peak");
}
