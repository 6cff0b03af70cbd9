// The dither the PCM16 encoders share (pcm.hip: p2phd_pcm_encode_ex; shaper.hip: p2phd_pcm_encode_shaped), include/p2phd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace p2phd {

// TPDF dither of the interleaved sample with global index i, in LSB: the difference of the two 16-bit halves of a hash of
// (seed, i), times 2^-16 -- exact in fp32, in (-1, 1), triangular.  fmix is the 32-bit finaliser of MurmurHash3.
__device__ __forceinline__ uint32_t fmix(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ float tpdf(uint64_t seed, uint64_t i) {
  const uint32_t h = fmix((uint32_t)i ^ fmix((uint32_t)(i >> 32) ^ (uint32_t)seed ^ 0x9E3779B9u) ^ (uint32_t)(seed >> 32));
  return (float)((int)(h & 0xFFFFu) - (int)(h >> 16)) * (1.0f / 65536.0f);
}

}  // namespace p2phd
