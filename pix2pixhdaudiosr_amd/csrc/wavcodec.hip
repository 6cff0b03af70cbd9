// Coded WAV input ("Coded WAV input" of include/p2phd.h): G.711 mu-law / A-law and 4-bit IMA ADPCM data chunks, for the feeder (host)
// and for whole-file generation (device).  Launch family "wavcodec".
//
//   host    p2phd_g711_decode_host     interleaved bytes -> planar f32
//           p2phd_ima_frames           the frames a payload holds
//           p2phd_ima_decode_host      a window of frames: only the covering blocks are read
//           p2phd_ima_scan_host        the first block with a step index above 88
//   device  p2phd_g711_decode          g711_decode_kernel: element-wise; from the payload's first 16-byte boundary on a lane reads 16 bytes
//                                      at once, the few bytes in front of it and behind the last whole piece go one by one
//           p2phd_ima_decode           ima_decode_kernel: the recursion is sequential inside a block and blocks are independent, so the
//                                      unit is one (block, channel) chain.  A workgroup stages the bytes of its blocks into LDS with
//                                      coalesced 4-byte reads, transposed so that word w of chain i lies at w * S + i (S odd: neither the
//                                      staging writes nor the lanes' reads collide on a bank); one lane runs one chain from LDS and
//                                      stores each group's 8 samples.  The grid is capped; a workgroup walks tiles b, b + grid, ...
//
// Both sides decode through ONE set of routines (g711_one, ima_header, ima_group: __host__ __device__).  The step table is an argument:
// the host's array, or the workgroup's copy of it in LDS (a lane's index is its own: LDS, not scratch).  The header's step index is
// clamped where it is loaded, so no byte stream indexes past the table.
#include "common.h"
#include "convplan.h"
#include <algorithm>
#include <cstdint>
#include <cstring>

#define WHD __host__ __device__ __forceinline__

namespace {
constexpr int kThreads = 256;
constexpr int kSteps = 89;
constexpr int kMaxChannels = 8;
constexpr int64_t kG711Grid = 2048;            // workgroups of g711_decode_kernel at most
constexpr int kImaGrid = 1024;                 // workgroups of ima_decode_kernel at most
constexpr int kImaLdsBytes = 32768;            // LDS of a workgroup that stages more than one block (one block: its block_align, < 64 KiB)
constexpr int kImaMaxAlignDev = 65536 - 512;   // the largest block the device decoder stages: 64 KiB of LDS less the step table
constexpr float kScale = 1.0f / 32768.0f;

// the 89 steps of IMA ADPCM
#define P2PHD_IMA_STEPS                                                                                                                  \
  7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,  \
  173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,     \
  1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635,       \
  13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767
const int32_t kStepHost[kSteps] = {P2PHD_IMA_STEPS};
__device__ const int32_t kStepDev[kSteps] = {P2PHD_IMA_STEPS};

// ---- the routines both sides call --------------------------------------------------------------------------------------------
WHD int32_t g711_one(uint32_t b, int law) {
  if (law == P2PHD_G711_ULAW) {
    const uint32_t u = ~b & 0xFFu;
    const int32_t e = (int32_t)((u >> 4) & 7u), m = (int32_t)(u & 15u);
    const int32_t mag = (((m << 3) + 0x84) << e) - 0x84;
    return (u & 0x80u) ? -mag : mag;
  }
  const uint32_t a = (b ^ 0x55u) & 0xFFu;
  const int32_t e = (int32_t)((a >> 4) & 7u), m = (int32_t)(a & 15u);
  const int32_t mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
  return (a & 0x80u) ? mag : -mag;
}

WHD float pcm16_scale(int32_t v) { return (float)v * kScale; }

// the 4-byte header of a chain as a little-endian word: predictor (the block's first sample), step index clamped to the table
WHD void ima_header(uint32_t word, int32_t& pred, int32_t& index) {
  pred = (int32_t)(int16_t)(word & 0xFFFFu);
  const int32_t i = (int32_t)((word >> 16) & 0xFFu);
  index = i > kSteps - 1 ? kSteps - 1 : i;
}

// the 8 nibbles of a chain's group as a little-endian word, low nibble of each byte first: nibble k is bits [4k, 4k + 4)
WHD void ima_group(const int32_t* __restrict__ step, uint32_t word, int32_t& pred, int32_t& index, int32_t (&out)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t n = (word >> (4 * k)) & 15u;
    const int32_t st = step[index];
    int32_t d = st >> 3;
    if (n & 1u) d += st >> 2;
    if (n & 2u) d += st >> 1;
    if (n & 4u) d += st;
    pred = (n & 8u) ? pred - d : pred + d;
    pred = pred > 32767 ? 32767 : pred < -32768 ? -32768 : pred;
    index += (n & 4u) ? (int32_t)((n & 3u) << 1) + 2 : -1;                      // {-1, -1, -1, -1, 2, 4, 6, 8}[n & 7]
    index = index > kSteps - 1 ? kSteps - 1 : index < 0 ? 0 : index;
    out[k] = pred;
  }
}

// ---- layout ----------------------------------------------------------------------------------------------------------------------
struct ImaLayout { int C, align, wpc; int64_t spb; };        // wpc: 4-byte words per chain of a block (the header and the groups)

bool ima_layout(int channels, int block_align, ImaLayout* L) {
  if (channels < 1 || channels > kMaxChannels || block_align < 8 * channels || block_align > 65535 || block_align % (4 * channels)) return false;
  L->C = channels; L->align = block_align; L->wpc = block_align / (4 * channels); L->spb = 1 + 8 * (int64_t)(L->wpc - 1);
  return true;
}

// frames of `nbytes`: spb per whole block, 1 + 8k for a trailing partial block with its headers and k whole groups
int64_t ima_frames(const ImaLayout& L, int64_t nbytes) {
  const int64_t full = nbytes / L.align, rest = nbytes - full * L.align;
  return full * L.spb + (rest >= 4 * L.C ? 1 + 8 * (rest / (4 * L.C) - 1) : 0);
}

int ima_bpw(const ImaLayout& L) {
  // a tile of b blocks takes wpc * ((b * C) | 1) words; one block alone is stored without the padding word
  const int64_t by_lds = (kImaLdsBytes / 4 / L.wpc - 1) / L.C;
  return (int)std::max<int64_t>(1, std::min<int64_t>(kThreads / L.C, by_lds));
}

#define IMA_LAYOUT_TEXT "%s: need 1 <= channels <= 8, 8 * channels <= block_align <= 65535 and block_align a multiple of 4 * channels (channels %d, block_align %d)"

// ---- device --------------------------------------------------------------------------------------------------------------------------
// e: index into the interleaved stream; n = e / C, c = e % C kept by increments
__global__ __launch_bounds__(kThreads) void g711_decode_kernel(const uint8_t* __restrict__ src, long total, int channels, int law, long head,
                                                               long pieces, float* __restrict__ out, long ld) {
  const uint4* body = reinterpret_cast<const uint4*>(src + head);
  for (long p = (long)blockIdx.x * kThreads + threadIdx.x; p < pieces; p += (long)gridDim.x * kThreads) {
    const uint4 q = body[p];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    const long e0 = head + 16 * p;
    long n = e0 / channels;
    int c = (int)(e0 - n * channels);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      out[(long)c * ld + n] = pcm16_scale(g711_one((w[k >> 2] >> (8 * (k & 3))) & 0xFFu, law));
      if (++c == channels) { c = 0; ++n; }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 32) {                       // fewer than 16 bytes at either end
    const long tail0 = head + 16 * pieces;
    const long e = threadIdx.x < 16 ? (long)threadIdx.x : tail0 + (threadIdx.x - 16);
    if (threadIdx.x < 16 ? e < head : e < total) {
      const long n = e / channels;
      out[(e - n * channels) * ld + n] = pcm16_scale(g711_one(src[e], law));
    }
  }
}

// nblocks: the blocks that hold one of the first `frames` frames; used: the bytes of the payload those blocks have (a multiple of 4)
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void ima_decode_kernel(const uint8_t* __restrict__ src, long used, long nblocks, int C, int align, int wpc, int bpw,
                                                              long frames, float* __restrict__ out, long ld) {
  extern __shared__ uint32_t s_words[];
  __shared__ int32_t s_step[kSteps];
  const int tid = threadIdx.x;
  if (tid < kSteps) s_step[tid] = kStepDev[tid];
  const int nch = bpw * C;                                         // chains of a full tile, <= kThreads
  const int S = bpw > 1 ? (nch | 1) : nch;
  const int wpb = align >> 2;                                      // words per block
  const long spb = 1 + 8 * (long)(wpc - 1);
  const long ntiles = (nblocks + bpw - 1) / bpw;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long b0 = t * bpw;
    const long byte0 = b0 * align;
    const int words = (int)((min(used, byte0 + (long)bpw * align) - byte0) >> 2);
    __syncthreads();                                               // the lanes of the last trip are done with s_words (first trip: s_step is there)
    for (int j = tid; j < words; j += kThreads) {
      uint32_t w;
      if (ALIGNED) w = reinterpret_cast<const uint32_t*>(src + byte0)[j];
      else {
        const uint8_t* p = src + byte0 + 4 * (long)j;
        w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
      }
      const int b = j / wpb, q = j - b * wpb;                       // q: headers of channels 0 .. C - 1, then group g = (q - C) / C of channel (q - C) % C
      const int g1 = q / C, c = q - g1 * C;                         // g1 = 0: the header; else group g1 - 1
      s_words[g1 * S + b * C + c] = w;
    }
    __syncthreads();
    if (tid < nch) {
      const int b = tid / C, c = tid - b * C;
      const long B = b0 + b;
      const long n0 = B * spb;
      if (B < nblocks && n0 < frames) {
        // whole groups of this chain that the payload holds (a partial last block) and that start inside `frames`
        const long have = (min(used - B * align, (long)align) >> 2) / C - 1;       // >= 0: the block holds its headers
        int32_t pred, index;
        ima_header(s_words[tid], pred, index);
        float* row = out + (long)c * ld + n0;
        row[0] = pcm16_scale(pred);
        const long left = frames - n0 - 1;                          // samples behind the first that are wanted
        const int groups = (int)min(have, (left + 7) >> 3);
        const bool vec = (reinterpret_cast<uintptr_t>(row + 1) & 15u) == 0;
        for (int g = 0; g < groups; ++g) {
          int32_t v[8];
          ima_group(s_step, s_words[(g + 1) * S + tid], pred, index, v);
          float* p = row + 1 + 8 * (long)g;
          const long room = left - 8 * (long)g;                     // > 0
          if (vec && room >= 8) {
            reinterpret_cast<float4*>(p)[0] = make_float4(pcm16_scale(v[0]), pcm16_scale(v[1]), pcm16_scale(v[2]), pcm16_scale(v[3]));
            reinterpret_cast<float4*>(p)[1] = make_float4(pcm16_scale(v[4]), pcm16_scale(v[5]), pcm16_scale(v[6]), pcm16_scale(v[7]));
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
              if (k < room) p[k] = pcm16_scale(v[k]);
          }
        }
      }
    }
  }
}

int check_ima(const char* what, int64_t nbytes, int channels, int block_align, ImaLayout* L) {
  P2PHD_REQUIRE(ima_layout(channels, block_align, L), IMA_LAYOUT_TEXT, what, channels, block_align);
  P2PHD_REQUIRE(nbytes >= 0 && nbytes <= (int64_t(1) << 40), "%s: need 0 <= nbytes <= 2^40 (nbytes %lld)", what, (long long)nbytes);
  return P2PHD_OK;
}

}  // namespace

// ---- host entries ----------------------------------------------------------------------------------------------------------------
extern "C" int p2phd_g711_decode_host(const void* bytes, int64_t frames, int channels, int law, float* out, int64_t ld) {
  const char* what = "g711_decode_host";
  P2PHD_REQUIRE(frames >= 0 && channels >= 1 && channels <= 65535, "%s: need frames >= 0 and 1 <= channels <= 65535 (frames %lld, channels %d)", what,
                (long long)frames, channels);
  P2PHD_REQUIRE(law == P2PHD_G711_ULAW || law == P2PHD_G711_ALAW, "%s: law must be 0 (mu-law) or 1 (A-law), got %d", what, law);
  P2PHD_REQUIRE(ld >= frames, "%s: ld %lld is shorter than the %lld frames of a row", what, (long long)ld, (long long)frames);
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes && out, "%s: null pointer", what);
  const uint8_t* b = static_cast<const uint8_t*>(bytes);
  for (int64_t n = 0; n < frames; ++n)
    for (int c = 0; c < channels; ++c) out[(int64_t)c * ld + n] = pcm16_scale(g711_one(b[n * channels + c], law));
  return P2PHD_OK;
}

extern "C" int64_t p2phd_ima_frames(int64_t nbytes, int channels, int block_align) {
  ImaLayout L;
  if (check_ima("ima_frames", nbytes, channels, block_align, &L)) return -1;
  return ima_frames(L, nbytes);
}

extern "C" int p2phd_ima_decode_host(const void* bytes, int64_t nbytes, int channels, int block_align, int64_t first_frame, int64_t frame_count,
                                     float* out, int64_t ld) {
  const char* what = "ima_decode_host";
  ImaLayout L;
  if (const int rc = check_ima(what, nbytes, channels, block_align, &L)) return rc;
  const int64_t there = ima_frames(L, nbytes);
  P2PHD_REQUIRE(first_frame >= 0 && frame_count >= 0 && first_frame <= there && frame_count <= there - first_frame,
                "%s: frames [%lld, %lld + %lld) are not inside the %lld the payload holds", what, (long long)first_frame, (long long)first_frame,
                (long long)frame_count, (long long)there);
  P2PHD_REQUIRE(ld >= frame_count, "%s: ld %lld is shorter than the %lld frames of a row", what, (long long)ld, (long long)frame_count);
  if (frame_count == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes && out, "%s: null pointer", what);
  const uint8_t* src = static_cast<const uint8_t*>(bytes);
  const int64_t stop = first_frame + frame_count;
  for (int64_t B = first_frame / L.spb; B * L.spb < stop; ++B) {
    const uint8_t* blk = src + B * L.align;
    const int64_t n0 = B * L.spb;
    for (int c = 0; c < L.C; ++c) {
      uint32_t w;
      memcpy(&w, blk + 4 * c, 4);
      int32_t pred, index;
      ima_header(w, pred, index);
      float* row = out + (int64_t)c * ld;                            // row[n - first_frame]: frame n of the payload
      if (n0 >= first_frame) row[n0 - first_frame] = pcm16_scale(pred);
      // the block's own groups, as far as the window goes (stop <= there: such a group of a partial last block is in the payload)
      for (int64_t g = 0; g < L.wpc - 1 && n0 + 1 + 8 * g < stop; ++g) {
        memcpy(&w, blk + 4 * L.C * (g + 1) + 4 * c, 4);
        int32_t v[8];
        ima_group(kStepHost, w, pred, index, v);
        for (int k = 0; k < 8; ++k) {
          const int64_t n = n0 + 1 + 8 * g + k;
          if (n >= first_frame && n < stop) row[n - first_frame] = pcm16_scale(v[k]);
        }
      }
    }
  }
  return P2PHD_OK;
}

extern "C" int64_t p2phd_ima_scan_host(const void* bytes, int64_t nbytes, int channels, int block_align) {
  ImaLayout L;
  if (check_ima("ima_scan_host", nbytes, channels, block_align, &L)) return -2;
  if (nbytes > 0 && bytes == nullptr) { p2phd::set_error("ima_scan_host: null pointer"); return -2; }
  const uint8_t* src = static_cast<const uint8_t*>(bytes);
  for (int64_t B = 0; B * L.align + 4 * L.C <= nbytes; ++B)
    for (int c = 0; c < L.C; ++c)
      if (src[B * L.align + 4 * c + 2] > kSteps - 1) return B;
  return -1;
}

extern "C" int p2phd_ima_blocks_per_workgroup(int channels, int block_align) {
  ImaLayout L;
  if (check_ima("ima_blocks_per_workgroup", 0, channels, block_align, &L)) return 0;
  return ima_bpw(L);
}

extern "C" int p2phd_ima_max_workgroups(void) { return kImaGrid; }
extern "C" int p2phd_g711_max_workgroups(void) { return (int)kG711Grid; }

// ---- device entries ----------------------------------------------------------------------------------------------------------------
extern "C" int p2phd_g711_decode(const void* bytes, int64_t frames, int channels, int law, float* out, int64_t ld, void* stream) {
  const char* what = "g711_decode";
  P2PHD_REQUIRE(frames >= 0 && channels >= 1 && channels <= 65535, "%s: need frames >= 0 and 1 <= channels <= 65535 (frames %lld, channels %d)", what,
                (long long)frames, channels);
  P2PHD_REQUIRE(law == P2PHD_G711_ULAW || law == P2PHD_G711_ALAW, "%s: law must be 0 (mu-law) or 1 (A-law), got %d", what, law);
  P2PHD_REQUIRE(ld >= frames, "%s: ld %lld is shorter than the %lld frames of a row", what, (long long)ld, (long long)frames);
  P2PHD_REQUIRE(frames <= (int64_t(1) << 40) / channels, "%s: frames * channels too large", what);
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes && out, "%s: null pointer", what);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out is not aligned to a float", what);
  const int64_t total = frames * channels;
  const int64_t head = std::min<int64_t>(total, (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(bytes) & 15u)) & 15u));
  const int64_t pieces = (total - head) / 16;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(p2phd::cdiv(pieces, kThreads), kG711Grid));
  hipLaunchKernelGGL(g711_decode_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, static_cast<const uint8_t*>(bytes), (long)total, channels, law,
                     (long)head, (long)pieces, out, (long)ld);
  ++p2phd::g_launch_count[p2phd::LC_WAVCODEC];
  return p2phd::check_launch(what);
}

extern "C" int p2phd_ima_decode(const void* bytes, int64_t nbytes, int channels, int block_align, int64_t frames, float* out, int64_t ld,
                                void* stream) {
  const char* what = "ima_decode";
  ImaLayout L;
  if (const int rc = check_ima(what, nbytes, channels, block_align, &L)) return rc;
  const int64_t there = ima_frames(L, nbytes);
  P2PHD_REQUIRE(frames >= 0 && frames <= there, "%s: %lld frames asked of a payload that holds %lld", what, (long long)frames, (long long)there);
  P2PHD_REQUIRE(ld >= frames, "%s: ld %lld is shorter than the %lld frames of a row", what, (long long)ld, (long long)frames);
  P2PHD_REQUIRE(block_align <= kImaMaxAlignDev, "%s: a block of %d bytes does not fit a workgroup's LDS beside the step table (at most %d)", what,
                block_align, kImaMaxAlignDev);
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes && out, "%s: null pointer", what);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out is not aligned to a float", what);
  const int64_t nblocks = p2phd::cdiv(frames, L.spb);
  // the bytes of those blocks that are there, in whole groups: the last block may be a partial one
  const int64_t used = std::min<int64_t>(nblocks * L.align, nbytes) / (4 * L.C) * (4 * L.C);
  const int bpw = ima_bpw(L);
  const int S = bpw > 1 ? ((bpw * L.C) | 1) : L.C;
  const size_t lds = (size_t)L.wpc * (size_t)S * sizeof(uint32_t);            // <= 32 KiB, or one block's bytes (< 64 KiB)
  const int grid = (int)std::min<int64_t>(p2phd::cdiv(nblocks, bpw), kImaGrid);
  const bool aligned = (reinterpret_cast<uintptr_t>(bytes) & 3) == 0;
  hipLaunchKernelGGL(aligned ? ima_decode_kernel<true> : ima_decode_kernel<false>, dim3(grid), dim3(kThreads), lds, (hipStream_t)stream,
                     static_cast<const uint8_t*>(bytes), (long)used, (long)nblocks, L.C, L.align, L.wpc, bpw, (long)frames, out, (long)ld);
  ++p2phd::g_launch_count[p2phd::LC_WAVCODEC];
  return p2phd::check_launch(what);
}
