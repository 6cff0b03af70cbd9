// Whole-file generation (pix2pixhdaudiosr_amd/generate/): the noise-shaped dither of the output stage (--dither shaped) -- an
// error-feedback quantiser in front of the 16-bit rounding, PCM16 only.  Launch family "shaper".
//
// The recursion runs along time and is not linear (it rounds), so it is made parallel by its definition: the row is cut in chunks
// of L samples and the error history is zero at the start of every chunk.  For channel c of C and sample n of the chunk at j L
// (e[m] = 0 for m < j L), include/p2phd.h:
//
//   v = (x[c][n] * g) * 32768                                  g = gain[0] read from device memory (no gain: 1); both exact or one rounding
//   u = v;  for k = K, K - 1, .., 1:  u = fmaf(-h[k], e[n - k], u)          one fmaf per tap, the newest error last
//   d = tpdf(seed, first_index + n C + c)                      dither.h, the dither of p2phd_pcm_encode_ex
//   w = u + d;  r = rintf(w);  stored = clamp(r, -32768, 32767), NaN -> 0
//   e[n] = r - u where w is finite, else 0                     from the unclamped r
//
// A lane's bits depend on its chunk's operands alone, whatever the grid.  Zero taps are the bytes of p2phd_pcm_encode_ex with TPDF.
//
// One lane owns one (chunk, channel) and walks it in order.  Lanes of a wave would read L * 4 bytes apart, so a workgroup of 256
// threads walks its rows -- G chunks x CW channels, at most 64, the lanes of its first wave -- in time tiles of 64 samples through
// LDS.  All four waves stage a tile: every row's 256 contiguous bytes are read in 16-byte pieces, one tile ahead of their use, and
// v and d (the hash is a dozen integer operations) are formed there and stored as two [64][65] images, the odd pitch making "lane i
// reads row i, column t" conflict-free.  The first wave then runs the recursion over the tile, 16 steps per pass: the taps are
// kernel arguments (scalar registers), the error history a rotating window of 16 registers with constant indices, and of the K
// fmaf of a step only the last waits for the step before.  It leaves the stored integer in place of v.  All four waves then write
// the tile out as whole interleaved frames: with CW = C the frames of a chunk are one contiguous run of bytes, written in 16-byte
// pieces where the pointer allows and sample by sample at the run's ends (byte by byte to an odd pointer).  More than 64 channels
// are walked 64 at a time (grid y), their frames written as runs of one frame.  K is padded with zero taps to 3, 5, 9 or 16: a zero
// tap changes at most the sign of a zero, never a stored integer.
//
// The launch is bound by the latency of the recursion, not by bandwidth: a 15 s mono clip at L = 4096 is 176 lanes.  G is 1 until
// there are more than 1024 chunks, so that short clips spread over the CUs with next to nothing to stage per workgroup.
#include "common.h"
#include "convplan.h"
#include "dither.h"
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace {
constexpr int kThreads = 256;
constexpr int kRows = 64;                     // rows (chunk, channel) of a workgroup at most: the lanes of the wave that runs the recursion
constexpr int kT = 64;                        // samples of a time tile
constexpr int kPitch = kT + 1;                // odd: lane i, column t is bank (i + t) mod 32
constexpr int kWin = 16;                      // error window = steps per pass = taps at most
constexpr int kLoads = kRows * (kT / 4) / kThreads;      // 16-byte pieces a thread stages per tile
constexpr int kSpread = 1024;                 // workgroups wanted before one takes a second chunk
constexpr int64_t kMinChunk = 256, kMaxChunk = 1 << 20;
static_assert(kT % kWin == 0 && kRows * (kT / 4) % kThreads == 0 && kT / 4 == 16, "tile shape");

struct Taps { float nh[kWin]; };              // nh[k - 1] = -h[k], zero beyond K
struct __attribute__((packed, aligned(4))) F4 { float x, y, z, w; };   // four floats at any float address

// The piece `p` of a tile's staging: its row, where the row's chunk and channel lie, and how many of its four samples exist
struct Piece { int at; long n; int c; int have; };
__device__ __forceinline__ Piece piece_of(int p, int t, long j0, int Gw, int CW, int c0, int cw, long L, long frames) {
  const int r = p >> 4, q = p & 15;
  const int gi = r / CW, cc = r - gi * CW;
  Piece pc;
  pc.at = r * kPitch + 4 * q;
  pc.c = c0 + cc;
  const long col = (long)t * kT + 4 * q;
  const long j = j0 + gi;
  pc.n = j * L + col;
  const long len = gi < Gw && cc < cw ? min(L, frames - j * L) : 0;      // samples of the row's chunk; 0: no such row
  pc.have = (int)max(0l, min(4l, len - col));
  return pc;
}

template <int KT>
__global__ __launch_bounds__(kThreads) void shaper_kernel(const float* __restrict__ planar, long frames, int C, long ld,
                                                          const float* __restrict__ gain, Taps taps, long L, uint64_t seed, uint64_t first,
                                                          uint8_t* __restrict__ out, int aligned, int G, int CW) {
  __shared__ float s_v[kRows * kPitch];       // v; behind the recursion the stored integer
  __shared__ float s_d[kRows * kPitch];
  const int tid = threadIdx.x;
  const long nchunks = (frames + L - 1) / L;
  const long j0 = (long)blockIdx.x * G;
  const int Gw = (int)min((long)G, nchunks - j0);
  const int c0 = blockIdx.y * CW, cw = min(CW, C - c0);
  const long len0 = min(L, frames - j0 * L);                       // the workgroup's first chunk is its longest
  const int ntiles = (int)((len0 + kT - 1) / kT);
  const float g = gain ? *gain : 1.0f;                             // x * 1 is x: one kernel with and without a gain
  const bool whole = gridDim.y == 1;                               // every channel is here: a chunk's frames are one run of bytes

  float e[kWin];
#pragma unroll
  for (int k = 0; k < kWin; ++k) e[k] = 0.0f;

  float4 x[kLoads];
  auto fetch = [&](int t) {
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const Piece pc = piece_of(tid + k * kThreads, t, j0, Gw, CW, c0, cw, L, frames);
      const float* src = planar + (long)pc.c * ld + pc.n;
      x[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (pc.have == 4) { const F4 f = *reinterpret_cast<const F4*>(src); x[k] = make_float4(f.x, f.y, f.z, f.w); }
      else if (pc.have > 0) {
        x[k].x = src[0];
        if (pc.have > 1) x[k].y = src[1];
        if (pc.have > 2) x[k].z = src[2];
      }
    }
  };
  fetch(0);
  for (int t = 0; t < ntiles; ++t) {
    // stage: v and d of the tile, zeros where there is no sample
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const Piece pc = piece_of(tid + k * kThreads, t, j0, Gw, CW, c0, cw, L, frames);
      const float xs[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const bool on = m < pc.have;
        const uint64_t i = first + (uint64_t)(pc.n + m) * (uint64_t)C + (uint64_t)pc.c;
        s_v[pc.at + m] = on ? (xs[m] * g) * 32768.0f : 0.0f;
        s_d[pc.at + m] = on ? p2phd::tpdf(seed, i) : 0.0f;
      }
    }
    __syncthreads();
    if (t + 1 < ntiles) fetch(t + 1);                              // in flight while the recursion runs
    if (tid < kRows) {
      float* rv = s_v + tid * kPitch;
      const float* rd = s_d + tid * kPitch;
#pragma unroll 1
      for (int b = 0; b < kT; b += kWin) {
        float v[kWin], d[kWin];
#pragma unroll
        for (int s = 0; s < kWin; ++s) { v[s] = rv[b + s]; d[s] = rd[b + s]; }
#pragma unroll
        for (int s = 0; s < kWin; ++s) {
          float u = v[s];
#pragma unroll
          for (int k = KT; k >= 1; --k) u = __builtin_fmaf(taps.nh[k - 1], e[(s - k) & (kWin - 1)], u);
          const float w = u + d[s];
          const float r = rintf(w);
          e[s] = fabsf(w) < INFINITY ? r - u : 0.0f;                // (a NaN compares false)
          const int code = w != w ? 0 : (int)fminf(fmaxf(r, -32768.0f), 32767.0f);
          rv[b + s] = __int_as_float(code);
        }
      }
    }
    __syncthreads();
    // write out: runs of interleaved samples -- a chunk's frames of this tile (every channel here), or one frame's channels
    {
      const long col0 = (long)t * kT;
      const int tn0 = (int)min((long)kT, len0 - col0);             // frames of the first chunk in this tile (>= 1)
      const int nruns = whole ? Gw : tn0;
      const int PP = ((whole ? kT * C : cw) + 7) / 8 + 1;           // 16-byte pieces a run touches at most
      for (int f = tid; f < nruns * PP; f += kThreads) {
        const int run = f / PP, pi = f - run * PP;
        long e0;                                                    // interleaved index of the run's first sample
        int len;                                                    // samples of the run
        if (whole) {
          const long j = j0 + run;
          len = (int)max(0l, min((long)kT, min(L, frames - j * L) - col0)) * C;
          e0 = (j * L + col0) * C;
        } else {
          len = cw;
          e0 = (j0 * L + col0 + run) * C + c0;
        }
        uint8_t* base = out + e0 * 2;
        const int lead = aligned ? (int)((reinterpret_cast<uintptr_t>(base) & 15u) >> 1) : 0;   // samples from the 16-byte boundary in front
        const int lo = pi * 8 - lead;
        if (lo >= len) continue;
        const int first_el = max(lo, 0);
        int n, cc, row0;
        if (whole) { n = first_el / C; cc = first_el - n * C; row0 = run * CW; }
        else { n = run; cc = first_el; row0 = 0; }
        uint32_t val[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const int el = lo + m;
          const bool on = el >= 0 && el < len;
          val[m] = on ? __float_as_uint(s_v[(row0 + cc) * kPitch + n]) & 0xFFFFu : 0u;
          if (on && ++cc == C) { cc = 0; ++n; }                     // (a run of one frame ends before cc reaches C)
        }
        if (aligned && lo >= 0 && lo + 8 <= len) {
          *reinterpret_cast<uint4*>(base + (long)lo * 2) = make_uint4(val[0] | val[1] << 16, val[2] | val[3] << 16, val[4] | val[5] << 16, val[6] | val[7] << 16);
        } else {
#pragma unroll
          for (int m = 0; m < 8; ++m) {
            const int el = lo + m;
            if (el < 0 || el >= len) continue;
            uint8_t* p = base + (long)el * 2;
            if (aligned) *reinterpret_cast<uint16_t*>(p) = (uint16_t)val[m];
            else { p[0] = (uint8_t)val[m]; p[1] = (uint8_t)(val[m] >> 8); }
          }
        }
      }
    }
    __syncthreads();                                                // the next tile's staging overwrites the images
  }
}

bool chunk_ok(int64_t chunk) { return chunk >= kMinChunk && chunk <= kMaxChunk && chunk % 64 == 0; }

// the published curves, h[1..K] in float64
struct Curve { int K; double h[kWin]; };
const Curve kCurves[] = {
    {9, {2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847}},     // 0 lipshitz9
    {5, {2.033, -2.165, 1.959, -1.590, 0.6149}},                                    // 1 e5
    {3, {1.623, -0.982, 0.109}},                                                    // 2 light3
};

}  // namespace

extern "C" int p2phd_shaper_taps_fill(int curve_id, float* out, int* K) {
  P2PHD_REQUIRE(curve_id >= 0 && curve_id < (int)(sizeof(kCurves) / sizeof(kCurves[0])), "shaper_taps_fill: unknown curve %d (0 lipshitz9, 1 e5, 2 light3)", curve_id);
  P2PHD_REQUIRE(out && K, "shaper_taps_fill: null output");
  const Curve& c = kCurves[curve_id];
  for (int k = 0; k < c.K; ++k) out[k] = (float)c.h[k];
  *K = c.K;
  return P2PHD_OK;
}

extern "C" int64_t p2phd_shaper_tile_len(int channels, int64_t chunk) {
  if (channels < 1 || channels > 65535 || !chunk_ok(chunk)) {
    p2phd::set_error("shaper_tile_len: need 1 <= channels <= 65535 and a chunk that is a multiple of 64 in [%lld, %lld] (channels %d, chunk %lld)",
                     (long long)kMinChunk, (long long)kMaxChunk, channels, (long long)chunk);
    return -1;
  }
  return kT;
}

extern "C" int p2phd_pcm_encode_shaped(const float* planar, int64_t frames, int channels, int64_t ld, const float* gain, const float* taps, int K,
                                       int64_t chunk, uint64_t seed, int64_t first_index, void* out, void* stream) {
  const char* what = "pcm_encode_shaped";
  if (const int rc = p2phd::pcm_check_rows(what, frames, channels, ld, P2PHD_PCM_S16, true)) return rc;
  P2PHD_REQUIRE(K >= 0 && K <= kWin, "%s: K must be in [0, %d], got %d", what, kWin, K);
  P2PHD_REQUIRE(K == 0 || taps != nullptr, "%s: null taps with K = %d", what, K);
  P2PHD_REQUIRE(chunk_ok(chunk), "%s: chunk must be a multiple of 64 in [%lld, %lld], got %lld", what, (long long)kMinChunk, (long long)kMaxChunk,
                (long long)chunk);
  P2PHD_REQUIRE(first_index >= 0 && first_index % (chunk * channels) == 0,
                "%s: first_index %lld is not a multiple of chunk * channels = %lld (a piece starts where a chunk starts)", what, (long long)first_index,
                (long long)(chunk * channels));
  Taps t;
  for (int k = 0; k < kWin; ++k) {
    const float h = k < K ? taps[k] : 0.0f;
    P2PHD_REQUIRE(std::isfinite(h), "%s: tap %d is not finite", what, k + 1);
    t.nh[k] = -h;
  }
  if (frames == 0) return P2PHD_OK;
  P2PHD_REQUIRE(planar && out, "%s: null pointer", what);
  P2PHD_REQUIRE(((reinterpret_cast<uintptr_t>(planar) | reinterpret_cast<uintptr_t>(gain)) & 3) == 0, "%s: planar or gain is not aligned to a float", what);
  const int64_t nchunks = p2phd::cdiv(frames, chunk);
  const int CW = std::min(channels, kRows);
  const int G = (int)std::max<int64_t>(1, std::min<int64_t>(channels <= kRows ? kRows / channels : 1, p2phd::cdiv(nchunks, kSpread)));
  const int64_t gx = p2phd::cdiv(nchunks, G);
  P2PHD_REQUIRE(gx <= 0x7FFFFFFF, "%s: %lld workgroups are too many", what, (long long)gx);
  const dim3 grid((unsigned)gx, (unsigned)p2phd::cdiv(channels, CW));
  const int aligned = (reinterpret_cast<uintptr_t>(out) & 1) == 0;
  const int KT = K <= 3 ? 3 : K <= 5 ? 5 : K <= 9 ? 9 : kWin;
  const auto kernel = KT == 3 ? shaper_kernel<3> : KT == 5 ? shaper_kernel<5> : KT == 9 ? shaper_kernel<9> : shaper_kernel<kWin>;
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, planar, (long)frames, channels, (long)ld, gain, t, (long)chunk, seed,
                     (uint64_t)first_index, static_cast<uint8_t*>(out), aligned, G, CW);
  ++p2phd::g_launch_count[p2phd::LC_SHAPER];
  return p2phd::check_launch(what);
}
