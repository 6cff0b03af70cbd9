// FLAC output (the stream contract of include/p2phd.h, "FLAC output"): the writer behind whole-file generation.  Launch family
// "flacenc".
//
//   host    p2phd_flac_encode_plan     frames, worst-case stream bytes (every subframe VERBATIM), workspace bytes
//           p2phd_flac_encode_host     the reference encoder: one thread, frame after frame
//   device  p2phd_flac_encode          flacenc_frames_kernel: one WORKGROUP owns one frame.  Per coded channel (left, right, mid and side
//                                      of a stereo pair; the channel itself otherwise) and per predictor order the lanes form the zig-zag
//                                      residuals of their samples and sum u >> k for every Rice parameter k per finest partition (registers,
//                                      then LDS integer adds); the coarser partitions are sums of pairs, so one pass serves every partition
//                                      order.  The cheapest subframe is then written: a prefix scan over the code lengths gives every code
//                                      its bit position and the lanes OR their stop bit and their k low bits into a zeroed LDS window of
//                                      the frame's bit stream (a unary run is the zeros that are already there); a full window is stored
//                                      to the frame's worst-case slot of the workspace and moves on.  The CRC-16 is taken in parallel:
//                                      a CRC per lane's piece, multiplied by x^(8 n) mod the polynomial for the n bytes behind it, XORed.
//                                      flacenc_scan_kernel: one workgroup turns the frame lengths into offsets and writes `lengths`.
//                                      flacenc_gather_kernel: a workgroup per frame copies its slot to its place in the stream.
//
// The LPC option ("FLAC output, LPC" of include/p2phd.h; p2phd_flac_lpc_fit / p2phd_flac_lpc_analyse / p2phd_flac_encode_lpc_host on the host,
// p2phd_flac_encode_lpc on the device) is a third template parameter of the frame kernel: that instantiation also keeps the coded
// channel's block as int32 and its analysis signal in dynamic LDS, lane 0 fits the predictors (lpc_fit, the only float in this file),
// and every admitted order goes through the same Rice sums and partition fold; the other instantiations are as they were.
//
// Both encoders decide with the SAME routines (__host__ __device__): sample access, residual, zig-zag, the best k of a partition, the
// stereo assignment, the frame header.  Every decision is an exact integer bit count; every sum is an integer sum, whose value does not
// depend on the order of its terms: the same bytes on every run, stream and grid.
#include "common.h"
#include "convplan.h"
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#define FHD __host__ __device__ __forceinline__

namespace {
constexpr int kThreads = 256;                  // lanes of flacenc_frames_kernel and of flacenc_gather_kernel
constexpr int kScan = 1024;                    // lanes of flacenc_scan_kernel: frames per step of its one workgroup
constexpr int kParts = 256;                    // finest partitions of a block at most (partition order 8)
constexpr int kMaxPorder = 8;
constexpr int kWin = 1024;                     // 32-bit words of the LDS window of the frame's bit stream
constexpr int kMid = 8, kSide = 9;             // coded channels of a stereo pair beside 0 (left) and 1 (right)
constexpr int kHeaderMax = 16;                 // bytes of a frame header at most (4 + 6 + 2 + 2 + 1 = 15)
constexpr int kLpcMax = 12;                    // LPC orders of the option lpc_order (the streamable subset's most up to 48 kHz)
constexpr int kLpcPrec = 13;                   // bits of a quantised LPC coefficient
constexpr int kLpcBlock = 16384;               // the largest block with lpc_order > 0 (the subset's; its int32 image is 64 KiB)
constexpr uint32_t kLpcResLimit = 1u << 28;    // an LPC order is admitted only where every |residual| is below it
enum { T_CONSTANT = 0, T_VERBATIM = 1, T_FIXED = 2, T_LPC = 3 };

// ---- the arithmetic both encoders share ---------------------------------------------------------------------------------------
struct Geo { const uint8_t* pcm; int C, bytes; int64_t first; int bs; };   // a frame: samples [first, first + bs) of the payload

FHD int32_t pcm_at(const uint8_t* p, int bytes, int64_t idx) {              // sample idx of the interleaved little-endian payload
  const uint8_t* q = p + idx * bytes;
  if (bytes == 2) return (int32_t)(int16_t)(uint16_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8));
  return (int32_t)(((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16)) << 8) >> 8;
}

FHD int32_t coded_at(const Geo& g, int ch, int n) {                         // sample n of coded channel ch
  if (ch < kMid) return pcm_at(g.pcm, g.bytes, (g.first + n) * g.C + ch);
  const int32_t l = pcm_at(g.pcm, g.bytes, (g.first + n) * 2), r = pcm_at(g.pcm, g.bytes, (g.first + n) * 2 + 1);
  return ch == kMid ? (l + r) >> 1 : l - r;
}

FHD int32_t residual(const Geo& g, int ch, int o, int n) {                  // of the fixed predictor of order o at n >= o (below 2^29 in size)
  const int32_t a = coded_at(g, ch, n);
  if (o == 0) return a;
  const int32_t b = coded_at(g, ch, n - 1);
  if (o == 1) return a - b;
  const int32_t c = coded_at(g, ch, n - 2);
  if (o == 2) return a - 2 * b + c;
  const int32_t d = coded_at(g, ch, n - 3);
  if (o == 3) return a - 3 * b + 3 * c - d;
  return a - 4 * b + 6 * c - 4 * d + coded_at(g, ch, n - 4);
}

FHD uint32_t zigzag(int32_t r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// The cheapest Rice parameter of a partition of n residuals: sum(k) = the sum of u >> k.  Ties: the smaller k.
template <class S> FHD void best_k(uint64_t n, int K, S sum, int& kbest, uint64_t& bits) {
  kbest = 0; bits = n + sum(0);
  for (int k = 1; k < K; ++k) {
    const uint64_t b = n * (uint64_t)(k + 1) + sum(k);
    if (b < bits) { bits = b; kbest = k; }
  }
}

FHD int max_porder(int bs) { const int z = bs ? __builtin_ctz((unsigned)bs) : 0; return z < kMaxPorder ? z : kMaxPorder; }

// cost[o * 9 + p] of every admitted pair -> the subframe: FIXED only where strictly below VERBATIM; ties: the smaller partition
// order, then the smaller order
FHD void pick_fixed(const unsigned long long* cost, int bs, int bps, int& type, int& o_, int& p_, uint64_t& bits) {
  type = T_VERBATIM; o_ = 0; p_ = 0; bits = 8 + (uint64_t)bs * (uint64_t)bps;
  const int pmax = max_porder(bs);
  for (int p = 0; p <= pmax; ++p)
    for (int o = 0; o <= 4 && o < bs; ++o)
      if ((bs >> p) > o && cost[o * 9 + p] < bits) { type = T_FIXED; o_ = o; p_ = p; bits = cost[o * 9 + p]; }
}

// best bits of left, right, mid, side -> the assignment code (1 independent, 8 left/side, 9 side/right, 10 mid/side); ties in that order
FHD int pick_assign(uint64_t l, uint64_t r, uint64_t m, uint64_t s) {
  int a = 1; uint64_t best = l + r;
  if (l + s < best) { best = l + s; a = 8; }
  if (s + r < best) { best = s + r; a = 9; }
  if (m + s < best) { best = m + s; a = 10; }
  return a;
}

// ---- LPC ("FLAC output, LPC"): the analysis value, the fit, the residual -----------------------------------------------------------
// v[n] of the contract's step 1: the sample cut to 16 bits, times the integer Welch window
FHD int32_t lpc_value(int32_t x, int bps, int n, int bs) {
  const int64_t a = x >> (bps > 16 ? bps - 16 : 0);
  const int64_t d = 2 * (int64_t)n - (bs - 1), D = (int64_t)bs + 1;
  const int64_t W = ((D * D - d * d) << 15) / (D * D);
  return (int32_t)((a * W) >> 15);
}

// Steps 2 and 3: R[0 .. Mo] -> per order o = 1 .. Mo (row o - 1): ok, shift, q[(o - 1) * kLpcMax + j].  Float64 add, multiply and divide
// in the written order, never contracted: one thread or one lane runs it, so host and device give the same bits.  lp, nw: kLpcMax
// doubles of working room each (LDS on the device: no indexed private array).
FHD void lpc_fit(const long long* R, int Mo, double* lp, double* nw, int* q, int* shift, int* ok) {
#pragma clang fp contract(off)
  for (int o = 0; o < kLpcMax; ++o) ok[o] = 0;
  if (R[0] == 0) return;
  double err = (double)R[0];
  for (int i = 0; i < Mo; ++i) {
    double acc = (double)R[i + 1];
    for (int j = 0; j < i; ++j) acc = acc - lp[j] * (double)R[i - j];
    const double k = acc / err;
    for (int j = 0; j < i; ++j) nw[j] = lp[j] - k * lp[i - 1 - j];
    nw[i] = k;
    err = err * (1.0 - k * k);
    if (!(err > 0.0) || !(err <= 1.7976931348623157e308)) return;          // this order and every higher one: not admitted
    double cmax = 0.0;
    for (int j = 0; j <= i; ++j) { lp[j] = nw[j]; const double a = lp[j] < 0.0 ? -lp[j] : lp[j]; if (a > cmax) cmax = a; }
    if (cmax == 0.0) continue;
    const int e = (int)((__builtin_bit_cast(unsigned long long, cmax) >> 52) & 0x7FFull) - 1022;   // frexp's exponent (a subnormal: lower still, the shift clamps)
    int s = kLpcPrec - 1 - e;
    if (s < 0) continue;
    if (s > 15) s = 15;
    const double scale = (double)(1 << s);
    double ee = 0.0;
    for (int j = 0; j <= i; ++j) {
      ee = ee + lp[j] * scale;
      double r = ee >= 0.0 ? __builtin_floor(ee + 0.5) : -__builtin_floor(-ee + 0.5);
      if (r < -4096.0) r = -4096.0;
      if (r > 4095.0) r = 4095.0;
      q[i * kLpcMax + j] = (int)r;
      ee = ee - r;
    }
    shift[i] = s; ok[i] = 1;
  }
}

// Step 4: the residual at n >= o from the block's int32 image; 64-bit, the caller holds it to kLpcResLimit
FHD int64_t lpc_residual(const int32_t* x, const int* q, int o, int shift, int n) {
  int64_t sum = 0;
  for (int j = 0; j < o; ++j) sum += (int64_t)q[j] * (int64_t)x[n - 1 - j];
  return (int64_t)x[n] - (sum >> shift);
}
FHD uint32_t lpc_size(int64_t r) { const uint64_t a = (uint64_t)(r < 0 ? -r : r); return a < kLpcResLimit ? (uint32_t)a : kLpcResLimit; }

// The bits of an LPC subframe of order o in front of its partitions
FHD uint64_t lpc_base_bits(int o, int bps) { return 8 + (uint64_t)o * (uint64_t)bps + 4 + 5 + (uint64_t)o * kLpcPrec + 6; }

FHD uint8_t crc8_step(uint8_t c, uint8_t b) {
  c ^= b;
  for (int i = 0; i < 8; ++i) c = (uint8_t)((c & 0x80) ? (c << 1) ^ 0x07 : c << 1);
  return c;
}

FHD uint32_t crc16_entry(int i) {                                           // the table entry of byte i (poly 0x8005)
  uint32_t c = (uint32_t)i << 8;
  for (int k = 0; k < 8; ++k) c = ((c & 0x8000u) ? (c << 1) ^ 0x8005u : c << 1) & 0xFFFFu;
  return c;
}

// The frame header as _flac_ref.frame_header writes it by default -> its length.  h: 16 bytes.
FHD int build_header(uint8_t* h, int bs, int rate, int assign, int bits, uint32_t number) {
  int bscode = bs <= 256 ? 6 : 7;
  if (bs == 192) bscode = 1;
  for (int i = 0; i < 4; ++i) if (bs == (576 << i)) bscode = 2 + i;
  for (int i = 0; i < 8; ++i) if (bs == (256 << i)) bscode = 8 + i;
  int rcode = rate < 65536 ? 13 : (rate % 10 == 0 && rate / 10 < 65536) ? 14 : 0;
  const int rates[11] = {88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  for (int i = 0; i < 11; ++i) if (rate == rates[i]) rcode = 1 + i;
  int at = 0;
  h[at++] = 0xFF; h[at++] = 0xF8;
  h[at++] = (uint8_t)((bscode << 4) | rcode);
  h[at++] = (uint8_t)((assign << 4) | ((bits == 16 ? 4 : 6) << 1));
  if (number < 0x80u) h[at++] = (uint8_t)number;
  else {
    int n = 2;                                                              // bytes: 11, 16, 21, 26, 31 bits
    while (n < 6 && number >= (1u << (5 * n + 1))) ++n;
    h[at++] = (uint8_t)(((0xFF << (8 - n)) & 0xFF) | (number >> (6 * (n - 1))));
    for (int i = n - 2; i >= 0; --i) h[at++] = (uint8_t)(0x80 | ((number >> (6 * i)) & 0x3F));
  }
  if (bscode == 6) h[at++] = (uint8_t)(bs - 1);
  if (bscode == 7) { h[at++] = (uint8_t)((bs - 1) >> 8); h[at++] = (uint8_t)(bs - 1); }
  if (rcode == 13) { h[at++] = (uint8_t)(rate >> 8); h[at++] = (uint8_t)rate; }
  if (rcode == 14) { h[at++] = (uint8_t)((rate / 10) >> 8); h[at++] = (uint8_t)(rate / 10); }
  uint8_t c = 0;
  for (int i = 0; i < at; ++i) c = crc8_step(c, h[i]);
  h[at++] = c;
  return at;
}

// a * b and x^(8 n) in GF(2)[x] mod x^16 + x^15 + x^2 + 1: CRC(A | B) = CRC(A) * x^(8 |B|) + CRC(B) for a CRC that starts at 0
FHD uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r = ((r & 0x8000u) ? (r << 1) ^ 0x8005u : r << 1) & 0xFFFFu;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
FHD uint32_t gf_xpow8(uint64_t n) {
  uint32_t r = 1, b = 0x100;
  for (; n; n >>= 1) { if (n & 1) r = gf_mul(r, b); b = gf_mul(b, b); }
  return r;
}

// ---- geometry --------------------------------------------------------------------------------------------------------------------
int64_t worst_frame_bytes(int C, int bits, int bs) {                        // every subframe VERBATIM, the side channel's extra bit included
  const int64_t body = (int64_t)C * (8 + (int64_t)bs * bits) + (C == 2 ? bs : 0);
  return kHeaderMax + (body + 7) / 8 + 2;
}
int64_t slot_bytes_of(int C, int bits, int block) { return (worst_frame_bytes(C, bits, block) + 7) / 8 * 8 + 8; }

int check_args(const char* what, int channels, int bits, int64_t L, int rate, int block) {
  P2PHD_REQUIRE(channels >= 1 && channels <= 8, "%s: need 1 <= channels <= 8 (channels %d)", what, channels);
  P2PHD_REQUIRE(bits == 16 || bits == 24, "%s: %d bits per sample (built: the payloads of pcm16 and pcm24)", what, bits);
  P2PHD_REQUIRE(L >= 1 && L < (int64_t(1) << 36), "%s: need 1 <= L < 2^36 samples per channel (L %lld)", what, (long long)L);
  P2PHD_REQUIRE(rate >= 1 && rate <= 1048575, "%s: need 1 <= rate <= 1048575 (rate %d)", what, rate);
  P2PHD_REQUIRE(block >= 16 && block <= 65535, "%s: need 16 <= block <= 65535 (block %d)", what, block);
  P2PHD_REQUIRE((L + block - 1) / block <= 0x7FFFFFFF, "%s: more than 2^31 - 1 frames (L %lld, block %d)", what, (long long)L, block);
  return P2PHD_OK;
}

int check_lpc(const char* what, int lpc_order, int block) {
  P2PHD_REQUIRE(lpc_order >= 0 && lpc_order <= kLpcMax, "%s: need 0 <= lpc_order <= %d (lpc_order %d)", what, kLpcMax, lpc_order);
  P2PHD_REQUIRE(lpc_order == 0 || block <= kLpcBlock, "%s: with lpc_order > 0 the block is at most %d (block %d)", what, kLpcBlock, block);
  return P2PHD_OK;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct Choice { int type, o, p; uint64_t bits; uint8_t k[kParts]; int q[kLpcMax], shift; };

struct Writer {                                                             // MSB first
  uint8_t* out; int64_t at; uint64_t acc; int n;
  void u(uint32_t v, int bits) {                                            // bits <= 32
    acc = (acc << bits) | v; n += bits;
    while (n >= 8) { out[at++] = (uint8_t)(acc >> (n - 8)); n -= 8; }
  }
  void zeros(uint64_t q) { while (q >= 32) { u(0, 32); q -= 32; } u(0, (int)q); }
  void align() { if (n) u(0, 8 - n); }
};

void choose_host(const Geo& g, int ch, int bps, int K, int pbits, Choice& c, std::vector<uint64_t>& sums) {
  const int bs = g.bs;
  const int32_t first = coded_at(g, ch, 0);
  bool same = true;
  for (int n = 1; n < bs && same; ++n) same = coded_at(g, ch, n) == first;
  if (same) { c.type = T_CONSTANT; c.o = c.p = 0; c.bits = 8 + bps; return; }
  const int pmax = max_porder(bs), P = 1 << pmax, s = bs >> pmax;
  unsigned long long cost[5 * 9];
  std::vector<uint8_t> ks((size_t)5 * 512);
  for (int o = 0; o <= 4 && o < bs; ++o) {
    std::fill(sums.begin(), sums.begin() + (size_t)P * K, 0);
    for (int n = o; n < bs; ++n) {
      const uint32_t u = zigzag(residual(g, ch, o, n));
      uint64_t* row = &sums[(size_t)(n / s) * K];
      for (int k = 0; k < K; ++k) row[k] += u >> k;
    }
    for (int p = pmax; p >= 0; --p) {
      const int np = 1 << p;
      if ((bs >> p) > o) {
        uint64_t total = 8 + (uint64_t)o * bps + 6;
        for (int j = 0; j < np; ++j) {
          const uint64_t* row = &sums[(size_t)j * K];
          int kb; uint64_t b;
          best_k((uint64_t)((bs >> p) - (j == 0 ? o : 0)), K, [row](int k) { return row[k]; }, kb, b);
          ks[(size_t)o * 512 + np - 1 + j] = (uint8_t)kb;
          total += pbits + b;
        }
        cost[o * 9 + p] = total;
      }
      for (int j = 0; j < np / 2; ++j)
        for (int k = 0; k < K; ++k) sums[(size_t)j * K + k] = sums[(size_t)(2 * j) * K + k] + sums[(size_t)(2 * j + 1) * K + k];
    }
  }
  pick_fixed(cost, bs, bps, c.type, c.o, c.p, c.bits);
  if (c.type == T_FIXED) memcpy(c.k, &ks[(size_t)c.o * 512 + (1 << c.p) - 1], (size_t)1 << c.p);
}

// steps 1 to 3 of one block
void lpc_analyse_host(const int32_t* x, int bs, int bps, int M, long long* R, int* q, int* shift, int* ok) {
  const int Mo = std::min(M, bs - 1);
  std::vector<int32_t> v((size_t)bs);
  for (int n = 0; n < bs; ++n) v[n] = lpc_value(x[n], bps, n, bs);
  for (int l = 0; l <= kLpcMax; ++l) R[l] = 0;
  for (int l = 0; l <= Mo; ++l)
    for (int n = l; n < bs; ++n) R[l] += (long long)v[n] * (long long)v[n - l];
  double lp[kLpcMax], nw[kLpcMax];
  lpc_fit(R, Mo, lp, nw, q, shift, ok);
}

// Behind choose_host: every LPC order 1 .. min(M, bs - 1) is tried; a pair replaces the choice only with strictly fewer bits, and among
// LPC pairs of equal bits the smaller partition order, then the smaller order, stays
void choose_lpc_host(const Geo& g, int ch, int bps, int K, int pbits, int M, Choice& c, std::vector<uint64_t>& sums) {
  if (M <= 0 || c.type == T_CONSTANT) return;
  const int bs = g.bs;
  std::vector<int32_t> x((size_t)bs);
  for (int n = 0; n < bs; ++n) x[n] = coded_at(g, ch, n);
  long long R[kLpcMax + 1];
  int q[kLpcMax * kLpcMax] = {}, shift[kLpcMax] = {}, ok[kLpcMax];
  lpc_analyse_host(x.data(), bs, bps, M, R, q, shift, ok);
  const int Mo = std::min(M, bs - 1), pmax = max_porder(bs), P = 1 << pmax, s = bs >> pmax;
  std::vector<uint8_t> ks(512);
  for (int o = 1; o <= Mo; ++o) {
    if (!ok[o - 1]) continue;
    const int* qo = &q[(o - 1) * kLpcMax];
    uint32_t rmax = 0;
    for (int n = o; n < bs; ++n) rmax = std::max(rmax, lpc_size(lpc_residual(x.data(), qo, o, shift[o - 1], n)));
    if (rmax >= kLpcResLimit) continue;
    std::fill(sums.begin(), sums.begin() + (size_t)P * K, 0);
    for (int n = o; n < bs; ++n) {
      const uint32_t u = zigzag((int32_t)lpc_residual(x.data(), qo, o, shift[o - 1], n));
      uint64_t* row = &sums[(size_t)(n / s) * K];
      for (int k = 0; k < K; ++k) row[k] += u >> k;
    }
    for (int p = pmax; p >= 0; --p) {
      const int np = 1 << p;
      if ((bs >> p) > o) {
        uint64_t total = lpc_base_bits(o, bps);
        for (int j = 0; j < np; ++j) {
          const uint64_t* row = &sums[(size_t)j * K];
          int kb; uint64_t b;
          best_k((uint64_t)((bs >> p) - (j == 0 ? o : 0)), K, [row](int k) { return row[k]; }, kb, b);
          ks[(size_t)np - 1 + j] = (uint8_t)kb;
          total += pbits + b;
        }
        if (total < c.bits || (c.type == T_LPC && total == c.bits && p < c.p)) {
          c.type = T_LPC; c.o = o; c.p = p; c.bits = total; c.shift = shift[o - 1];
          memcpy(c.q, qo, sizeof(c.q));
          memcpy(c.k, &ks[(size_t)np - 1], (size_t)np);
        }
      }
      for (int j = 0; j < np / 2; ++j)
        for (int k = 0; k < K; ++k) sums[(size_t)j * K + k] = sums[(size_t)(2 * j) * K + k] + sums[(size_t)(2 * j + 1) * K + k];
    }
  }
}

void write_subframe_host(Writer& w, const Geo& g, int ch, int bps, int pbits, const Choice& c) {
  const uint32_t mask = bps == 32 ? ~0u : (1u << bps) - 1u;
  w.u((uint32_t)(c.type == T_CONSTANT ? 0 : c.type == T_VERBATIM ? 1 : c.type == T_LPC ? (32 | (c.o - 1)) : (8 | c.o)) << 1, 8);
  if (c.type == T_CONSTANT) { w.u((uint32_t)coded_at(g, ch, 0) & mask, bps); return; }
  if (c.type == T_VERBATIM) { for (int n = 0; n < g.bs; ++n) w.u((uint32_t)coded_at(g, ch, n) & mask, bps); return; }
  for (int n = 0; n < c.o; ++n) w.u((uint32_t)coded_at(g, ch, n) & mask, bps);
  std::vector<int32_t> x;
  if (c.type == T_LPC) {                                                    // precision - 1, the shift, the coefficients
    w.u((uint32_t)(kLpcPrec - 1), 4);
    w.u((uint32_t)c.shift, 5);
    for (int j = 0; j < c.o; ++j) w.u((uint32_t)c.q[j] & ((1u << kLpcPrec) - 1u), kLpcPrec);
    x.resize((size_t)g.bs);
    for (int n = 0; n < g.bs; ++n) x[n] = coded_at(g, ch, n);
  }
  w.u((uint32_t)((pbits == 5 ? 1 : 0) << 4 | c.p), 6);
  const int psize = g.bs >> c.p;
  for (int n = c.o; n < g.bs; ++n) {
    const int j = n / psize, k = c.k[j];
    if (n == c.o || n == j * psize) w.u((uint32_t)k, pbits);
    const uint32_t u = zigzag(c.type == T_LPC ? (int32_t)lpc_residual(x.data(), c.q, c.o, c.shift, n) : residual(g, ch, c.o, n));
    w.zeros(u >> k);
    w.u((1u << k) | (u & ((1u << k) - 1u)), k + 1);
  }
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
template <int BYTES> struct Smem {
  static constexpr int KLO = BYTES == 2 ? 15 : 16;                          // parameters whose sums need 64 bits: k < 16
  static constexpr int KHI = BYTES == 2 ? 0 : 15;                           // k = 16 .. 30: u >> k < 2^13, a block's sum < 2^29
  unsigned long long lo[KLO * kParts];                                      // [k][partition]: lanes of neighbouring partitions on neighbouring banks
  unsigned long long cost[5 * 9];
  unsigned long long bits[4];
  uint32_t hi[(KHI ? KHI : 1) * kParts];
  uint32_t win[kWin];
  uint32_t wave[4];
  uint32_t crc;
  int neq, hlen, type[4], o[4], p[4];
  uint16_t t16[256];
  uint8_t kall[5 * 512], ck[4 * kParts], hdr[kHeaderMax];
};

// The frame's bit stream goes through a window of kWin words: win[i] is word wbase + i of the frame, bit `at` of the frame is bit
// 31 - at % 32 of word at / 32.  wbase and pos are the same in every lane.
struct Emit { uint32_t* win; uint32_t* slot; uint32_t wbase, pos; };

// value (below 2^nbits, nbits <= 32) at bit `at`: the part of it inside the window, zeros cost nothing
__device__ __forceinline__ void put(const Emit& e, uint32_t at, uint32_t value, int nbits) {
  if (nbits <= 0) return;
  const uint32_t w = (at >> 5) - e.wbase;                                   // (wraps where the word lies in front of the window)
  const uint64_t v = (uint64_t)value << (64 - (int)(at & 31u) - nbits);
  const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
  if (hi && w < (uint32_t)kWin) atomicOr(&e.win[w], hi);
  if (lo && w + 1u < (uint32_t)kWin) atomicOr(&e.win[w + 1u], lo);
}

// Behind the puts of a step that ends at bit `end`: false where it ends inside the window.  Else the window, which is complete, is
// stored and moves on, and the caller repeats the step's puts for the next window.
__device__ __forceinline__ bool emit_more(Emit& e, uint32_t end) {
  if (end <= (e.wbase + (uint32_t)kWin) * 32u) return false;
  __syncthreads();
  for (int i = threadIdx.x; i < kWin; i += kThreads) { e.slot[e.wbase + i] = __builtin_bswap32(e.win[i]); e.win[i] = 0u; }
  e.wbase += (uint32_t)kWin;
  __syncthreads();
  return true;
}

// exclusive prefix sum over the workgroup's 256 lanes; total: the sum of all
__device__ __forceinline__ uint32_t exscan256(uint32_t v, uint32_t* s_wave, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(x, d, 64); if (lane >= d) x += t; }
  if (lane == 63) s_wave[wave] = x;
  __syncthreads();
  uint32_t base = 0; total = 0;
  for (int w = 0; w < 4; ++w) { const uint32_t t = s_wave[w]; if (w < wave) base += t; total += t; }
  __syncthreads();
  return base + x - v;
}

// One predictor's Rice sums: the lanes sum u >> k of their residuals res(n), n >= o, for every parameter k (registers), then fold them
// into the finest partitions' sums in LDS.  sm.cost[slot * 9 + p] starts at `base`, the subframe's bits in front of its partitions.
// The caller's barrier follows.
template <int BYTES, class RF> __device__ __forceinline__ void rice_accumulate(Smem<BYTES>& sm, int bs, int o, int slot, unsigned long long base, RF res) {
  constexpr int KLO = Smem<BYTES>::KLO, KHI = Smem<BYTES>::KHI;
  const int tid = threadIdx.x;
  const int pmax = max_porder(bs), s = bs >> pmax, T = kThreads >> pmax;    // T lanes share a finest partition
  const int j = tid / T, sub = tid - j * T;
  for (int i = tid; i < KLO * kParts; i += kThreads) sm.lo[i] = 0ull;
  if (KHI) for (int i = tid; i < KHI * kParts; i += kThreads) sm.hi[i] = 0u;
  if (tid < 9) sm.cost[slot * 9 + tid] = base;                               // the partitions' bits are added to it
  __syncthreads();
  unsigned long long alo[KLO];
  uint32_t ahi[KHI ? KHI : 1];
#pragma unroll
  for (int k = 0; k < KLO; ++k) alo[k] = 0ull;
#pragma unroll
  for (int k = 0; k < (KHI ? KHI : 1); ++k) ahi[k] = 0u;
  for (int n = j * s + sub; n < (j + 1) * s; n += T) {
    if (n < o) continue;
    const uint32_t u = zigzag(res(n));
#pragma unroll
    for (int k = 0; k < KLO; ++k) alo[k] += u >> k;
#pragma unroll
    for (int k = 0; k < KHI; ++k) ahi[k] += u >> (16 + k);
  }
#pragma unroll
  for (int k = 0; k < KLO; ++k) atomicAdd(&sm.lo[k * kParts + j], alo[k]);
#pragma unroll
  for (int k = 0; k < KHI; ++k) atomicAdd(&sm.hi[k * kParts + j], ahi[k]);
}

// Behind rice_accumulate and a barrier: the best k and the bits of every partition of every partition order, the coarser partitions
// being sums of pairs -> sm.cost[slot * 9 + p] of the admitted p, sm.kall[slot * 512 + 2^p - 1 + partition].  Ends on a barrier.
template <int BYTES> __device__ __forceinline__ void rice_fold(Smem<BYTES>& sm, int bs, int o, int slot) {
  constexpr int KLO = Smem<BYTES>::KLO, KHI = Smem<BYTES>::KHI, K = KLO + KHI, PBITS = BYTES == 2 ? 4 : 5;
  const int tid = threadIdx.x, pmax = max_porder(bs);
  for (int p = pmax; p >= 0; --p) {
    const int np = 1 << p;
    if ((bs >> p) > o && tid < np) {
      int kb; uint64_t b;
      best_k((uint64_t)((bs >> p) - (tid == 0 ? o : 0)), K,
             [&sm, tid](int k) -> uint64_t { return k < KLO ? (uint64_t)sm.lo[k * kParts + tid] : (uint64_t)sm.hi[(KHI ? k - KLO : 0) * kParts + tid]; }, kb, b);
      sm.kall[slot * 512 + np - 1 + tid] = (uint8_t)kb;
      atomicAdd(&sm.cost[slot * 9 + p], (unsigned long long)(PBITS + b));
    }
    if (p == 0) break;
    // the pairs' sums: read, barrier, write (a lane's target is another lane's source)
    const int half = np >> 1;
    unsigned long long rlo[8];
    uint32_t rhi[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int idx = tid + m * kThreads, k = idx >> (p - 1), jj = idx & (half - 1);
      rlo[m] = 0ull; rhi[m] = 0u;
      if (k < KLO) rlo[m] = sm.lo[k * kParts + 2 * jj] + sm.lo[k * kParts + 2 * jj + 1];
      if (k < KHI) rhi[m] = sm.hi[k * kParts + 2 * jj] + sm.hi[k * kParts + 2 * jj + 1];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int idx = tid + m * kThreads, k = idx >> (p - 1), jj = idx & (half - 1);
      if (k < KLO) sm.lo[k * kParts + jj] = rlo[m];
      if (k < KHI) sm.hi[k * kParts + jj] = rhi[m];
    }
    __syncthreads();
  }
  __syncthreads();
}

// The cheapest subframe of coded channel ch -> sm.type / o / p / bits [cand], its Rice parameters -> sm.ck[cand]
template <int BYTES> __device__ __forceinline__ void choose_dev(Smem<BYTES>& sm, const Geo& g, int ch, int bps, int cand) {
  const int tid = threadIdx.x, bs = g.bs;
  if (tid == 0) sm.neq = 0;
  const int32_t first = coded_at(g, ch, 0);
  bool constant = false;
  for (int o = 0; o <= 4 && o < bs; ++o) {
    bool neq = false;
    rice_accumulate<BYTES>(sm, bs, o, o, 8ull + (unsigned long long)(o * bps) + 6ull, [&](int n) -> int32_t {
      const int32_t r = residual(g, ch, o, n);
      if (o == 0 && r != first) neq = true;
      return r;
    });
    if (neq) sm.neq = 1;
    __syncthreads();
    if (o == 0 && sm.neq == 0) { constant = true; break; }
    rice_fold<BYTES>(sm, bs, o, o);
  }
  __syncthreads();
  int type = T_CONSTANT, o_ = 0, p_ = 0;
  uint64_t bits = 8 + (uint64_t)bps;
  if (!constant) pick_fixed(sm.cost, bs, bps, type, o_, p_, bits);
  if (type == T_FIXED && tid < (1 << p_)) sm.ck[cand * kParts + tid] = sm.kall[o_ * 512 + (1 << p_) - 1 + tid];
  if (tid == 0) { sm.type[cand] = type; sm.o[cand] = o_; sm.p[cand] = p_; sm.bits[cand] = bits; }
  __syncthreads();
}

// ---- device, LPC: what the LPC instantiations keep in dynamic LDS behind Smem: this record, the int32 image of the coded channel's
// block, the int16 analysis signal (lpc_v_in_sums: in sm.lo where it fits)
struct LpcSm {
  unsigned long long R[kLpcMax + 1];
  double lp[kLpcMax], nw[kLpcMax];
  int q[kLpcMax * kLpcMax], shift[kLpcMax], ok[kLpcMax];                    // row o - 1: lpc_fit's answer
  int cq[4 * kLpcMax], cshift[4];                                           // of the chosen LPC subframe of candidate cand
  uint32_t rmax;
  uint32_t pad;
};
template <int BYTES> constexpr size_t lpc_lds_offset() { return (sizeof(Smem<BYTES>) + 15) / 16 * 16; }
// The analysis signal is read before the first Rice pass of its channel zeroes sm.lo: where it fits (2 bytes a sample) it lives there,
// else behind the image.  At block 4096 that keeps two workgroups of either sample size on a CU's 160 KiB.
template <int BYTES> FHD bool lpc_v_in_sums(int block) { return (size_t)block * 2 <= sizeof(Smem<BYTES>::lo); }
template <int BYTES> size_t lpc_lds_bytes(int block) {
  return lpc_lds_offset<BYTES>() + sizeof(LpcSm) + (size_t)block * 4 + (lpc_v_in_sums<BYTES>(block) ? 0 : ((size_t)block * 2 + 15) / 16 * 16);
}

__device__ __forceinline__ void lpc_stage(int32_t* x, const Geo& g, int ch) {   // the coded channel's block -> LDS; ends on a barrier
  for (int n = threadIdx.x; n < g.bs; n += kThreads) x[n] = coded_at(g, ch, n);
  __syncthreads();
}

// Behind choose_dev, where the block is not CONSTANT: the analysis, the fit (lane 0), then every admitted order through the Rice
// accumulation and the partition fold (slot 0 of sm.cost / sm.kall, free again); a cheaper pair replaces candidate cand's choice.
template <int BYTES> __device__ __forceinline__ void choose_lpc_dev(Smem<BYTES>& sm, LpcSm& ls, int32_t* x, int16_t* v, const Geo& g, int ch, int bps, int M, int cand) {
  const int tid = threadIdx.x, bs = g.bs;
  if (sm.type[cand] == T_CONSTANT) return;                                   // (the same in every lane)
  const int Mo = min(M, bs - 1), pmax = max_porder(bs);
  for (int n = tid; n < bs; n += kThreads) { const int32_t a = coded_at(g, ch, n); x[n] = a; v[n] = (int16_t)lpc_value(a, bps, n, bs); }
  if (tid <= kLpcMax) ls.R[tid] = 0ull;
  __syncthreads();
  {
    long long acc[kLpcMax + 1];
#pragma unroll
    for (int l = 0; l <= kLpcMax; ++l) acc[l] = 0;
    for (int n = tid; n < bs; n += kThreads) {
      const long long vn = v[n];
#pragma unroll
      for (int l = 0; l <= kLpcMax; ++l) if (l <= Mo && n >= l) acc[l] += vn * (long long)v[n - l];
    }
#pragma unroll
    for (int l = 0; l <= kLpcMax; ++l) if (l <= Mo) atomicAdd(&ls.R[l], (unsigned long long)acc[l]);
  }
  __syncthreads();
  if (tid == 0) lpc_fit(reinterpret_cast<const long long*>(ls.R), Mo, ls.lp, ls.nw, ls.q, ls.shift, ls.ok);
  __syncthreads();
  int btype = sm.type[cand], bp = sm.p[cand];
  uint64_t bbits = sm.bits[cand];
  __syncthreads();
  for (int o = 1; o <= Mo; ++o) {
    if (!ls.ok[o - 1]) continue;
    const int* q = &ls.q[(o - 1) * kLpcMax];
    const int shift = ls.shift[o - 1];
    if (tid == 0) ls.rmax = 0u;
    uint32_t rmax = 0u;
    rice_accumulate<BYTES>(sm, bs, o, 0, lpc_base_bits(o, bps), [&](int n) -> int32_t {
      const int64_t r = lpc_residual(x, q, o, shift, n);
      rmax = max(rmax, lpc_size(r));
      return (int32_t)r;
    });
    atomicMax(&ls.rmax, rmax);
    __syncthreads();
    if (ls.rmax >= kLpcResLimit) { __syncthreads(); continue; }
    rice_fold<BYTES>(sm, bs, o, 0);
    for (int p = pmax; p >= 0; --p) {
      if ((bs >> p) <= o) continue;
      const uint64_t total = sm.cost[p];
      if (total < bbits || (btype == T_LPC && total == bbits && p < bp)) {
        btype = T_LPC; bp = p; bbits = total;                              // (a lane rewrites its own entries: no barrier between two wins)
        if (tid < (1 << p)) sm.ck[cand * kParts + tid] = sm.kall[(1 << p) - 1 + tid];
        if (tid < o) ls.cq[cand * kLpcMax + tid] = q[tid];
        if (tid == 0) { sm.type[cand] = T_LPC; sm.o[cand] = o; sm.p[cand] = p; sm.bits[cand] = total; ls.cshift[cand] = shift; }
      }
    }
    __syncthreads();
  }
  __syncthreads();
}

// LPC (the LPC instantiations; ls, x: their record and image, else null): an LPC subframe's header, and its residuals from the image,
// which is staged again here where `restage` says so: a stereo pair's four candidates went through it since (any other channel is
// written right behind its choice, with its image still there).  Its per-step uint32 totals hold: a chosen subframe is below
// VERBATIM's size.
template <int BYTES, bool LPC> __device__ __forceinline__ void emit_subframe(Smem<BYTES>& sm, LpcSm* ls, int32_t* x, Emit& e, const Geo& g, int ch, int bps, int cand,
                                                                             bool restage) {
  constexpr int PBITS = BYTES == 2 ? 4 : 5;
  const int tid = threadIdx.x, bs = g.bs;
  const int type = sm.type[cand], o = sm.o[cand], p = sm.p[cand];
  const uint32_t mask = (1u << bps) - 1u;                                    // bps <= 25
  uint32_t end = e.pos + 8u;
  const bool lpc = LPC && type == T_LPC;
  do { if (tid == 0) put(e, e.pos, (uint32_t)(type == T_CONSTANT ? 0 : type == T_VERBATIM ? 1 : lpc ? (32 | (o - 1)) : (8 | o)) << 1, 8); } while (emit_more(e, end));
  e.pos = end;
  if (type == T_CONSTANT) {
    end = e.pos + (uint32_t)bps;
    do { if (tid == 0) put(e, e.pos, (uint32_t)coded_at(g, ch, 0) & mask, bps); } while (emit_more(e, end));
    e.pos = end;
    return;
  }
  if (type == T_VERBATIM) {
    for (int n0 = 0; n0 < bs; n0 += kThreads) {
      const int cnt = min(kThreads, bs - n0);
      end = e.pos + (uint32_t)(cnt * bps);
      do { if (tid < cnt) put(e, e.pos + (uint32_t)(tid * bps), (uint32_t)coded_at(g, ch, n0 + tid) & mask, bps); } while (emit_more(e, end));
      e.pos = end;
    }
    return;
  }
  end = e.pos + (uint32_t)(o * bps);
  do { if (tid < o) put(e, e.pos + (uint32_t)(tid * bps), (uint32_t)coded_at(g, ch, tid) & mask, bps); } while (emit_more(e, end));
  e.pos = end;
  int shift = 0;
  const int* cq = nullptr;
  if constexpr (LPC) {
    if (lpc) {
      shift = ls->cshift[cand];
      cq = &ls->cq[cand * kLpcMax];
      end = e.pos + 9u + (uint32_t)(o * kLpcPrec);
      do {
        if (tid == 0) put(e, e.pos, (uint32_t)((kLpcPrec - 1) << 5 | shift), 9);
        if (tid < o) put(e, e.pos + 9u + (uint32_t)(tid * kLpcPrec), (uint32_t)cq[tid] & ((1u << kLpcPrec) - 1u), kLpcPrec);
      } while (emit_more(e, end));
      e.pos = end;
      if (restage) lpc_stage(x, g, ch);
    }
  }
  end = e.pos + 6u;
  do { if (tid == 0) put(e, e.pos, (uint32_t)((BYTES == 3 ? 1 : 0) << 4 | p), 6); } while (emit_more(e, end));
  e.pos = end;
  const int psize = bs >> p;
  for (int n0 = o; n0 < bs; n0 += kThreads) {
    const int n = n0 + tid;
    uint32_t u = 0, q = 0, head = 0, len = 0;
    int k = 0;
    if (n < bs) {
      if constexpr (LPC) u = zigzag(lpc ? (int32_t)lpc_residual(x, cq, o, shift, n) : residual(g, ch, o, n));
      else u = zigzag(residual(g, ch, o, n));
      const int jp = n / psize;
      k = sm.ck[cand * kParts + jp];
      head = (n == o || n == jp * psize) ? (uint32_t)PBITS : 0u;
      q = u >> k;
      len = head + q + 1u + (uint32_t)k;
    }
    uint32_t total;
    const uint32_t off = exscan256(len, sm.wave, total);
    end = e.pos + total;
    do {
      if (n < bs) {
        if (head) put(e, e.pos + off, (uint32_t)k, PBITS);
        put(e, e.pos + off + head + q, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
      }
    } while (emit_more(e, end));
    e.pos = end;
  }
}

extern __shared__ __align__(16) unsigned char flacenc_dyn_lds[];            // the LPC instantiations': Smem, LpcSm, the image, the analysis signal

template <int BYTES, bool LPC> __device__ __forceinline__ Smem<BYTES>& smem_of() {
  if constexpr (LPC) return *reinterpret_cast<Smem<BYTES>*>(flacenc_dyn_lds);
  else { __shared__ Smem<BYTES> sm; return sm; }
}

// CRC false (p2phd_flac_encode_stage, measurement only): the frame's CRC-16 is not taken and written as zeros.  LPC true
// (p2phd_flac_encode_lpc with lpc_order M > 0): every coded channel's choice goes through choose_lpc_dev as well; dynamic LDS of
// lpc_lds_bytes(block).
template <int BYTES, bool CRC, bool LPC> __global__ __launch_bounds__(kThreads) void flacenc_frames_kernel(const uint8_t* __restrict__ pcm, long L, int C, int rate, int block,
                                                                                     uint8_t* slots, long slot_bytes, long long* __restrict__ wlen, int M) {
  constexpr int BITS = BYTES * 8;
  Smem<BYTES>& sm = smem_of<BYTES, LPC>();
  LpcSm* ls = LPC ? reinterpret_cast<LpcSm*>(flacenc_dyn_lds + lpc_lds_offset<BYTES>()) : nullptr;
  int32_t* lx = LPC ? reinterpret_cast<int32_t*>(flacenc_dyn_lds + lpc_lds_offset<BYTES>() + sizeof(LpcSm)) : nullptr;
  int16_t* lv = !LPC ? nullptr : lpc_v_in_sums<BYTES>(block) ? reinterpret_cast<int16_t*>(sm.lo) : reinterpret_cast<int16_t*>(lx + block);
  const int tid = threadIdx.x;
  const long f = blockIdx.x;
  Geo g{pcm, C, BYTES, (int64_t)f * block, (int)min((long)block, L - f * block)};
  uint8_t* slot8 = slots + f * slot_bytes;
  Emit e{sm.win, reinterpret_cast<uint32_t*>(slot8), 0u, 0u};
  for (int i = tid; i < kWin; i += kThreads) sm.win[i] = 0u;
  sm.t16[tid] = (uint16_t)crc16_entry(tid);
  __syncthreads();
  int assign = C - 1, ca = 0, cb = 1;
  if (C == 2) {
    choose_dev<BYTES>(sm, g, 0, BITS, 0);
    if constexpr (LPC) choose_lpc_dev<BYTES>(sm, *ls, lx, lv, g, 0, BITS, M, 0);
    choose_dev<BYTES>(sm, g, 1, BITS, 1);
    if constexpr (LPC) choose_lpc_dev<BYTES>(sm, *ls, lx, lv, g, 1, BITS, M, 1);
    choose_dev<BYTES>(sm, g, kMid, BITS, 2);
    if constexpr (LPC) choose_lpc_dev<BYTES>(sm, *ls, lx, lv, g, kMid, BITS, M, 2);
    choose_dev<BYTES>(sm, g, kSide, BITS + 1, 3);
    if constexpr (LPC) choose_lpc_dev<BYTES>(sm, *ls, lx, lv, g, kSide, BITS + 1, M, 3);
    assign = pick_assign(sm.bits[0], sm.bits[1], sm.bits[2], sm.bits[3]);
    ca = assign == 9 ? 3 : assign == 10 ? 2 : 0;
    cb = assign == 1 || assign == 9 ? 1 : 3;
  }
  if (tid == 0) sm.hlen = build_header(sm.hdr, g.bs, rate, assign, BITS, (uint32_t)f);
  __syncthreads();
  {
    const int hlen = sm.hlen;
    const uint32_t end = (uint32_t)hlen * 8u;
    do { if (tid < hlen) put(e, (uint32_t)tid * 8u, sm.hdr[tid], 8); } while (emit_more(e, end));
    e.pos = end;
  }
  if (C == 2) {
    emit_subframe<BYTES, LPC>(sm, ls, lx, e, g, ca == 0 ? 0 : ca == 2 ? kMid : kSide, BITS + (ca == 3), ca, true);
    emit_subframe<BYTES, LPC>(sm, ls, lx, e, g, cb == 1 ? 1 : kSide, BITS + (cb == 3), cb, true);
  } else {
    for (int c = 0; c < C; ++c) {
      choose_dev<BYTES>(sm, g, c, BITS, 0);
      if constexpr (LPC) choose_lpc_dev<BYTES>(sm, *ls, lx, lv, g, c, BITS, M, 0);
      emit_subframe<BYTES, LPC>(sm, ls, lx, e, g, c, BITS, 0, false);
    }
  }
  // zero bits to the byte boundary are there already; the rest of the window goes out, whole words (the slot has the room)
  const uint32_t nbytes = (e.pos + 7u) >> 3, nwords = (nbytes + 3u) >> 2;
  if (tid == 0) sm.crc = 0u;
  __syncthreads();
  for (uint32_t i = e.wbase + tid; i < nwords; i += kThreads) e.slot[i] = __builtin_bswap32(sm.win[i - e.wbase]);
  __syncthreads();
  // CRC-16 of the frame's bytes, as this workgroup stored them: a piece of whole words per lane, the last 0 .. 3 bytes by lane 0
  if (CRC) {
    const uint32_t nw = nbytes >> 2, cw = (nw + kThreads - 1) / kThreads;
    const uint32_t a = min((uint32_t)tid * cw, nw), b = min(a + cw, nw);
    uint32_t c = 0;
    for (uint32_t i = a; i < b; ++i) {
      const uint32_t w = e.slot[i];
      c = ((c << 8) ^ sm.t16[(c >> 8) ^ (w & 0xFFu)]) & 0xFFFFu;
      c = ((c << 8) ^ sm.t16[(c >> 8) ^ ((w >> 8) & 0xFFu)]) & 0xFFFFu;
      c = ((c << 8) ^ sm.t16[(c >> 8) ^ ((w >> 16) & 0xFFu)]) & 0xFFFFu;
      c = ((c << 8) ^ sm.t16[(c >> 8) ^ (w >> 24)]) & 0xFFFFu;
    }
    if (b > a) atomicXor(&sm.crc, gf_mul(c, gf_xpow8((uint64_t)(nbytes - 4u * b))));
    if (tid == 0) {
      uint32_t t = 0;
      for (uint32_t i = 4u * nw; i < nbytes; ++i) t = ((t << 8) ^ sm.t16[(t >> 8) ^ slot8[i]]) & 0xFFFFu;
      if (nbytes > 4u * nw) atomicXor(&sm.crc, t);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t c = sm.crc;
    slot8[nbytes] = (uint8_t)(c >> 8);
    slot8[nbytes + 1u] = (uint8_t)c;
    wlen[f] = (long long)nbytes + 2;
  }
}

// one workgroup: the frames' lengths -> their offsets in the stream (workspace) and `lengths` with the total behind them
__global__ __launch_bounds__(kScan) void flacenc_scan_kernel(const long long* __restrict__ wlen, long nframes, long long* __restrict__ woff,
                                                             long long* __restrict__ lengths) {
  __shared__ long long s_w[kScan / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long long carry = 0;
  for (long base = 0; base < nframes; base += kScan) {
    const long i = base + tid;
    const long long v = i < nframes ? wlen[i] : 0;
    long long x = v;
    for (int d = 1; d < 64; d <<= 1) { const long long t = __shfl_up(x, d, 64); if (lane >= d) x += t; }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    long long before = 0, total = 0;
    for (int w = 0; w < kScan / 64; ++w) { const long long t = s_w[w]; if (w < wave) before += t; total += t; }
    __syncthreads();
    if (i < nframes) { woff[i] = carry + before + x - v; lengths[i] = v; }
    carry += total;
  }
  if (tid == 0) lengths[nframes] = carry;
}

__global__ __launch_bounds__(kThreads) void flacenc_gather_kernel(const uint8_t* __restrict__ slots, long slot_bytes, const long long* __restrict__ wlen,
                                                                  const long long* __restrict__ woff, uint8_t* __restrict__ stream) {
  const long f = blockIdx.x;
  const uint8_t* src = slots + f * slot_bytes;
  uint8_t* dst = stream + woff[f];
  const long n = wlen[f];
  for (long i = threadIdx.x; i < n; i += kThreads) dst[i] = src[i];
}
#endif

}  // namespace

extern "C" int p2phd_flac_encode_plan(int channels, int bits, int64_t L, int block, int64_t* nframes, int64_t* max_stream_bytes, int64_t* workspace_bytes) {
  const char* what = "flac_encode_plan";
  if (int rc = check_args(what, channels, bits, L, 1, block)) return rc;
  P2PHD_REQUIRE(nframes && max_stream_bytes && workspace_bytes, "%s: null pointer", what);
  const int64_t n = (L + block - 1) / block;
  const int last = (int)(L - (n - 1) * block);
  *nframes = n;
  *max_stream_bytes = (n - 1) * worst_frame_bytes(channels, bits, block) + worst_frame_bytes(channels, bits, last);
  *workspace_bytes = n * (16 + slot_bytes_of(channels, bits, block));
  return P2PHD_OK;
}

extern "C" int p2phd_flac_encode_threads(void) { return kThreads; }
extern "C" int p2phd_flac_encode_scan_threads(void) { return kScan; }
extern "C" int p2phd_flac_encode_window_words(void) { return kWin; }

namespace {
int flac_encode_host(const char* what, const void* payload, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream,
                     int64_t cap, int64_t* lengths) {
  if (int rc = check_args(what, channels, bits, L, rate, block)) return rc;
  if (int rc = check_lpc(what, lpc_order, block)) return rc;
  P2PHD_REQUIRE(payload && stream && lengths, "%s: null pointer", what);
  int64_t nframes, worst, wsb;
  p2phd_flac_encode_plan(channels, bits, L, block, &nframes, &worst, &wsb);
  P2PHD_REQUIRE(cap >= worst, "%s: the stream buffer holds %lld bytes, the plan's worst case is %lld", what, (long long)cap, (long long)worst);
  static const struct Table { uint16_t t[256]; Table() { for (int i = 0; i < 256; ++i) t[i] = (uint16_t)crc16_entry(i); } } crc;
  const int K = bits == 16 ? 15 : 31, pbits = bits == 16 ? 4 : 5;
  std::vector<uint64_t> sums((size_t)kParts * K);
  std::vector<Choice> ch(4);
  uint8_t* out = static_cast<uint8_t*>(stream);
  int64_t at = 0;
  for (int64_t f = 0; f < nframes; ++f) {
    Geo g{static_cast<const uint8_t*>(payload), channels, bits / 8, f * block, (int)std::min<int64_t>(block, L - f * block)};
    int assign = channels - 1, ca = 0, cb = 1;
    if (channels == 2) {
      const int chs[4] = {0, 1, kMid, kSide};
      for (int i = 0; i < 4; ++i) {
        choose_host(g, chs[i], bits + (i == 3), K, pbits, ch[i], sums);
        choose_lpc_host(g, chs[i], bits + (i == 3), K, pbits, lpc_order, ch[i], sums);
      }
      assign = pick_assign(ch[0].bits, ch[1].bits, ch[2].bits, ch[3].bits);
      ca = assign == 9 ? 3 : assign == 10 ? 2 : 0;
      cb = assign == 1 || assign == 9 ? 1 : 3;
    }
    const int64_t start = at;
    at += build_header(out + at, g.bs, rate, assign, bits, (uint32_t)f);
    Writer w{out, at, 0, 0};
    if (channels == 2) {
      const int chs[4] = {0, 1, kMid, kSide};
      write_subframe_host(w, g, chs[ca], bits + (ca == 3), pbits, ch[ca]);
      write_subframe_host(w, g, chs[cb], bits + (cb == 3), pbits, ch[cb]);
    } else {
      for (int c = 0; c < channels; ++c) {
        choose_host(g, c, bits, K, pbits, ch[0], sums);
        choose_lpc_host(g, c, bits, K, pbits, lpc_order, ch[0], sums);
        write_subframe_host(w, g, c, bits, pbits, ch[0]);
      }
    }
    w.align();
    at = w.at;
    uint32_t c = 0;
    for (int64_t i = start; i < at; ++i) c = ((c << 8) ^ crc.t[(c >> 8) ^ out[i]]) & 0xFFFFu;
    out[at++] = (uint8_t)(c >> 8);
    out[at++] = (uint8_t)c;
    lengths[f] = at - start;
  }
  lengths[nframes] = at;
  return P2PHD_OK;
}
}  // namespace

extern "C" int p2phd_flac_encode_host(const void* payload, int channels, int bits, int64_t L, int rate, int block, void* stream, int64_t cap,
                                      int64_t* lengths) {
  return flac_encode_host("flac_encode_host", payload, channels, bits, L, rate, block, 0, stream, cap, lengths);
}

extern "C" int p2phd_flac_encode_lpc_host(const void* payload, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream,
                                          int64_t cap, int64_t* lengths) {
  return flac_encode_host("flac_encode_lpc_host", payload, channels, bits, L, rate, block, lpc_order, stream, cap, lengths);
}

extern "C" int p2phd_flac_lpc_fit(const int64_t* R, int orders, int32_t* admitted, int32_t* q, int32_t* shift) {
  const char* what = "flac_lpc_fit";
  P2PHD_REQUIRE(R && admitted && q && shift, "%s: null pointer", what);
  P2PHD_REQUIRE(orders >= 0 && orders <= kLpcMax, "%s: need 0 <= orders <= %d (orders %d)", what, kLpcMax, orders);
  for (int l = 0; l <= orders; ++l)
    P2PHD_REQUIRE(R[l] > -(int64_t(1) << 53) && R[l] < (int64_t(1) << 53), "%s: R[%d] is not exact as a double", what, l);
  long long r[kLpcMax + 1] = {};
  for (int l = 0; l <= orders; ++l) r[l] = R[l];
  int qq[kLpcMax * kLpcMax] = {}, ss[kLpcMax] = {}, ok[kLpcMax];
  double lp[kLpcMax], nw[kLpcMax];
  lpc_fit(r, orders, lp, nw, qq, ss, ok);
  for (int o = 0; o < kLpcMax; ++o) {
    admitted[o] = ok[o]; shift[o] = ok[o] ? ss[o] : 0;
    for (int j = 0; j < kLpcMax; ++j) q[o * kLpcMax + j] = ok[o] && j <= o ? qq[o * kLpcMax + j] : 0;
  }
  return P2PHD_OK;
}

extern "C" int p2phd_flac_lpc_analyse(const int32_t* samples, int bs, int bps, int lpc_order, int32_t* admitted, int32_t* q, int32_t* shift, int64_t* R) {
  const char* what = "flac_lpc_analyse";
  P2PHD_REQUIRE(samples && admitted && q && shift && R, "%s: null pointer", what);
  P2PHD_REQUIRE(bs >= 1 && bs <= kLpcBlock, "%s: need 1 <= bs <= %d (bs %d)", what, kLpcBlock, bs);
  P2PHD_REQUIRE(bps == 16 || bps == 17 || bps == 24 || bps == 25, "%s: bps must be 16, 17, 24 or 25 (bps %d)", what, bps);
  P2PHD_REQUIRE(lpc_order >= 1 && lpc_order <= kLpcMax, "%s: need 1 <= lpc_order <= %d (lpc_order %d)", what, kLpcMax, lpc_order);
  const int64_t lim = int64_t(1) << (bps - 1);
  for (int n = 0; n < bs; ++n) P2PHD_REQUIRE(samples[n] >= -lim && samples[n] < lim, "%s: sample %d (%d) does not fit %d bits", what, n, samples[n], bps);
  long long r[kLpcMax + 1];
  int qq[kLpcMax * kLpcMax] = {}, ss[kLpcMax] = {}, ok[kLpcMax];
  lpc_analyse_host(samples, bs, bps, lpc_order, r, qq, ss, ok);
  for (int l = 0; l <= kLpcMax; ++l) R[l] = r[l];
  for (int o = 0; o < kLpcMax; ++o) {
    admitted[o] = ok[o]; shift[o] = ok[o] ? ss[o] : 0;
    for (int j = 0; j < kLpcMax; ++j) q[o * kLpcMax + j] = ok[o] && j <= o ? qq[o * kLpcMax + j] : 0;
  }
  return P2PHD_OK;
}

namespace {
// stage 0: the three kernels; 1 / 2 (p2phd_flac_encode_stage): the frame kernel alone, with / without its CRC-16
template <int BYTES, bool CRC> int launch_lpc(const char* what, dim3 grid, hipStream_t st, const uint8_t* pcm, long L, int channels, int rate, int block,
                                              uint8_t* slots, long sb, long long* wlen, int M) {
  static bool lds_set[64] = {};                                             // (the attribute is per device)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { p2phd::set_error("%s: no HIP device", what); return P2PHD_ELAUNCH; }
  if (!lds_set[dev]) {
    const size_t most = lpc_lds_bytes<BYTES>(kLpcBlock);                     // above the 64 KiB a kernel gets unasked
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(flacenc_frames_kernel<BYTES, CRC, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most) != hipSuccess) {
      (void)hipGetLastError();
      p2phd::set_error("%s: the device refuses %zu bytes of LDS per workgroup", what, most);
      return P2PHD_ELAUNCH;
    }
    lds_set[dev] = true;
  }
  hipLaunchKernelGGL((flacenc_frames_kernel<BYTES, CRC, true>), grid, dim3(kThreads), lpc_lds_bytes<BYTES>(block), st, pcm, L, channels, rate, block, slots, sb, wlen, M);
  return P2PHD_OK;
}

int flac_encode(const char* what, int stage, const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream_dev,
                int64_t cap, int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_args(what, channels, bits, L, rate, block)) return rc;
  if (int rc = check_lpc(what, lpc_order, block)) return rc;
  P2PHD_REQUIRE(payload_dev && stream_dev && lengths_dev && workspace, "%s: null pointer", what);
  int64_t nframes, worst, wsb;
  p2phd_flac_encode_plan(channels, bits, L, block, &nframes, &worst, &wsb);
  P2PHD_REQUIRE(cap >= worst, "%s: the stream buffer holds %lld bytes, the plan's worst case is %lld", what, (long long)cap, (long long)worst);
  P2PHD_REQUIRE(workspace_bytes >= wsb, "%s: the workspace holds %lld bytes, the plan asks for %lld", what, (long long)workspace_bytes, (long long)wsb);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(lengths_dev) & 7) == 0,
                "%s: workspace or lengths is not aligned to 8 bytes", what);
  hipStream_t st = (hipStream_t)stream;
  long long* wlen = static_cast<long long*>(workspace);
  long long* woff = wlen + nframes;
  uint8_t* slots = reinterpret_cast<uint8_t*>(woff + nframes);
  const long sb = (long)slot_bytes_of(channels, bits, block);
  const uint8_t* pcm = static_cast<const uint8_t*>(payload_dev);
  const dim3 grid((unsigned)nframes), lanes(kThreads);
  if (lpc_order > 0) {
    int rc;
    if (bits == 16 && stage != 2) rc = launch_lpc<2, true>(what, grid, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, lpc_order);
    else if (bits == 16) rc = launch_lpc<2, false>(what, grid, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, lpc_order);
    else if (stage != 2) rc = launch_lpc<3, true>(what, grid, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, lpc_order);
    else rc = launch_lpc<3, false>(what, grid, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, lpc_order);
    if (rc) return rc;
  }
  else if (bits == 16 && stage != 2) hipLaunchKernelGGL((flacenc_frames_kernel<2, true, false>), grid, lanes, 0, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, 0);
  else if (bits == 16) hipLaunchKernelGGL((flacenc_frames_kernel<2, false, false>), grid, lanes, 0, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, 0);
  else if (stage != 2) hipLaunchKernelGGL((flacenc_frames_kernel<3, true, false>), grid, lanes, 0, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, 0);
  else hipLaunchKernelGGL((flacenc_frames_kernel<3, false, false>), grid, lanes, 0, st, pcm, (long)L, channels, rate, block, slots, sb, wlen, 0);
  if (stage == 0) {
    hipLaunchKernelGGL(flacenc_scan_kernel, dim3(1), dim3(kScan), 0, st, wlen, (long)nframes, woff, reinterpret_cast<long long*>(lengths_dev));
    hipLaunchKernelGGL(flacenc_gather_kernel, grid, lanes, 0, st, slots, sb, wlen, woff, static_cast<uint8_t*>(stream_dev));
  }
  p2phd::g_launch_count[p2phd::LC_FLACENC] += stage ? 1 : 3;
  return p2phd::check_launch(what);
}
}  // namespace

extern "C" int p2phd_flac_encode(const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, void* stream_dev, int64_t cap,
                                 int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return flac_encode("flac_encode", 0, payload_dev, channels, bits, L, rate, block, 0, stream_dev, cap, lengths_dev, workspace, workspace_bytes, stream);
}

extern "C" int p2phd_flac_encode_lpc(const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream_dev,
                                     int64_t cap, int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  return flac_encode("flac_encode_lpc", 0, payload_dev, channels, bits, L, rate, block, lpc_order, stream_dev, cap, lengths_dev, workspace, workspace_bytes, stream);
}

extern "C" int p2phd_flac_encode_stage(int stage, const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, void* stream_dev, int64_t cap,
                                       int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  P2PHD_REQUIRE(stage == 1 || stage == 2, "flac_encode_stage: stage must be 1 (the frame kernel alone) or 2 (the frame kernel without its CRC-16), got %d", stage);
  return flac_encode("flac_encode_stage", stage, payload_dev, channels, bits, L, rate, block, 0, stream_dev, cap, lengths_dev, workspace, workspace_bytes, stream);
}

extern "C" int p2phd_flac_encode_lpc_stage(int stage, const void* payload_dev, int channels, int bits, int64_t L, int rate, int block, int lpc_order, void* stream_dev,
                                           int64_t cap, int64_t* lengths_dev, void* workspace, int64_t workspace_bytes, void* stream) {
  P2PHD_REQUIRE(stage == 1 || stage == 2, "flac_encode_lpc_stage: stage must be 1 (the frame kernel alone) or 2 (the frame kernel without its CRC-16), got %d", stage);
  return flac_encode("flac_encode_lpc_stage", stage, payload_dev, channels, bits, L, rate, block, lpc_order, stream_dev, cap, lengths_dev, workspace, workspace_bytes,
                     stream);
}
