// FLAC input (native streams, RFC 9639 subset of include/p2phd.h): the reader in front of the feeder (host) and of whole-file
// generation (device).  Launch family "flac".
//
//   host    p2phd_flac_info            "fLaC" (behind an optional ID3v2 tag), the metadata blocks, STREAMINFO
//           p2phd_flac_index           one row per frame: every header's CRC-8, every frame's CRC-16, the chain of frames without a gap
//                                      from the first frame to the end of the file, consecutive sample numbers.  A frame ends where its
//                                      CRC-16 closes AND the next header stands (or the file ends): bytes inside a frame that look like a
//                                      header do not close the CRC-16 in front of them, so they do not split it.  No sample is decoded.
//           p2phd_flac_decode_host     the reference decoder: frames of the table -> planar int32
//   device  p2phd_flac_decode          flac_frames_kernel: one LANE owns one frame -- a subframe starts where the Rice codes in front of it
//                                      end and the predictor is an integer recursion, so the frame is the unit that has no neighbour.  The
//                                      lane reads its frame in 8-byte pieces, parses the subframes, decodes the residual, runs the
//                                      predictor and leaves every channel's integers (wasted bits restored) in the int32 workspace
//                                      [channels][ld].  flac_pcm_kernel: one workgroup per frame, element-wise: undoes the stereo
//                                      decorrelation and scales to fp32, coalesced on both sides.
//
// Both decoders are ONE routine (decode_frame, __host__ __device__) over a storage policy: where the predictor's coefficients and its
// history of 32 samples live (host: two arrays; device: two LDS columns of the lane, indexed by run-time values -- LDS, not scratch) and
// where a sample goes.  Every prediction sum is 64-bit (v_mad_i64_i32 on the device).  Every read goes through a bit reader that
// knows [offset, offset + length) of the frame's table row and never loads outside it, whatever the bits say: running out of bits is a
// reason code, not an overrun.
#include "common.h"
#include "convplan.h"
#include <algorithm>
#include <cstdint>
#include <cstring>

#define FHD __host__ __device__ __forceinline__

namespace {
constexpr int kRow = P2PHD_FLAC_ROW_WORDS;     // int64 words of a table row: offset, length, first sample, block size, assignment, bits
constexpr int kLanes = 64;                     // frames per workgroup of flac_frames_kernel: one wave
constexpr int kTile = 256;                     // threads (samples per step) of flac_pcm_kernel
constexpr int kHist = 32;                      // the longest predictor

// ---- bit reader, MSB first, bounded by [p, end) ---------------------------------------------------------------------------
// buf: the next n bits at the top, zeros below them
struct Reader { const uint8_t* b; int64_t p, end; uint64_t buf; int n; int bad; };

FHD uint64_t load_be64(const uint8_t* p) { uint64_t w; __builtin_memcpy(&w, p, 8); return __builtin_bswap64(w); }

FHD void rd_init(Reader& r, const uint8_t* b, int64_t off, int64_t len) { r.b = b; r.p = off; r.end = off + len; r.buf = 0; r.n = 0; r.bad = 0; }

FHD void rd_fill(Reader& r) {
  if (r.n > 56) return;
  if (r.p + 8 <= r.end) {                                       // a whole 8-byte piece lies inside the frame
    const uint64_t w = load_be64(r.b + r.p);
    const int k = (64 - r.n) >> 3;                              // whole bytes that fit
    r.buf |= w >> r.n;
    r.p += k; r.n += 8 * k;
    if (r.n < 64) r.buf &= ~0ull << (64 - r.n);
  } else {
    while (r.n <= 56 && r.p < r.end) { r.buf |= (uint64_t)r.b[r.p++] << (56 - r.n); r.n += 8; }
  }
}

FHD void rd_fail(Reader& r) { r.bad = 1; r.n = 0; r.buf = 0; r.p = r.end; }

FHD uint32_t rd_bits(Reader& r, int k) {                        // 0 <= k <= 32
  if (k == 0) return 0u;
  if (r.n < k) { rd_fill(r); if (r.n < k) { rd_fail(r); return 0u; } }
  const uint32_t v = (uint32_t)(r.buf >> (64 - k));
  r.buf <<= k; r.n -= k;
  return v;
}

FHD int32_t rd_sbits(Reader& r, int k) {                        // two's complement of k bits; k = 0: 0
  if (k == 0) return 0;
  return (int32_t)(rd_bits(r, k) << (32 - k)) >> (32 - k);
}

FHD uint32_t rd_unary(Reader& r) {                              // zeros in front of the next 1, which is consumed
  uint32_t q = 0u;
  for (;;) {
    if (r.n == 0) { rd_fill(r); if (r.n == 0) { rd_fail(r); return q; } }
    if (r.buf) {
      const int z = __builtin_clzll(r.buf);                     // < n: nothing is set below the n valid bits
      q += (uint32_t)z; r.buf = (r.buf << z) << 1; r.n -= z + 1;
      return q;
    }
    q += (uint32_t)r.n; r.n = 0;
  }
}

FHD int64_t rd_consumed_bits(const Reader& r, int64_t off) { return (r.p - off) * 8 - r.n; }

// ---- one frame -------------------------------------------------------------------------------------------------------------
// P: coef_set(i, v) / coef(i), i < 32; hist_set(n, v) / hist(n), n a sample index, the last 32 kept; store(c, n, v)
template <class P> FHD int decode_subframe(P& pol, Reader& r, int bs, int bps, int c) {
  if (rd_bits(r, 1)) return P2PHD_FLAC_E_RESERVED;
  const int type = (int)rd_bits(r, 6);
  int wasted = 0;
  if (rd_bits(r, 1)) {
    wasted = (int)rd_unary(r) + 1;
    if (r.bad) return P2PHD_FLAC_E_BITS;
    if (wasted >= bps) return P2PHD_FLAC_E_RESERVED;
    bps -= wasted;
  }
  if (type == 0) {
    const uint32_t v = (uint32_t)rd_sbits(r, bps) << wasted;
    for (int n = 0; n < bs; ++n) pol.store(c, n, (int32_t)v);
    return r.bad ? P2PHD_FLAC_E_BITS : P2PHD_FLAC_OK;
  }
  if (type == 1) {
    for (int n = 0; n < bs; ++n) pol.store(c, n, (int32_t)((uint32_t)rd_sbits(r, bps) << wasted));
    return r.bad ? P2PHD_FLAC_E_BITS : P2PHD_FLAC_OK;
  }
  int order, shift = 0;
  const bool lpc = (type & 0x20) != 0;
  if (lpc) order = (type & 31) + 1;
  else if ((type & 0x38) == 0x08) { order = type & 7; if (order > 4) return P2PHD_FLAC_E_RESERVED; }
  else return P2PHD_FLAC_E_RESERVED;
  if (order > bs) return P2PHD_FLAC_E_GEOMETRY;
  for (int n = 0; n < order; ++n) {
    const int32_t v = rd_sbits(r, bps);
    pol.hist_set(n, v);
    pol.store(c, n, (int32_t)((uint32_t)v << wasted));
  }
  if (lpc) {
    const int prec = (int)rd_bits(r, 4) + 1;
    if (prec == 16) return P2PHD_FLAC_E_RESERVED;
    shift = rd_sbits(r, 5);
    if (shift < 0) return P2PHD_FLAC_E_RESERVED;
    for (int i = 0; i < order; ++i) pol.coef_set(i, rd_sbits(r, prec));
  } else {                                                      // the fixed predictors are these polynomials
    if (order == 1) pol.coef_set(0, 1);
    if (order == 2) { pol.coef_set(0, 2); pol.coef_set(1, -1); }
    if (order == 3) { pol.coef_set(0, 3); pol.coef_set(1, -3); pol.coef_set(2, 1); }
    if (order == 4) { pol.coef_set(0, 4); pol.coef_set(1, -6); pol.coef_set(2, 4); pol.coef_set(3, -1); }
  }
  if (r.bad) return P2PHD_FLAC_E_BITS;
  const int method = (int)rd_bits(r, 2);
  if (method >= 2) return P2PHD_FLAC_E_RESERVED;
  const int pbits = method ? 5 : 4;
  const int escape = (1 << pbits) - 1;
  const int porder = (int)rd_bits(r, 4);
  if (r.bad) return P2PHD_FLAC_E_BITS;
  const int parts = 1 << porder;
  if (porder > 0 && (bs & (parts - 1))) return P2PHD_FLAC_E_GEOMETRY;
  const int psize = bs >> porder;
  if (psize < order) return P2PHD_FLAC_E_GEOMETRY;
  int n = order;
  for (int part = 0; part < parts; ++part) {
    const int count = psize - (part == 0 ? order : 0);
    const int k = (int)rd_bits(r, pbits);
    const int raw = k == escape ? (int)rd_bits(r, 5) : 0;
    for (int j = 0; j < count; ++j, ++n) {
      int64_t res;
      if (k == escape) res = rd_sbits(r, raw);
      else {
        const uint64_t q = rd_unary(r);
        const uint64_t u = (q << k) | rd_bits(r, k);
        res = (int64_t)(u >> 1) ^ -(int64_t)(u & 1u);
      }
      int64_t acc = 0;
      for (int i = 0; i < order; ++i) acc += (int64_t)pol.coef(i) * (int64_t)pol.hist(n - 1 - i);
      const int32_t v = (int32_t)(res + (acc >> shift));
      pol.hist_set(n, v);
      pol.store(c, n, (int32_t)((uint32_t)v << wasted));
    }
    if (r.bad) return P2PHD_FLAC_E_BITS;
  }
  return P2PHD_FLAC_OK;
}

// The frame at [off, off + len) with the table row's block size, channel assignment and bits -> a P2PHD_FLAC_* reason code.  The
// header was verified by the index: here only its length is worked out.
template <class P> FHD int decode_frame(P& pol, const uint8_t* bytes, int64_t off, int64_t len, int bs, int assign, int bits, int channels) {
  if (assign < 0 || assign > 10) return P2PHD_FLAC_E_RESERVED;
  if ((assign < 8 ? assign + 1 : 2) != channels) return P2PHD_FLAC_E_ROW;
  Reader r;
  rd_init(r, bytes, off, len);
  const uint32_t b0 = rd_bits(r, 8), b1 = rd_bits(r, 8), b2 = rd_bits(r, 8);
  rd_bits(r, 8);
  if (b0 != 0xFFu || (b1 & 0xFEu) != 0xF8u) return r.bad ? P2PHD_FLAC_E_BITS : P2PHD_FLAC_E_RESERVED;
  const uint32_t lead = rd_bits(r, 8);
  const int ones = lead == 0xFFu ? 8 : __builtin_clz(~(lead << 24));
  if (ones == 1 || ones == 8) return P2PHD_FLAC_E_RESERVED;
  for (int i = 1; i < ones; ++i) rd_bits(r, 8);
  const int bscode = (int)(b2 >> 4), srcode = (int)(b2 & 15u);
  if (bscode == 6) rd_bits(r, 8);
  if (bscode == 7) rd_bits(r, 16);
  if (srcode == 12) rd_bits(r, 8);
  if (srcode == 13 || srcode == 14) rd_bits(r, 16);
  rd_bits(r, 8);                                                // CRC-8
  if (r.bad) return P2PHD_FLAC_E_BITS;
  for (int c = 0; c < channels; ++c) {
    const int side = (assign == 8 && c == 1) || (assign == 9 && c == 0) || (assign == 10 && c == 1);
    const int rc = decode_subframe(pol, r, bs, bits + side, c);
    if (rc) return rc;
  }
  const int pad = (int)((-rd_consumed_bits(r, off)) & 7);
  if (rd_bits(r, pad) != 0u) return r.bad ? P2PHD_FLAC_E_BITS : P2PHD_FLAC_E_RESERVED;
  if (r.bad) return P2PHD_FLAC_E_BITS;
  if (rd_consumed_bits(r, off) + 16 != len * 8) return P2PHD_FLAC_E_LENGTH;
  return P2PHD_FLAC_OK;
}

// left / right of a decorrelated pair (a: channel 0, b: channel 1 as coded)
FHD void undo_stereo(int assign, int32_t a, int32_t b, int32_t& left, int32_t& right) {
  if (assign == 8) { left = a; right = a - b; }                 // left / side
  else if (assign == 9) { left = a + b; right = b; }            // side / right
  else { const int32_t mid = (int32_t)((uint32_t)a << 1) | (b & 1); left = (mid + b) >> 1; right = (mid - b) >> 1; }   // mid / side
}

FHD bool row_ok(int64_t off, int64_t len, int64_t nbytes, int64_t col, int64_t bs, int64_t ld, int64_t bits) {
  return off >= 0 && len >= 0 && off <= nbytes && len <= nbytes - off && bs >= 1 && bs <= 65535 && col >= 0 && col <= ld && bs <= ld - col &&
         bits >= 4 && bits <= 24;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
struct HostPolicy {
  int32_t cf[kHist], hs[kHist];
  int32_t* out; int64_t ld, col;
  void coef_set(int i, int v) { cf[i] = v; }
  int coef(int i) const { return cf[i]; }
  void hist_set(int n, int v) { hs[n & (kHist - 1)] = v; }
  int hist(int n) const { return hs[n & (kHist - 1)]; }
  void store(int c, int n, int32_t v) { out[(int64_t)c * ld + col + n] = v; }
};

// decodes and keeps nothing: whether [off, off + len) is one whole frame (p2phd_flac_index)
struct ProbePolicy {
  int32_t cf[kHist], hs[kHist];
  void coef_set(int i, int v) { cf[i] = v; }
  int coef(int i) const { return cf[i]; }
  void hist_set(int n, int v) { hs[n & (kHist - 1)] = v; }
  int hist(int n) const { return hs[n & (kHist - 1)]; }
  void store(int, int, int32_t) {}
};

struct Crc {
  uint8_t t8[256]; uint16_t t16[256];
  Crc() {
    for (int i = 0; i < 256; ++i) {
      uint8_t a = (uint8_t)i; uint16_t b = (uint16_t)(i << 8);
      for (int k = 0; k < 8; ++k) { a = (uint8_t)((a & 0x80) ? (a << 1) ^ 0x07 : a << 1); b = (uint16_t)((b & 0x8000) ? (b << 1) ^ 0x8005 : b << 1); }
      t8[i] = a; t16[i] = b;
    }
  }
};
const Crc& crc() { static const Crc c; return c; }

struct Hdr { int len, bs, rate, channels, assign, bits, variable; int64_t number; };

// The frame header at `pos` -> nullptr, or why it is none
const char* parse_header(const uint8_t* b, int64_t nbytes, int64_t pos, const p2phd_flac_streaminfo& si, Hdr* h) {
  if (nbytes - pos < 6) return "the file ends inside a frame header";
  const uint8_t* p = b + pos;
  if (p[0] != 0xFF || (p[1] & 0xFC) != 0xF8) return "no frame sync code";
  if (p[1] & 2) return "reserved bit set behind the sync code";
  h->variable = p[1] & 1;
  const int bscode = p[2] >> 4, srcode = p[2] & 15, assign = p[3] >> 4, szcode = (p[3] >> 1) & 7;
  if (bscode == 0) return "reserved block-size code 0";
  if (srcode == 15) return "reserved sample-rate code 15";
  if (assign > 10) return "reserved channel assignment";
  if (szcode == 3) return "reserved sample-size code 3";
  if (szcode == 7) return "32-bit samples are not built";
  if (p[3] & 1) return "reserved bit set behind the sample size";
  int at = 4;
  const int lead = p[at];
  const int ones = lead == 0xFF ? 8 : __builtin_clz(~((uint32_t)lead << 24));
  if (ones == 1 || ones == 8 || (ones == 7 && !h->variable)) return "bad coded frame / sample number";
  const int extra = ones ? ones - 1 : 0;
  if (nbytes - pos < 5 + extra) return "the file ends inside a frame header";
  int64_t number = ones ? (lead & (0x7F >> ones)) : lead;
  ++at;
  for (int i = 0; i < extra; ++i, ++at) {
    if ((p[at] & 0xC0) != 0x80) return "bad coded frame / sample number";
    number = (number << 6) | (p[at] & 0x3F);
  }
  h->number = number;
  const int need = at + (bscode == 6 ? 1 : bscode == 7 ? 2 : 0) + (srcode == 12 ? 1 : srcode >= 13 ? 2 : 0) + 1;
  if (nbytes - pos < need) return "the file ends inside a frame header";
  if (bscode == 1) h->bs = 192;
  else if (bscode <= 5) h->bs = 576 << (bscode - 2);
  else if (bscode == 6) { h->bs = p[at] + 1; at += 1; }
  else if (bscode == 7) { h->bs = ((p[at] << 8) | p[at + 1]) + 1; at += 2; }
  else h->bs = 256 << (bscode - 8);
  static const int rates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  if (srcode == 0) h->rate = si.sample_rate;
  else if (srcode < 12) h->rate = rates[srcode];
  else if (srcode == 12) { h->rate = p[at] * 1000; at += 1; }
  else { h->rate = ((p[at] << 8) | p[at + 1]) * (srcode == 14 ? 10 : 1); at += 2; }
  if (h->bs > 65535) return "a block of 65536 samples is not allowed";
  static const int sizes[8] = {0, 8, 12, 0, 16, 20, 24, 0};
  h->bits = szcode == 0 ? si.bits : sizes[szcode];
  h->assign = assign;
  h->channels = assign < 8 ? assign + 1 : 2;
  uint8_t c = 0;
  for (int i = 0; i < at; ++i) c = crc().t8[c ^ p[i]];
  if (c != p[at]) return "header CRC-8 mismatch";
  h->len = at + 1;
  return nullptr;
}

int stream_info(const char* what, const uint8_t* b, int64_t nbytes, p2phd_flac_streaminfo* si) {
  P2PHD_REQUIRE(b != nullptr && nbytes >= 0 && si != nullptr, "%s: null pointer or negative length", what);
  memset(si, 0, sizeof(*si));
  int64_t pos = 0;
  if (nbytes >= 10 && !memcmp(b, "ID3", 3)) {                   // ID3v2: 10 bytes, a sync-safe size, an optional footer of 10
    P2PHD_REQUIRE(!((b[6] | b[7] | b[8] | b[9]) & 0x80), "%s: ID3v2 tag with a size that is not sync-safe", what);
    pos = 10 + (((int64_t)b[6] << 21) | (b[7] << 14) | (b[8] << 7) | b[9]) + ((b[5] & 0x10) ? 10 : 0);
    P2PHD_REQUIRE(pos <= nbytes, "%s: the ID3v2 tag is longer than the file", what);
  }
  P2PHD_REQUIRE(!(nbytes - pos >= 4 && !memcmp(b + pos, "OggS", 4)), "%s: Ogg FLAC is not built (native FLAC streams only)", what);
  P2PHD_REQUIRE(nbytes - pos >= 4 && !memcmp(b + pos, "fLaC", 4), "%s: not a FLAC stream (no fLaC marker at byte %lld)", what, (long long)pos);
  pos += 4;
  bool have = false;
  for (int block = 0;; ++block) {
    P2PHD_REQUIRE(nbytes - pos >= 4, "%s: the file ends inside the metadata (block %d at byte %lld)", what, block, (long long)pos);
    const int last = b[pos] >> 7, type = b[pos] & 0x7F;
    const int64_t len = ((int64_t)b[pos + 1] << 16) | (b[pos + 2] << 8) | b[pos + 3];
    pos += 4;
    P2PHD_REQUIRE(type != 127, "%s: reserved metadata block type 127 (block %d)", what, block);
    P2PHD_REQUIRE(nbytes - pos >= len, "%s: the file ends inside the metadata (block %d of %lld bytes at byte %lld)", what, block, (long long)len, (long long)pos);
    P2PHD_REQUIRE((block == 0) == (type == 0), "%s: STREAMINFO must be the first metadata block and the only one of its type (block %d has type %d)", what, block, type);
    if (type == 0) {
      P2PHD_REQUIRE(len == 34, "%s: STREAMINFO of %lld bytes, not 34", what, (long long)len);
      const uint8_t* p = b + pos;
      si->min_block = (p[0] << 8) | p[1];
      si->max_block = (p[2] << 8) | p[3];
      si->sample_rate = (p[10] << 12) | (p[11] << 4) | (p[12] >> 4);
      si->channels = ((p[12] >> 1) & 7) + 1;
      si->bits = (((p[12] & 1) << 4) | (p[13] >> 4)) + 1;
      si->total_samples = ((int64_t)(p[13] & 15) << 32) | ((int64_t)p[14] << 24) | ((int64_t)p[15] << 16) | (p[16] << 8) | p[17];
      memcpy(si->md5, p + 18, 16);
      have = true;
    } else if (type == 3) {
      P2PHD_REQUIRE(len % 18 == 0, "%s: SEEKTABLE of %lld bytes, not a multiple of 18", what, (long long)len);
      si->seek_points = (int32_t)(len / 18);
    }
    pos += len;
    if (last) break;
  }
  P2PHD_REQUIRE(have, "%s: no STREAMINFO block", what);
  si->first_frame_offset = pos;
  P2PHD_REQUIRE(si->bits != 32, "%s: 32-bit samples are not built", what);
  P2PHD_REQUIRE(si->bits == 8 || si->bits == 12 || si->bits == 16 || si->bits == 20 || si->bits == 24,
                "%s: %d bits per sample (built: 8, 12, 16, 20, 24)", what, si->bits);
  P2PHD_REQUIRE(si->sample_rate > 0, "%s: STREAMINFO states a sample rate of 0", what);
  P2PHD_REQUIRE(si->min_block >= 16 && si->max_block >= si->min_block, "%s: STREAMINFO states block sizes %d .. %d", what, si->min_block, si->max_block);
  return P2PHD_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
struct DevicePolicy {
  int32_t* cf; int32_t* hs;                                     // the lane's columns of the two LDS tables [32][kLanes]
  int32_t* ws; int64_t ld, col;
  __device__ __forceinline__ void coef_set(int i, int v) { cf[i * kLanes] = v; }
  __device__ __forceinline__ int coef(int i) const { return cf[i * kLanes]; }
  __device__ __forceinline__ void hist_set(int n, int v) { hs[(n & (kHist - 1)) * kLanes] = v; }
  __device__ __forceinline__ int hist(int n) const { return hs[(n & (kHist - 1)) * kLanes]; }
  __device__ __forceinline__ void store(int c, int n, int32_t v) { ws[(int64_t)c * ld + col + n] = v; }
};

__global__ __launch_bounds__(kLanes) void flac_frames_kernel(const uint8_t* __restrict__ bytes, long nbytes, const long long* __restrict__ table,
                                                             int nframes, int channels, long ld, int32_t* __restrict__ ws,
                                                             unsigned long long* __restrict__ status) {
  __shared__ int32_t s_cf[kHist * kLanes], s_hs[kHist * kLanes];
  const int f = blockIdx.x * kLanes + threadIdx.x;
  if (f >= nframes) return;
  const long long* row = table + (size_t)f * kRow;
  const long off = row[0], len = row[1], col = row[2] - table[2], bs = row[3], assign = row[4], bits = row[5];
  int rc = P2PHD_FLAC_E_ROW;
  if (row_ok(off, len, nbytes, col, bs, ld, bits)) {
    DevicePolicy pol{s_cf + threadIdx.x, s_hs + threadIdx.x, ws, ld, col};
    rc = decode_frame(pol, bytes, off, len, (int)bs, (int)assign, (int)bits, channels);
    if (rc)                                                     // a bad frame is silence in every channel
      for (int c = 0; c < channels; ++c)
        for (int n = 0; n < (int)bs; ++n) pol.store(c, n, 0);
  }
  if (rc) atomicMin(status, ((unsigned long long)f << 8) | (unsigned long long)rc);
}

// workgroup b: the samples of frames b, b + gridDim.x, ..., every channel; ws holds the subframes' integers as coded
__global__ __launch_bounds__(kTile) void flac_pcm_kernel(const long long* __restrict__ table, long nframes, long nbytes, int channels, int bits, long ld,
                                                         const int32_t* __restrict__ ws, float* __restrict__ out) {
  const float scale = __uint_as_float((uint32_t)(127 - (bits - 1)) << 23);
  for (long f = blockIdx.x; f < nframes; f += gridDim.x) {
  const long long* row = table + (size_t)f * kRow;
  const long off = row[0], len = row[1], col = row[2] - table[2], bs = row[3], assign = row[4];
  if (!row_ok(off, len, nbytes, col, bs, ld, row[5])) continue;   // (reported by flac_frames_kernel; nothing of such a row is written)
  for (long n = threadIdx.x; n < bs; n += kTile) {
    const long at = col + n;
    if (assign >= 8 && assign <= 10 && channels == 2) {
      int32_t l, r;
      undo_stereo((int)assign, ws[at], ws[ld + at], l, r);
      out[at] = (float)l * scale;
      out[ld + at] = (float)r * scale;
    } else {
      for (int c = 0; c < channels; ++c) out[(long)c * ld + at] = (float)ws[(long)c * ld + at] * scale;
    }
  }
  }
}
#endif

bool bits_ok(int bits) { return bits == 8 || bits == 12 || bits == 16 || bits == 20 || bits == 24; }

}  // namespace

extern "C" int p2phd_flac_info(const void* bytes, int64_t nbytes, p2phd_flac_streaminfo* info) {
  return stream_info("flac_info", static_cast<const uint8_t*>(bytes), nbytes, info);
}

extern "C" int64_t p2phd_flac_index(const void* bytes, int64_t nbytes, int64_t* table, int64_t cap) {
  const char* what = "flac_index";
  const uint8_t* b = static_cast<const uint8_t*>(bytes);
  p2phd_flac_streaminfo si;
  if (stream_info(what, b, nbytes, &si)) return -1;
  if (cap < 0 || (cap > 0 && table == nullptr)) { p2phd::set_error("%s: cap %lld with a null table", what, (long long)cap); return -1; }
  int64_t pos = si.first_frame_offset, k = 0, expect = 0, counted = 0;
  int variable = 0, bs0 = 0, prev_bs = 0;
  Hdr h, nh;
  while (pos < nbytes) {
    if (const char* why = parse_header(b, nbytes, pos, si, &h)) {
      p2phd::set_error("%s: frame %lld at byte %lld: %s", what, (long long)k, (long long)pos, why);
      return -1;
    }
    const char* why = nullptr;
    if (h.rate != si.sample_rate) why = "the sample rate changes mid-stream";
    else if (h.channels != si.channels) why = "the channel count changes mid-stream";
    else if (h.bits != si.bits) why = "the sample size changes mid-stream";
    else if (k > 0 && h.variable != variable) why = "the blocking strategy changes mid-stream";
    else if (k > 0 && h.number != expect) why = "gap in the sample numbers (the frame or sample number is not the one that follows)";
    else if (k > 0 && !variable && prev_bs != bs0) why = "a fixed-block-size stream with a shorter frame in front of the last";
    if (why) {
      p2phd::set_error("%s: frame %lld at byte %lld: %s", what, (long long)k, (long long)pos, why);
      return -1;
    }
    if (k == 0) { variable = h.variable; bs0 = h.bs; }
    expect = variable ? h.number + h.bs : h.number + 1;
    prev_bs = h.bs;
    // the end: the first q where the CRC-16 of [pos, q) closes (it is then 0) and the next header stands, or the file ends.  Where
    // it closes in front of something at most one bit from a sync code that is no standing header, either the next frame's header
    // is at fault or the frame's own bytes happen to look so (once in 2^27 bytes of audio): the subframes decide -- [pos, q) is the
    // frame exactly when they decode to its last bit.  Then the scan stops and the next round says what is wrong with the header
    // behind it (it must stop: a CRC that closed stays closed at the end of every whole frame that follows); else it goes on.
    int64_t end = -1;
    uint16_t c = 0;
    for (int64_t q = pos; q <= nbytes; ++q) {
      if (c == 0 && q - pos >= h.len + 3) {
        if (q == nbytes) { end = q; break; }
        if (!parse_header(b, nbytes, q, si, &nh) && nh.variable == variable && nh.number == expect && nh.rate == si.sample_rate &&
            nh.channels == si.channels && nh.bits == si.bits) { end = q; break; }
        if (q + 1 < nbytes && __builtin_popcount((((unsigned)b[q] << 8 | b[q + 1]) ^ 0xFFF8u) & 0xFFFEu) <= 1) {
          ProbePolicy probe;
          if (decode_frame(probe, b, pos, q - pos, h.bs, h.assign, h.bits, h.channels) == P2PHD_FLAC_OK) { end = q; break; }
        }
      }
      if (q < nbytes) c = (uint16_t)((c << 8) ^ crc().t16[(c >> 8) ^ b[q]]);
    }
    if (end < 0) {
      p2phd::set_error("%s: frame %lld at byte %lld: no end with a good CRC-16 (a corrupt or truncated frame)", what, (long long)k, (long long)pos);
      return -1;
    }
    if (k < cap) {
      int64_t* row = table + k * kRow;
      row[0] = pos; row[1] = end - pos; row[2] = variable ? h.number : h.number * (int64_t)bs0; row[3] = h.bs; row[4] = h.assign; row[5] = h.bits;
    }
    counted += h.bs;
    pos = end;
    ++k;
  }
  if (si.total_samples != 0 && counted != si.total_samples) {
    p2phd::set_error("%s: the %lld frames hold %lld samples, STREAMINFO states %lld (a truncated file)", what, (long long)k, (long long)counted,
                     (long long)si.total_samples);
    return -1;
  }
  return k;
}

extern "C" int p2phd_flac_decode_host(const void* bytes, int64_t nbytes, const int64_t* table, int64_t first_frame, int64_t frame_count,
                                      int channels, int32_t* out, int64_t ld) {
  const char* what = "flac_decode_host";
  P2PHD_REQUIRE(first_frame >= 0 && frame_count >= 0 && nbytes >= 0, "%s: negative frame range or length", what);
  P2PHD_REQUIRE(channels >= 1 && channels <= 8, "%s: need 1 <= channels <= 8 (channels %d)", what, channels);
  if (frame_count == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes && table && out, "%s: null pointer", what);
  const uint8_t* b = static_cast<const uint8_t*>(bytes);
  const int64_t base = table[first_frame * kRow + 2];
  static const char* reasons[] = {"", "the bit stream runs past the frame's end", "reserved code", "impossible partition or predictor order",
                                  "the subframes end short of the frame's length", "bad table row"};
  for (int64_t f = first_frame; f < first_frame + frame_count; ++f) {
    const int64_t* row = table + f * kRow;
    const int64_t off = row[0], len = row[1], col = row[2] - base, bs = row[3], assign = row[4], bits = row[5];
    P2PHD_REQUIRE(row_ok(off, len, nbytes, col, bs, ld, bits) && assign >= 0 && assign <= 10,
                  "%s: frame %lld: bad table row (offset %lld, length %lld of %lld bytes, column %lld + %lld of ld %lld, assignment %lld, %lld bit)", what,
                  (long long)f, (long long)off, (long long)len, (long long)nbytes, (long long)col, (long long)bs, (long long)ld, (long long)assign, (long long)bits);
    HostPolicy pol;
    pol.out = out; pol.ld = ld; pol.col = col;
    P2PHD_REQUIRE((assign < 8 ? (int)assign + 1 : 2) == channels, "%s: frame %lld: bad table row (assignment %lld is not one of %d channels)", what,
                  (long long)f, (long long)assign, channels);
    const int rc = decode_frame(pol, b, off, len, (int)bs, (int)assign, (int)bits, channels);
    P2PHD_REQUIRE(rc == P2PHD_FLAC_OK, "%s: frame %lld at byte %lld: %s", what, (long long)f, (long long)off, reasons[rc]);
    if (assign >= 8)
      for (int64_t n = col; n < col + bs; ++n) {
        int32_t l, r;
        undo_stereo((int)assign, out[n], out[ld + n], l, r);
        out[n] = l; out[ld + n] = r;
      }
  }
  return P2PHD_OK;
}

extern "C" size_t p2phd_flac_workspace_bytes(int channels, int64_t ld) {
  if (channels < 1 || channels > 8 || ld < 0 || ld > (int64_t(1) << 40) / 8) {
    p2phd::set_error("flac_workspace_bytes: need 1 <= channels <= 8 and 0 <= ld <= 2^37 (channels %d, ld %lld)", channels, (long long)ld);
    return 0;
  }
  return std::max<size_t>((size_t)channels * (size_t)ld * sizeof(int32_t), 4);
}

extern "C" int p2phd_flac_tile_len(void) { return kTile; }
extern "C" int p2phd_flac_frames_per_workgroup(void) { return kLanes; }

namespace {
constexpr int64_t kPcmGrid = 1 << 20;          // workgroups of flac_pcm_kernel at most: each walks frames b, b + grid, ...

// stage 0: both kernels; 1 / 2 (p2phd_flac_decode_stage): the frame / the element-wise kernel alone
int flac_decode(const char* what, int stage, const void* bytes_dev, int64_t nbytes, const int64_t* table_dev, int64_t nframes, int channels, int bits,
                float* out, int64_t ld, void* workspace, uint64_t* status_dev, void* stream) {
  P2PHD_REQUIRE(nframes >= 0 && nframes <= 0x7FFFFFFF, "%s: need 0 <= nframes < 2^31 (nframes %lld)", what, (long long)nframes);
  P2PHD_REQUIRE(channels >= 1 && channels <= 8, "%s: need 1 <= channels <= 8 (channels %d)", what, channels);
  P2PHD_REQUIRE(bits_ok(bits), "%s: %d bits per sample (built: 8, 12, 16, 20, 24)", what, bits);
  P2PHD_REQUIRE(nbytes >= 0 && ld >= 0 && ld <= (int64_t(1) << 40) / channels, "%s: need nbytes >= 0 and 0 <= ld * channels <= 2^40 (nbytes %lld, ld %lld)", what,
                (long long)nbytes, (long long)ld);
  if (nframes == 0) return P2PHD_OK;
  P2PHD_REQUIRE(bytes_dev && table_dev && out && workspace && status_dev, "%s: null pointer", what);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out is not aligned to a float", what);
  P2PHD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(table_dev) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(status_dev) & 7) == 0, "%s: workspace, table or status is not aligned to its type", what);
  hipStream_t st = (hipStream_t)stream;
  const long long* table = reinterpret_cast<const long long*>(table_dev);
  int32_t* ws = static_cast<int32_t*>(workspace);
  if (stage != 2)
    hipLaunchKernelGGL(flac_frames_kernel, dim3((unsigned)p2phd::cdiv(nframes, kLanes)), dim3(kLanes), 0, st, static_cast<const uint8_t*>(bytes_dev),
                       (long)nbytes, table, (int)nframes, channels, (long)ld, ws, reinterpret_cast<unsigned long long*>(status_dev));
  if (stage != 1)
    hipLaunchKernelGGL(flac_pcm_kernel, dim3((unsigned)std::min<int64_t>(nframes, kPcmGrid)), dim3(kTile), 0, st, table, (long)nframes, (long)nbytes, channels,
                       bits, (long)ld, ws, out);
  p2phd::g_launch_count[p2phd::LC_FLAC] += stage ? 1 : 2;
  return p2phd::check_launch(what);
}
}  // namespace

extern "C" int p2phd_flac_decode(const void* bytes_dev, int64_t nbytes, const int64_t* table_dev, int64_t nframes, int channels, int bits,
                                 float* out, int64_t ld, void* workspace, uint64_t* status_dev, void* stream) {
  return flac_decode("flac_decode", 0, bytes_dev, nbytes, table_dev, nframes, channels, bits, out, ld, workspace, status_dev, stream);
}

extern "C" int p2phd_flac_decode_stage(int stage, const void* bytes_dev, int64_t nbytes, const int64_t* table_dev, int64_t nframes, int channels, int bits,
                                       float* out, int64_t ld, void* workspace, uint64_t* status_dev, void* stream) {
  P2PHD_REQUIRE(stage == 1 || stage == 2, "flac_decode_stage: stage must be 1 (the frame kernel alone) or 2 (the element-wise kernel alone), got %d", stage);
  return flac_decode("flac_decode_stage", stage, bytes_dev, nbytes, table_dev, nframes, channels, bits, out, ld, workspace, status_dev, stream);
}
