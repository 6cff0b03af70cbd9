// Stand-alone driver of the HOST entries of the FLAC encoder's LPC option (csrc/flacenc.hip) for a sanitizer build (never a test, never
// run on a GPU machine, never through Python):
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Ipix2pixhdaudiosr_amd/csrc \
//         tools/flac_lpc_host_check.hip pix2pixhdaudiosr_amd/csrc/flacenc.hip pix2pixhdaudiosr_amd/csrc/flac.hip -o flac_lpc_host_check \
//         && ./flac_lpc_host_check
//
// p2phd_flac_lpc_fit on sequences R of every kind (positive definite, indefinite, zeros, the largest magnitudes) and
// p2phd_flac_lpc_analyse on blocks of 1 .. 16384 samples at 16, 17, 24 and 25 bits, into heap buffers of exactly the stated sizes (one
// element past either end is the sanitizer's).  Then, over channels 1, 2, 3, 8, both sample sizes, blocks 16 .. 16384, lengths around the
// block and M in {0, 1, 4, 12}, with a resonance, a tone, DC, full-scale noise, alternating full scale and a quiet resonance in the
// channels, and for random payloads of random geometry: p2phd_flac_encode_plan, p2phd_flac_encode_lpc_host into buffers of exactly the
// planned sizes, "fLaC" and STREAMINFO in front, then p2phd_flac_info, p2phd_flac_index and p2phd_flac_decode_host on the result, whose
// samples must be the payload's; no frame may be longer than the same frame at a smaller M, and M = 0 must give p2phd_flac_encode_host's
// bytes.  It links none of the device entries' callers: the few symbols of core.hip that the two files name are defined here.
#include "common.h"
#include "convplan.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace p2phd {
static char g_text[1024];
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_text, sizeof(g_text), fmt, ap); va_end(ap); }
void fold_launched() {}
thread_local int g_fold_pending = -1;
unsigned long long g_launch_count[LC_FAMILIES];
}  // namespace p2phd

namespace {
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }
long g_cases = 0, g_lpc_frames = 0;
int64_t g_bytes = 0, g_pcm = 0;

// kind 0 resonance (two pole pairs driven by noise), 1 tone with noise, 2 DC, 3 full-scale noise, 4 alternating full scale, 5 quiet resonance
struct Source {
  double s[4] = {0, 0, 0, 0};
  int32_t next(int kind, int bits, int64_t n, int c) {
    const int32_t top = (1 << (bits - 1)) - 1;
    if (kind == 0 || kind == 5) {
      const double e = ((double)(rnd() % 2001) - 1000.0) / 1000.0;
      const double a = e + 2 * 0.97 * cos(0.2 + 0.1 * c) * s[0] - 0.97 * 0.97 * s[1];
      s[1] = s[0]; s[0] = a;
      const double b = a + 2 * 0.97 * cos(0.9) * s[2] - 0.97 * 0.97 * s[3];
      s[3] = s[2]; s[2] = b;
      double v = b * (kind == 0 ? 0.002 : 0.00002) * top;
      if (v > top) v = top;
      if (v < -top - 1) v = -top - 1;
      return (int32_t)lrint(v);
    }
    switch (kind) {
      case 1: return (int32_t)lrint(0.3 * top * sin(2 * M_PI * 997 * n / 48000.0 + c)) + (int32_t)(rnd() % 3) - 1;
      case 2: return 3 - 5 * c;
      case 3: return (int32_t)(rnd() % (2u * top + 2u)) - top - 1;
      default: return (n + c) % 2 ? top : -top - 1;
    }
  }
};

int check_fit_and_analyse() {
  for (int k = 0; k < 4000; ++k) {
    const int orders = (int)(rnd() % 13);
    std::vector<int64_t> R((size_t)orders + 1);
    std::vector<int32_t> ok(12), q(144), shift(12);
    const int kind = k % 4;
    for (int l = 0; l <= orders; ++l) {
      const int64_t big = (int64_t)(((uint64_t)rnd() << 21) ^ rnd()) % ((int64_t(1) << 53) - 1);
      R[l] = kind == 0 ? big * (rnd() % 2 ? 1 : -1) : kind == 1 ? (l == 0 ? (int64_t(1) << 46) : (int64_t)(rnd() % 2000) - 1000) : kind == 2 ? 0 : (int64_t)(rnd() % 7) - 3;
    }
    if (kind == 0 && R[0] < 0) R[0] = -R[0];
    if (p2phd_flac_lpc_fit(R.data(), orders, ok.data(), q.data(), shift.data())) { fprintf(stderr, "fit: %s\n", p2phd::g_text); return 1; }
    for (int o = 0; o < 12; ++o) {
      if (o >= orders && ok[o]) { fprintf(stderr, "fit admits order %d of %d\n", o + 1, orders); return 1; }
      for (int j = 0; j < 12; ++j) if (q[o * 12 + j] < -4096 || q[o * 12 + j] > 4095) { fprintf(stderr, "fit: coefficient outside 13 bits\n"); return 1; }
      if (shift[o] < 0 || shift[o] > 15) { fprintf(stderr, "fit: shift outside 0 .. 15\n"); return 1; }
    }
  }
  const int sizes[12] = {1, 2, 3, 12, 13, 16, 17, 192, 1152, 4096, 4608, 16384};
  for (int bs : sizes)
    for (int bps : {16, 17, 24, 25})
      for (int kind = 0; kind < 6; ++kind)
        for (int M : {1, 7, 12}) {
          Source src;
          std::vector<int32_t> x((size_t)bs), ok(12), q(144), shift(12);
          std::vector<int64_t> R(13);
          for (int n = 0; n < bs; ++n) x[n] = src.next(kind, bps, n, 0);
          if (p2phd_flac_lpc_analyse(x.data(), bs, bps, M, ok.data(), q.data(), shift.data(), R.data())) { fprintf(stderr, "analyse: %s\n", p2phd::g_text); return 1; }
          for (int o = 0; o < 12; ++o) if (ok[o] && o + 1 > (M < bs - 1 ? M : bs - 1)) { fprintf(stderr, "analyse admits order %d (bs %d, M %d)\n", o + 1, bs, M); return 1; }
          for (int l = 0; l < 13; ++l) if (R[l] >= (int64_t(1) << 46) || R[l] <= -(int64_t(1) << 46)) { fprintf(stderr, "analyse: R outside 2^46\n"); return 1; }
        }
  return 0;
}

int run(int C, int bits, int64_t L, int rate, int block, int kind0) {
  const int nb = bits / 8;
  std::vector<int32_t> want((size_t)C * L);
  std::vector<uint8_t> pay((size_t)C * L * nb);
  std::vector<Source> src((size_t)C);
  for (int64_t n = 0; n < L; ++n)
    for (int c = 0; c < C; ++c) {
      const int32_t v = src[c].next(kind0 < 0 ? (c - kind0) % 6 : kind0, bits, n, c);
      want[(size_t)c * L + n] = v;
      for (int b = 0; b < nb; ++b) pay[((size_t)n * C + c) * nb + b] = (uint8_t)((uint32_t)v >> (8 * b));
    }
  int64_t nframes, worst, work;
  if (p2phd_flac_encode_plan(C, bits, L, block, &nframes, &worst, &work)) { fprintf(stderr, "plan: %s\n", p2phd::g_text); return 1; }
  std::vector<uint8_t> base((size_t)worst);
  std::vector<int64_t> base_lengths((size_t)nframes + 1), before;
  if (p2phd_flac_encode_host(pay.data(), C, bits, L, rate, block, base.data(), worst, base_lengths.data())) { fprintf(stderr, "encode: %s\n", p2phd::g_text); return 1; }
  for (int M : {0, 1, 4, 12}) {
    std::vector<uint8_t> frames((size_t)worst);
    std::vector<int64_t> lengths((size_t)nframes + 1);
    if (p2phd_flac_encode_lpc_host(pay.data(), C, bits, L, rate, block, M, frames.data(), worst, lengths.data())) { fprintf(stderr, "encode_lpc: %s\n", p2phd::g_text); return 1; }
    int64_t lo = lengths[0], hi = lengths[0], sum = 0;
    for (int64_t f = 0; f < nframes; ++f) { lo = lengths[f] < lo ? lengths[f] : lo; hi = lengths[f] > hi ? lengths[f] : hi; sum += lengths[f]; }
    if (sum != lengths[nframes] || sum > worst) { fprintf(stderr, "lengths do not add up\n"); return 1; }
    if (M == 0 && (lengths != base_lengths || memcmp(frames.data(), base.data(), (size_t)sum))) { fprintf(stderr, "M = 0 is not the existing entry\n"); return 1; }
    if (M > 0)
      for (int64_t f = 0; f < nframes; ++f) {
        if (lengths[f] > before[f]) { fprintf(stderr, "frame %lld grows with M = %d\n", (long long)f, M); return 1; }
        if (M == 12 && lengths[f] < base_lengths[f]) ++g_lpc_frames;
      }
    before = lengths;
    std::vector<uint8_t> file(42 + (size_t)sum);                            // exact size
    memcpy(file.data(), "fLaC\x80\0\0\x22", 8);
    uint8_t* p = file.data() + 8;
    p[0] = p[2] = (uint8_t)(block >> 8); p[1] = p[3] = (uint8_t)block;
    p[4] = (uint8_t)(lo >> 16); p[5] = (uint8_t)(lo >> 8); p[6] = (uint8_t)lo;
    p[7] = (uint8_t)(hi >> 16); p[8] = (uint8_t)(hi >> 8); p[9] = (uint8_t)hi;
    const uint64_t v = ((uint64_t)rate << 44) | ((uint64_t)(C - 1) << 41) | ((uint64_t)(bits - 1) << 36) | (uint64_t)L;
    for (int i = 0; i < 8; ++i) p[10 + i] = (uint8_t)(v >> (56 - 8 * i));
    memset(p + 18, 0, 16);
    memcpy(file.data() + 42, frames.data(), (size_t)sum);
    p2phd_flac_streaminfo si;
    if (p2phd_flac_info(file.data(), (int64_t)file.size(), &si)) { fprintf(stderr, "info: %s\n", p2phd::g_text); return 1; }
    std::vector<int64_t> table((size_t)nframes * P2PHD_FLAC_ROW_WORDS);
    if (p2phd_flac_index(file.data(), (int64_t)file.size(), table.data(), nframes) != nframes) { fprintf(stderr, "index: %s\n", p2phd::g_text); return 1; }
    std::vector<int32_t> got((size_t)C * L);
    if (p2phd_flac_decode_host(file.data(), (int64_t)file.size(), table.data(), 0, nframes, C, got.data(), L)) { fprintf(stderr, "decode: %s\n", p2phd::g_text); return 1; }
    if (got != want) { fprintf(stderr, "the decoded samples are not the payload's (M %d)\n", M); return 1; }
    ++g_cases; g_bytes += sum; g_pcm += (int64_t)pay.size();
  }
  return 0;
}
}  // namespace

int main() {
  if (check_fit_and_analyse()) return 1;
  const int blocks[9] = {16, 17, 192, 255, 256, 1000, 4096, 4608, 16384}, chans[4] = {1, 2, 3, 8};
  int i = 0;
  for (int C : chans)
    for (int bits : {16, 24})
      for (int block : blocks) {
        const int64_t Ls[5] = {1, 5, block - 1, block + 1, (block > 4096 && C > 2 ? 1 : 2) * (int64_t)block + 13};
        for (int64_t L : Ls) {
          ++i;
          if (run(C, bits, L, i % 2 ? 48000 : 12345, block, -(i % 6))) { fprintf(stderr, "matrix case C %d bits %d block %d L %lld\n", C, bits, block, (long long)L); return 1; }
        }
      }
  // refusals leave the buffers alone
  {
    std::vector<uint8_t> pay(80), out(4096);
    std::vector<int64_t> lengths(4);
    if (!p2phd_flac_encode_lpc_host(pay.data(), 1, 16, 40, 48000, 16, 13, out.data(), 4096, lengths.data()) ||
        !p2phd_flac_encode_lpc_host(pay.data(), 1, 16, 40, 48000, 16385, 1, out.data(), 4096, lengths.data()) ||
        !p2phd_flac_encode_lpc_host(pay.data(), 1, 16, 40, 48000, 16, -1, out.data(), 4096, lengths.data())) { fprintf(stderr, "a refusal is missing\n"); return 1; }
  }
  for (int k = 0; k < 200; ++k) {
    const int C = 1 + (int)(rnd() % 8), bits = rnd() % 2 ? 16 : 24, block = 16 + (int)(rnd() % 3000);
    const int64_t L = 1 + (int64_t)(rnd() % (unsigned)(4 * block));
    if (run(C, bits, L, 1 + (int)(rnd() % 1048575u), block, (int)(rnd() % 5) == 4 ? 3 : -(int)(rnd() % 6))) {
      fprintf(stderr, "random case %d: C %d bits %d block %d L %lld\n", k, C, bits, block, (long long)L);
      return 1;
    }
  }
  printf("%ld streams encoded, indexed and decoded to their payload: %lld bytes of FLAC for %lld of PCM; %ld frames shorter at M = 12 than at M = 0\n", g_cases,
         (long long)g_bytes, (long long)g_pcm, g_lpc_frames);
  return g_lpc_frames > 0 ? 0 : 1;
}
