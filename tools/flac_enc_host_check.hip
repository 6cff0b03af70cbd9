// Stand-alone driver of the HOST encoder of csrc/flacenc.hip for a sanitizer build (never a test, never run on a GPU machine):
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Ipix2pixhdaudiosr_amd/csrc \
//         tools/flac_enc_host_check.hip pix2pixhdaudiosr_amd/csrc/flacenc.hip pix2pixhdaudiosr_amd/csrc/flac.hip -o flac_enc_host_check \
//         && ./flac_enc_host_check
//
// For every case of the host test matrix (channels 1, 2, 3, 8; 16 and 24 bits; the eight block sizes; the eight lengths; each at all
// five rates: 2560 streams) with a tone, DC, full-scale noise and a quiet tone in its channels, for the decision cases (silence, alternating
// full scale, a quiet block with one full-scale sample at block 65535, equal stereo channels) and for random payloads of random
// geometry: p2phd_flac_encode_plan, p2phd_flac_encode_host into heap buffers of exactly the planned sizes (one byte past either end
// is the sanitizer's), "fLaC" and STREAMINFO in front, then p2phd_flac_info, p2phd_flac_index and p2phd_flac_decode_host on the
// result, whose samples must be the payload's.  It links none of the device entries' callers: the few symbols of core.hip that the
// two files name are defined here.
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
long g_cases = 0;
int64_t g_bytes = 0, g_pcm = 0;

// kind 0 tone with noise, 1 DC, 2 full-scale noise, 3 quiet tone, 4 alternating full scale, 5 silence with one full-scale sample
int32_t sample(int kind, int bits, int64_t n, int c) {
  const int32_t top = (1 << (bits - 1)) - 1;
  switch (kind) {
    case 0: return (int32_t)lrint(0.3 * top * sin(2 * M_PI * 997 * n / 48000.0 + c)) + (int32_t)(rnd() % 3) - 1;
    case 1: return 3 - 5 * c;
    case 2: return (int32_t)(rnd() % (2u * top + 2u)) - top - 1;
    case 3: return (int32_t)lrint(0.01 * top * sin(2 * M_PI * 997 * n / 48000.0 + c)) + (int32_t)(rnd() % 7) - 3;
    case 4: return (n + c) % 2 ? top : -top - 1;
    default: return n == 30000 ? top : (int32_t)(rnd() % 3) - 1;
  }
}

int run(int C, int bits, int64_t L, int rate, int block, int kind0, bool same_channels = false) {
  const int nb = bits / 8;
  std::vector<int32_t> want((size_t)C * L);
  std::vector<uint8_t> pay((size_t)C * L * nb);
  for (int64_t n = 0; n < L; ++n)
    for (int c = 0; c < C; ++c) {
      const int32_t v = same_channels && c ? want[(size_t)n] : sample(kind0 < 0 ? (c - kind0) % 4 : kind0, bits, n, c);
      want[(size_t)c * L + n] = v;
      for (int b = 0; b < nb; ++b) pay[((size_t)n * C + c) * nb + b] = (uint8_t)((uint32_t)v >> (8 * b));
    }
  int64_t nframes, worst, work;
  if (p2phd_flac_encode_plan(C, bits, L, block, &nframes, &worst, &work)) { fprintf(stderr, "plan: %s\n", p2phd::g_text); return 1; }
  std::vector<uint8_t> frames((size_t)worst);
  std::vector<int64_t> lengths((size_t)nframes + 1);
  if (p2phd_flac_encode_host(pay.data(), C, bits, L, rate, block, frames.data(), worst, lengths.data())) { fprintf(stderr, "encode: %s\n", p2phd::g_text); return 1; }
  int64_t lo = lengths[0], hi = lengths[0], sum = 0;
  for (int64_t f = 0; f < nframes; ++f) { lo = lengths[f] < lo ? lengths[f] : lo; hi = lengths[f] > hi ? lengths[f] : hi; sum += lengths[f]; }
  if (sum != lengths[nframes] || sum > worst) { fprintf(stderr, "lengths do not add up\n"); return 1; }
  std::vector<uint8_t> file(42 + (size_t)sum);                              // exact size
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
  if (si.sample_rate != rate || si.channels != C || si.bits != bits || si.total_samples != L) { fprintf(stderr, "STREAMINFO differs\n"); return 1; }
  std::vector<int64_t> table((size_t)nframes * P2PHD_FLAC_ROW_WORDS);
  if (p2phd_flac_index(file.data(), (int64_t)file.size(), table.data(), nframes) != nframes) { fprintf(stderr, "index: %s\n", p2phd::g_text); return 1; }
  std::vector<int32_t> got((size_t)C * L);
  if (p2phd_flac_decode_host(file.data(), (int64_t)file.size(), table.data(), 0, nframes, C, got.data(), L)) { fprintf(stderr, "decode: %s\n", p2phd::g_text); return 1; }
  if (got != want) { fprintf(stderr, "the decoded samples are not the payload's\n"); return 1; }
  ++g_cases; g_bytes += sum; g_pcm += (int64_t)pay.size();
  return 0;
}
}  // namespace

int main() {
  const int rates[5] = {44100, 12345, 96000, 352800, 100001}, blocks[8] = {16, 64, 100, 192, 256, 576, 1000, 4096}, chans[4] = {1, 2, 3, 8};
  int i = 0;
  for (int C : chans)
    for (int bits : {16, 24})
      for (int block : blocks) {
        const int64_t Ls[8] = {1, 2, 4, 5, block - 1, block, block + 1, 3 * block + 5};
        for (int64_t L : Ls) {
          ++i;
          for (int rate : rates)
            if (run(C, bits, L, rate, block, -(i % 7))) { fprintf(stderr, "matrix case C %d bits %d block %d L %lld rate %d\n", C, bits, block, (long long)L, rate); return 1; }
        }
      }
  if (run(1, 16, 300, 48000, 256, 1) || run(3, 24, 100, 48000, 64, 1) || run(2, 24, 512, 96000, 512, 4) || run(1, 24, 512, 96000, 512, 4) ||
      run(1, 24, 65535, 48000, 65535, 5) || run(2, 16, 4096, 44100, 4096, 0, true) || run(1, 16, 70000, 1048575, 65535, 3)) {
    fprintf(stderr, "decision case\n");
    return 1;
  }
  for (int k = 0; k < 300; ++k) {
    const int C = 1 + (int)(rnd() % 8), bits = rnd() % 2 ? 16 : 24, block = 16 + (int)(rnd() % 3000);
    const int64_t L = 1 + (int64_t)(rnd() % (unsigned)(4 * block));
    if (run(C, bits, L, 1 + (int)(rnd() % 1048575u), block, (int)(rnd() % 5) == 4 ? 2 : -(int)(rnd() % 4))) {
      fprintf(stderr, "random case %d: C %d bits %d block %d L %lld\n", k, C, bits, block, (long long)L);
      return 1;
    }
  }
  printf("%ld streams encoded, indexed and decoded to their payload: %lld bytes of FLAC for %lld of PCM\n", g_cases, (long long)g_bytes, (long long)g_pcm);
  return 0;
}
