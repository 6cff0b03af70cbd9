// Stand-alone driver of the HOST part of csrc/wavcodec.hip for a sanitizer build (never a test, never run on a GPU machine):
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Ipix2pixhdaudiosr_amd/csrc \
//         tools/wavcodec_host_check.hip pix2pixhdaudiosr_amd/csrc/wavcodec.hip -o wavcodec_host_check && ./wavcodec_host_check [a.wav ...]
//
// Without arguments it builds its own fixtures (random byte streams in every layout of a small table, header indices 0 .. 255
// included); with arguments it takes the data chunk of every coded WAVE file named (tags 6, 7 and 0x11).  Every payload goes through
// p2phd_ima_frames, p2phd_ima_scan_host and p2phd_ima_decode_host (or p2phd_g711_decode_host) as it stands, in windows around every
// block boundary, at every truncation inside its first block and a few hundred lengths above, with single bits flipped in the headers
// and first groups of its first blocks, and with arguments bent past what the payload holds.  Every buffer is an exact-size heap copy: one byte past either end is the
// sanitizer's.  The library's answers are counted, not judged.  It links none of the device entries' callers: the few symbols of
// core.hip that wavcodec.hip names are defined here.
#include "common.h"
#include "convplan.h"
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
long g_ok = 0, g_refused = 0;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }

void count(int rc) { if (rc) ++g_refused; else ++g_ok; }

void window(const std::vector<uint8_t>& b, int C, int align, int64_t first, int64_t n) {
  if (n < 0) n = 0;
  std::vector<float> out((size_t)C * (size_t)n);                  // exact: ld = n
  count(p2phd_ima_decode_host(b.data(), (int64_t)b.size(), C, align, first, n, out.data(), n));
}

// every: windows around the first block boundaries too (the payload as it stands); else the whole, its ends and the refusals
void run_ima(const std::vector<uint8_t>& raw, int C, int align, bool every = false) {
  std::vector<uint8_t> b(raw.begin(), raw.end());
  const int64_t frames = p2phd_ima_frames((int64_t)b.size(), C, align);
  if (frames < 0) { ++g_refused; return; }
  p2phd_ima_scan_host(b.data(), (int64_t)b.size(), C, align);
  window(b, C, align, 0, frames);
  window(b, C, align, 0, frames + 1);                             // refused: beyond the payload
  window(b, C, align, frames, 1);
  if (frames > 3) window(b, C, align, frames - 3, 3);
  if (!every) return;
  const int64_t spb = 1 + 8 * (int64_t)(align / (4 * C) - 1);
  for (int64_t B = 0; B * spb <= frames && B < 6; ++B)
    for (int64_t d = -2; d <= 2; ++d)
      for (int64_t n : {(int64_t)0, (int64_t)1, spb - 1, spb, spb + 1}) {
        const int64_t first = B * spb + d;
        if (first >= 0 && first + n <= frames) window(b, C, align, first, n);
      }
}

void run_g711(const std::vector<uint8_t>& raw, int C) {
  std::vector<uint8_t> b(raw.begin(), raw.end());
  const int64_t frames = (int64_t)b.size() / C;
  for (int law = 0; law < 2; ++law) {
    std::vector<float> out((size_t)C * (size_t)frames);
    count(p2phd_g711_decode_host(b.data(), frames, C, law, out.data(), frames));
  }
  std::vector<float> out((size_t)C * (size_t)frames);
  count(p2phd_g711_decode_host(b.data(), frames, C, 2, out.data(), frames));
  count(p2phd_g711_decode_host(b.data(), frames, C, 0, out.data(), frames - 1));
}

void variants_ima(const std::vector<uint8_t>& raw, int C, int align) {
  run_ima(raw, C, align, true);
  // every truncation to a length inside the first block and a group, every 61st up to 2048, about 200 lengths above
  const size_t dense = (size_t)align + 8 * (size_t)C, coarse = raw.size() / 200 + 61;
  for (size_t len = 0; len < raw.size(); len += len < dense ? 1 : len < 2048 ? 61 : coarse) run_ima(std::vector<uint8_t>(raw.begin(), raw.begin() + len), C, align);
  // single flipped bits: the headers and the first group of the first three blocks
  for (int B = 0; B < 3; ++B)
    for (int bit = 0; bit < 8 * 8 * C; ++bit) {
      const size_t at = (size_t)B * (size_t)align + (size_t)bit / 8;
      if (at >= raw.size()) break;
      std::vector<uint8_t> v(raw);
      v[at] ^= (uint8_t)(1u << (bit % 8));
      run_ima(v, C, align);
    }
  // layouts the contract does not admit, on the same bytes
  for (int a : {0, 4 * C, 8 * C - 4, align + 1, align + 2, 65536})
    if (a < 8 * C || a % (4 * C) || a > 65535) run_ima(raw, C, a);
  run_ima(raw, 0, align);
  run_ima(raw, 9, 72);
}

uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    static const int layouts[][2] = {{1, 8}, {1, 36}, {2, 16}, {2, 72}, {3, 24}, {3, 108}, {8, 64}, {1, 256}, {2, 2048}, {8, 8192}};
    for (const auto& l : layouts) {
      const int C = l[0], align = l[1];
      const size_t blocks = align > 1024 ? 3 : 7;
      std::vector<uint8_t> raw(blocks * (size_t)align + (size_t)(4 * C * 2 + 3));      // a partial last block of one group, and three stray bytes
      for (auto& v : raw) v = (uint8_t)rnd();
      const long ok0 = g_ok, ref0 = g_refused;
      variants_ima(raw, C, align);
      printf("ima %d ch, block_align %d: %ld calls answered, %ld refused\n", C, align, g_ok - ok0, g_refused - ref0);
    }
    for (int C : {1, 2, 3, 8}) {
      std::vector<uint8_t> raw(256 * (size_t)C + 5);
      for (size_t i = 0; i < raw.size(); ++i) raw[i] = (uint8_t)(i / C);
      for (size_t len = 0; len <= raw.size(); ++len) run_g711(std::vector<uint8_t>(raw.begin(), raw.begin() + len), C);
    }
    printf("fixtures: %ld calls answered, %ld refused\n", g_ok, g_refused);
    return 0;
  }
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> file;
    uint8_t chunk[65536];
    for (size_t k; (k = fread(chunk, 1, sizeof(chunk), f)) > 0;) file.insert(file.end(), chunk, chunk + k);
    fclose(f);
    // the fmt and data chunks of a RIFF/WAVE file (the parser of record is data/wavio.py; this one only finds the payload)
    int tag = 0, C = 0, align = 0;
    size_t pos = 12, off = 0, len = 0;
    while (pos + 8 <= file.size()) {
      const uint32_t size = le32(&file[pos + 4]);
      if (!memcmp(&file[pos], "fmt ", 4) && pos + 8 + 16 <= file.size()) {
        tag = le16(&file[pos + 8]); C = le16(&file[pos + 10]); align = le16(&file[pos + 20]);
        if (tag == 0xFFFE && size >= 26 && pos + 8 + 26 <= file.size()) tag = le16(&file[pos + 8 + 24]);
      } else if (!memcmp(&file[pos], "data", 4)) {
        off = pos + 8; len = size < file.size() - off ? size : file.size() - off;
        break;
      }
      pos += 8 + (size_t)size + (size & 1);
    }
    if (!off || (tag != 6 && tag != 7 && tag != 0x11) || C < 1) { fprintf(stderr, "%s: no coded data chunk (tag %d)\n", argv[a], tag); return 1; }
    const std::vector<uint8_t> raw(file.begin() + off, file.begin() + off + len);
    const long ok0 = g_ok, ref0 = g_refused;
    if (tag == 0x11) variants_ima(raw, C, align);
    else for (size_t l = 0; l <= raw.size(); l += l < 512 ? 1 : 61) run_g711(std::vector<uint8_t>(raw.begin(), raw.begin() + l), C);
    printf("%s (tag %d, %d ch, block_align %d, %zu bytes): %ld calls answered, %ld refused\n", argv[a], tag, C, align, len, g_ok - ok0, g_refused - ref0);
  }
  return 0;
}
