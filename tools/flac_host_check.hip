// Stand-alone driver of the HOST part of csrc/flac.hip for a sanitizer build (never a test, never run on a GPU machine):
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Ipix2pixhdaudiosr_amd/csrc \
//         tools/flac_host_check.hip pix2pixhdaudiosr_amd/csrc/flac.hip -o flac_host_check && ./flac_host_check a.flac b.flac ...
//
// For every file: info, index and host decode of the file as it stands, then of corrupted variants of it -- every single flipped bit
// of its first `kBits` bits and of as many bits around every frame start, every truncation to a length below 4096 and every 97th
// above, and table rows bent to point past the buffer.  The library's answers are counted, not judged: the point is that no variant
// makes the host code read or write outside its buffers, which the sanitizer watches.  It links none of the device entry's callers:
// the few symbols of core.hip that flac.hip names are defined here.
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
constexpr int kBits = 2048;
long g_ok = 0, g_refused = 0;

void run(const std::vector<uint8_t>& raw, bool bend) {
  // an exact-size copy on the heap: one byte past either end is the sanitizer's
  std::vector<uint8_t> b(raw.begin(), raw.end());
  p2phd_flac_streaminfo si;
  if (p2phd_flac_info(b.data(), (int64_t)b.size(), &si)) { ++g_refused; return; }
  const int64_t n = p2phd_flac_index(b.data(), (int64_t)b.size(), nullptr, 0);
  if (n < 0) { ++g_refused; return; }
  std::vector<int64_t> table((size_t)n * P2PHD_FLAC_ROW_WORDS);
  if (n && p2phd_flac_index(b.data(), (int64_t)b.size(), table.data(), n) != n) { ++g_refused; return; }
  int64_t total = 0;
  for (int64_t f = 0; f < n; ++f) total += table[f * P2PHD_FLAC_ROW_WORDS + 3];
  std::vector<int32_t> out((size_t)si.channels * (size_t)total);
  if (bend && n) {
    table[(n / 2) * P2PHD_FLAC_ROW_WORDS + 1] += 7;              // a frame said to be longer than it is
    if (p2phd_flac_decode_host(b.data(), (int64_t)b.size(), table.data(), 0, n, si.channels, out.data(), total)) ++g_refused; else ++g_ok;
    table[(n / 2) * P2PHD_FLAC_ROW_WORDS + 1] -= 12;             // ... and shorter
    if (p2phd_flac_decode_host(b.data(), (int64_t)b.size(), table.data(), 0, n, si.channels, out.data(), total)) ++g_refused; else ++g_ok;
    table[(n / 2) * P2PHD_FLAC_ROW_WORDS + 1] += 5;
    table[(n - 1) * P2PHD_FLAC_ROW_WORDS + 0] += 1 << 20;        // a frame outside the buffer
    if (p2phd_flac_decode_host(b.data(), (int64_t)b.size(), table.data(), 0, n, si.channels, out.data(), total)) ++g_refused; else ++g_ok;
    table[(n - 1) * P2PHD_FLAC_ROW_WORDS + 0] -= 1 << 20;
    table[(n - 1) * P2PHD_FLAC_ROW_WORDS + 3] += 9;              // samples outside the rows
    if (p2phd_flac_decode_host(b.data(), (int64_t)b.size(), table.data(), 0, n, si.channels, out.data(), total)) ++g_refused; else ++g_ok;
    table[(n - 1) * P2PHD_FLAC_ROW_WORDS + 3] -= 9;
    table[(n / 2) * P2PHD_FLAC_ROW_WORDS + 4] = si.channels < 8 ? si.channels : 8;   // an assignment of more channels than the rows
    if (p2phd_flac_decode_host(b.data(), (int64_t)b.size(), table.data(), 0, n, si.channels, out.data(), total)) ++g_refused; else ++g_ok;
    return;
  }
  if (p2phd_flac_decode_host(b.data(), (int64_t)b.size(), table.data(), 0, n, si.channels, out.data(), total)) ++g_refused; else ++g_ok;
}
}  // namespace

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> raw;
    uint8_t chunk[65536];
    for (size_t k; (k = fread(chunk, 1, sizeof(chunk), f)) > 0;) raw.insert(raw.end(), chunk, chunk + k);
    fclose(f);
    const long ok0 = g_ok;
    run(raw, false);
    if (g_ok != ok0 + 1) { fprintf(stderr, "%s does not decode as it stands: %s\n", argv[a], p2phd::g_text); return 1; }
    run(raw, true);
    // where the frames start, from the good index
    std::vector<int64_t> starts{0};
    const int64_t n = p2phd_flac_index(raw.data(), (int64_t)raw.size(), nullptr, 0);
    std::vector<int64_t> table((size_t)n * P2PHD_FLAC_ROW_WORDS);
    p2phd_flac_index(raw.data(), (int64_t)raw.size(), table.data(), n);
    for (int64_t k = 0; k < n && k < 6; ++k) starts.push_back(table[k * P2PHD_FLAC_ROW_WORDS]);
    for (int64_t s : starts)
      for (int bit = 0; bit < kBits && s + bit / 8 < (int64_t)raw.size(); ++bit) {
        std::vector<uint8_t> v(raw);
        v[s + bit / 8] ^= (uint8_t)(0x80 >> (bit % 8));
        run(v, false);
      }
    for (size_t len = 0; len < raw.size(); len += len < 4096 ? 1 : 97) run(std::vector<uint8_t>(raw.begin(), raw.begin() + len), false);
    printf("%s: %ld variants decoded, %ld refused\n", argv[a], g_ok - ok0, g_refused);
  }
  return 0;
}
