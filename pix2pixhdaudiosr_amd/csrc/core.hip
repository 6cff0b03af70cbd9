// Error channel, ABI version and device query of libp2phd_hip.so.
#include "common.h"
#include "convplan.h"
#include "streamgrid.h"
#include <cstring>

namespace p2phd {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace p2phd

namespace p2phd { int g_opt_gconv_bm = 0; int g_opt_wgrad_tm = 0; int g_opt_wgrad_xcd = 1; int g_opt_march = 1; int g_opt_cls_skip = 1; int g_opt_gconv_halo = 1; int g_opt_cw_inject = 0; int g_opt_tile128x192 = 1; int g_opt_mdct_generic = 0; int g_opt_mdct_iters = 0; int g_opt_c7_generic = 0; int g_opt_dfirst = 1; int g_opt_dlast = 1; int g_opt_c7_abl = 0; int g_opt_reflect_generic = 0; int g_opt_splitk_tail = 1; int g_opt_truepeak_grid = 0; int g_opt_limiter_grid = 0; int g_opt_speechlevel_grid = 0; int g_opt_cus = 0;
unsigned long long g_launch_count[LC_FAMILIES] = {};
int device_cus() {
  static int cached[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    hipDeviceProp_t prop;
    cached[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
  }
  return cached[dev];
}
}

// scratch of the fixed-order cross-workgroup reductions (common.h): zero-initialised with the code object
namespace {
constexpr int kFoldRegions = 9;
// (the last region, FOLD_LTAS, is tickets only: p2phd_ltas keeps its partials in the caller's workspace)
constexpr size_t kFoldFloats[kFoldRegions] = {size_t(4) << 20, size_t(1) << 20, size_t(1) << 20, 4096, size_t(16) << 20, size_t(5) << 16, size_t(1) << 16, size_t(1) << 16, 0};
constexpr int kFoldTickets[kFoldRegions] = {2048, 1024, 8, 8, 256, 8, 8, 8, 1024};
constexpr int kFoldTicketsAll = 2048 + 1024 + 16 + 256 + 8 + 8 + 8 + 1024;
__device__ float g_fold_part[(size_t(22) << 20) + 4096 + (size_t(7) << 16)];      // 90 MiB, zero-initialised with the code object
__device__ unsigned g_fold_ticket[kFoldTicketsAll];
}  // namespace
namespace p2phd {
namespace {
struct FoldDev { float* part = nullptr; unsigned* ticket = nullptr; hipStream_t last[kFoldRegions] = {}; bool used[kFoldRegions] = {}; hipEvent_t ev[kFoldRegions] = {}; bool ev_set[kFoldRegions] = {}; };
FoldDev g_fold_dev[64];
thread_local hipStream_t g_fold_pending_stream = nullptr;
FoldDev* fold_dev() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  FoldDev& f = g_fold_dev[dev];
  if (f.part == nullptr) {                                      // (the symbol has one address per device)
    void* p = nullptr; void* t = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_fold_part)) != hipSuccess || hipGetSymbolAddress(&t, HIP_SYMBOL(g_fold_ticket)) != hipSuccess)
      return nullptr;
    f.part = static_cast<float*>(p); f.ticket = static_cast<unsigned*>(t);
  }
  return &f;
}
bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
}  // namespace

thread_local int g_fold_pending = -1;

FoldScratch fold_capacity(int region) {
  if (region < 0 || region >= kFoldRegions) return FoldScratch{nullptr, nullptr, 0, 0};
  return FoldScratch{nullptr, nullptr, kFoldFloats[region], kFoldTickets[region]};
}

// The region's partial rows and tickets, for a launch on `stream`.  One region serves ONE stream at a time.  Round 5 (advisor):
// the region's last launch is remembered as an EVENT recorded behind it (fold_launched), never as a stream handle to be
// queried later -- the handle may belong to a stream that has been destroyed since, and hipStreamQuery on it is undefined.
// A launch that arrives on another stream makes that stream wait for the event: the two launches of the family are ordered
// on the device.  Streams under capture enqueue nothing (their launches run in graph order when the graph is replayed, and a
// capture is entered behind a synchronisation), so they neither wait nor record.
FoldScratch fold_scratch(int region, hipStream_t stream) {
  FoldDev* f = fold_dev();
  if (f == nullptr || region < 0 || region >= kFoldRegions) { set_error("reduction scratch unavailable"); return FoldScratch{nullptr, nullptr, 0, 0}; }
  const bool cap = capturing(stream);
  if (f->used[region] && f->last[region] != stream && f->ev_set[region] && !cap) {
    if (hipStreamWaitEvent(stream, f->ev[region], 0) != hipSuccess) {
      (void)hipGetLastError();
      set_error("reduction-scratch region %d: cannot order this stream behind the region's previous launch "
                "(include/p2phd.h, \"Streams\")", region);
      return FoldScratch{nullptr, nullptr, 0, 0};
    }
  }
  f->used[region] = true;
  f->last[region] = stream;
  g_fold_pending = cap ? -1 : region;
  g_fold_pending_stream = stream;
  size_t fo = 0; int to = 0;
  for (int r = 0; r < region; ++r) { fo += kFoldFloats[r]; to += kFoldTickets[r]; }
  const FoldScratch cap_of = fold_capacity(region);
  return FoldScratch{f->part + fo, f->ticket + to, cap_of.floats, cap_of.tickets};
}

void fold_launched() {
  const int region = g_fold_pending;
  g_fold_pending = -1;
  FoldDev* f = fold_dev();
  if (f == nullptr || region < 0 || region >= kFoldRegions) return;
  if (f->ev[region] == nullptr && hipEventCreateWithFlags(&f->ev[region], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); f->ev[region] = nullptr; return; }
  if (hipEventRecord(f->ev[region], g_fold_pending_stream) == hipSuccess) f->ev_set[region] = true;
  else (void)hipGetLastError();
}
}  // namespace p2phd

// Re-arms every arrival ticket of the fixed-order reductions (an aborted or faulted launch may have left one non-zero, which
// would make every later launch of that kernel family fold at the wrong moment): a 17 KB memset on `stream`; the Python
// mirror issues it once per training step beside its own per-step memset (_ops.begin_step).
extern "C" int p2phd_reduction_reset(void* stream) {
  void* t = nullptr;
  if (hipGetSymbolAddress(&t, HIP_SYMBOL(g_fold_ticket)) != hipSuccess) { p2phd::set_error("reduction_reset: no device symbol"); return P2PHD_ELAUNCH; }
  if (hipMemsetAsync(t, 0, sizeof(unsigned) * kFoldTicketsAll, (hipStream_t)stream) != hipSuccess) {
    p2phd::set_error("reduction_reset: memset failed");
    return P2PHD_ELAUNCH;
  }
  return P2PHD_OK;
}

// The grid of a grid-stride launch (streamgrid.h: the function the launchers take theirs from).  Host arithmetic only.
extern "C" int p2phd_stream_grid(const char* family, int dtype, int64_t work, int rows, int64_t* unit_work, int* wanted, int* used) {
  P2PHD_REQUIRE(family && unit_work && wanted && used, "stream_grid: null pointer");
  *unit_work = 0; *wanted = *used = 0;
  const p2phd::StreamFamily f = p2phd::stream_family(family);
  P2PHD_REQUIRE(f != p2phd::SG_UNKNOWN, "stream_grid: unknown family \"%s\" (include/p2phd.h lists them)", family);
  P2PHD_REQUIRE(dtype == P2PHD_BF16 || dtype == P2PHD_F32, "stream_grid: unsupported dtype %d", dtype);
  P2PHD_REQUIRE(work >= 0 && work <= (int64_t(1) << 40) && rows >= 1 && rows <= 65535, "stream_grid: need 0 <= work <= 2^40 and 1 <= rows <= 65535 (work %lld, rows %d)",
                (long long)work, rows);
  if (work == 0) return P2PHD_OK;                                 // nothing to launch
  const p2phd::StreamGrid g = p2phd::stream_grid_of(f, dtype, work, rows);
  *unit_work = g.unit_work; *wanted = g.wanted; *used = g.used;
  return P2PHD_OK;
}

extern "C" int p2phd_set_option(const char* name, int value) {
  if (name && !strcmp(name, "gconv_bm") && (value == 0 || value == 128 || value == 192 || value == 256 || value == 258 || value == 512)) { p2phd::g_opt_gconv_bm = value; return P2PHD_OK; }
  if (name && !strcmp(name, "wgrad_tm") && (value == 0 || value == 128)) { p2phd::g_opt_wgrad_tm = value; return P2PHD_OK; }
  if (name && !strcmp(name, "march") && (value == 0 || value == 1)) { p2phd::g_opt_march = value; return P2PHD_OK; }
  if (name && !strcmp(name, "cls_skip") && (value == 0 || value == 1)) { p2phd::g_opt_cls_skip = value; return P2PHD_OK; }   // (changes the packed layout: repack after a change)
  if (name && !strcmp(name, "gconv_halo") && (value == 0 || value == 1)) { p2phd::g_opt_gconv_halo = value; return P2PHD_OK; }
  if (name && !strcmp(name, "tile128x192") && (value == 0 || value == 1)) { p2phd::g_opt_tile128x192 = value; return P2PHD_OK; }   // (A/B: the 128 x 192 tile of small planes vs 128 x 128)
  if (name && !strcmp(name, "dlast") && (value == 0 || value == 1)) { p2phd::g_opt_dlast = value; return P2PHD_OK; }     // (A/B, parity tests: dlast.hip vs the W-fold path)
  if (name && !strcmp(name, "dfirst") && (value == 0 || value == 1)) { p2phd::g_opt_dfirst = value; return P2PHD_OK; }   // (A/B, parity tests: dfirst.hip vs the W-fold path)
#ifdef P2PHD_CHECK_WAITS
  if (name && !strcmp(name, "cw_inject") && (value == 0 || value == 1)) { p2phd::g_opt_cw_inject = value; return P2PHD_OK; }   // (check build only: see p2phd_wait_check)
#endif
  if (name && !strcmp(name, "wgrad_xcd") && (value == 0 || value == 1)) { p2phd::g_opt_wgrad_xcd = value; return P2PHD_OK; }
  if (name && !strcmp(name, "reflect_generic") && (value == 0 || value == 1)) { p2phd::g_opt_reflect_generic = value; return P2PHD_OK; }
  if (name && !strcmp(name, "mdct_iters") && value >= 0 && value <= 8) { p2phd::g_opt_mdct_iters = value; return P2PHD_OK; }
  if (name && !strcmp(name, "splitk_tail") && value >= 0 && value <= 2) { p2phd::g_opt_splitk_tail = value; return P2PHD_OK; }
  if (name && !strcmp(name, "cus") && value >= 0 && value <= 4096) { p2phd::g_opt_cus = value; return P2PHD_OK; }
  if (name && !strcmp(name, "truepeak_grid") && value >= 0 && value <= 65536) { p2phd::g_opt_truepeak_grid = value; return P2PHD_OK; }
  if (name && !strcmp(name, "limiter_grid") && value >= 0 && value <= 16384) { p2phd::g_opt_limiter_grid = value; return P2PHD_OK; }
  if (name && !strcmp(name, "speechlevel_grid") && value >= 0 && value <= 16384) { p2phd::g_opt_speechlevel_grid = value; return P2PHD_OK; }
  if (name && !strcmp(name, "c7_abl")) { p2phd::g_opt_c7_abl = value; return P2PHD_OK; }
  if (name && !strcmp(name, "c7_generic") && (value == 0 || value == 1)) { p2phd::g_opt_c7_generic = value; return P2PHD_OK; }
  if (name && !strcmp(name, "mdct_generic") && (value == 0 || value == 1)) { p2phd::g_opt_mdct_generic = value; return P2PHD_OK; }
  p2phd::set_error("set_option: unknown option or value (%s = %d)", name ? name : "(null)", value);
  return P2PHD_EINVAL;
}

extern "C" int64_t p2phd_launch_count(const char* family, int reset) {
  static const char* names[p2phd::LC_FAMILIES] = {"gconv", "halo", "cls_skip", "march", "march_w", "wgrad", "splitk", "tile256", "tile128x192",
                                                       "dfirst", "dlast", "c7", "thin_wgrad", "timed_pack", "timed_frames", "stitch", "pcm",
                                                       "metrics_rows", "xover", "specimg", "loudness", "truepeak", "limiter", "bandwidth", "stereo", "rateconv",
                                                       "normscope", "shaper", "flac", "flacenc", "wavcodec", "speechlevel", "normrows", "wpack_generic", "wpack_dense", "wpack_transposed",
                                                       "wpack_kmajor", "wpack_kmajor_t", "wpack_merged", "wpack_fp8", "wpack_frag"};
  if (family == nullptr) {                                       // all families at once
    if (reset) for (auto& c : p2phd::g_launch_count) c = 0;
    return 0;
  }
  for (int i = 0; i < p2phd::LC_FAMILIES; ++i)
    if (!strcmp(family, names[i])) {
      const int64_t v = (int64_t)p2phd::g_launch_count[i];
      if (reset) p2phd::g_launch_count[i] = 0;
      return v;
    }
  p2phd::set_error("launch_count: unknown kernel family %s", family);
  return -1;
}

extern "C" const char* p2phd_last_error(void) { return p2phd::g_err; }
extern "C" int p2phd_abi_version(void) { return 1; }
// 1: this library's 16-bit storage type (dtype code P2PHD_BF16) is bf16; 2: IEEE fp16 (the -DP2PHD_F16 build, libp2phd_hip_f16.so)
extern "C" int p2phd_half_type(void) {
#ifdef P2PHD_F16
  return 2;
#else
  return 1;
#endif
}

extern "C" int p2phd_device_info(char* name, int cap) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    p2phd::set_error("no HIP device");
    return P2PHD_ELAUNCH;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    p2phd::set_error("hipGetDeviceProperties failed");
    return P2PHD_ELAUNCH;
  }
  if (name && cap > 0) {
    strncpy(name, prop.gcnArchName, cap - 1);
    name[cap - 1] = 0;
  }
  return prop.multiProcessorCount;
}
