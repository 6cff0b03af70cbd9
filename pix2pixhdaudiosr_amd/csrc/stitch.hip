// Whole-file generation (pix2pixhdaudiosr_amd/generate/): the two ends of the waveform -> segments -> generator -> segments ->
// waveform path that are not a transform or a conv.
//
//   gather  audio[L] -> seg[S,T], seg[s,i] = audio[s * stride + i], zero beyond L.  stride = T is the reference's
//           seg_pad_audio (data/audio_dataset.py:124-135); stride < T makes neighbouring segments share V = T - stride samples.
//   stitch  seg[S,T] -> out[L_out]: each sample from the one or two segments that cover it.  Inside an overlap the later
//           segment fades in with w = sin^2(pi (i + 1/2) / (2 V)) and the earlier one fades out with 1 - w; V = 0 is the
//           reference's torch.cat(...).view(1, -1) times `gain`.
//
// The `_planar` entries run the same two kernels over C rows in one launch each (blockIdx.y = row): audio[C][ld] -> seg[C*S][T],
// channel-major, and seg[C*S][T] -> out[C][ld].  A row goes through the code of the single-row entries, which are the C = 1 case.
// The `_ragged` entries run them over N clip rows that share nothing but T and stride -- channels of several files, each with its
// own base, length L_j and segment count S_j, row j's segments at rows row0_j .. row0_j + S_j - 1 of one seg[rows, T] -- through
// the same two row bodies (gather_row, stitch_row): a row's bits are the planar entry's on that clip alone.
// The `_stream` entry stitches one window of a clip that is generated in windows -- K consecutive segments of every channel -- and
// fades its first segment with the tail the window before left in a carry buffer, through stitch_row again: the windows' outputs
// laid one behind the other are the planar stitch of the whole clip.
//
// Both are streaming kernels (one pass, no reuse, no atomics): one thread per four consecutive outputs, 16-byte accesses
// where the addresses allow.  The cross-fade is evaluated in double and rounded once, so an output is the correctly rounded
// value of the formula whatever the two operands' signs (a float evaluation loses bits where they cancel); the fp64 sine
// runs on at most half of the samples of a kernel that is a few microseconds long.
#include "common.h"
#include "convplan.h"
#include "streamgrid.h"
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>

namespace {
constexpr int kThreads = 256;

// One row of a gather: audio[L] -> out[total], total = S * T.  The body of every gather kernel of this file.
__device__ __forceinline__ void gather_row(const float* __restrict__ audio, long L, long T, long stride, long total, float* __restrict__ out,
                                           int vec4) {
  const long quads = (total + 3) >> 2;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
    const long e0 = q << 2;
    if (vec4) {                                                   // T, stride multiples of 4: a quad stays in one row, 16-byte aligned
      const long s = e0 / T, src = s * stride + (e0 - s * T);
      float4 v;
      if (src + 4 <= L) {
        v = *reinterpret_cast<const float4*>(audio + src);
      } else {
        v.x = src < L ? audio[src] : 0.f;
        v.y = src + 1 < L ? audio[src + 1] : 0.f;
        v.z = src + 2 < L ? audio[src + 2] : 0.f;
        v.w = 0.f;
      }
      *reinterpret_cast<float4*>(out + e0) = v;
    } else {
      const long n = min(4l, total - e0);
      for (long j = 0; j < n; ++j) {
        const long e = e0 + j, s = e / T, src = s * stride + (e - s * T);
        out[e] = src < L ? audio[src] : 0.f;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void segments_gather_kernel(const float* __restrict__ audio, long L, long T, long stride,
                                                                   long total, float* __restrict__ out, int vec4, long ld) {
  // row of a planar clip; its segments follow the previous row's
  gather_row(audio + (long)blockIdx.y * ld, L, T, stride, total, out + (long)blockIdx.y * total, vec4);
}

// The ragged launches: blockIdx.y = clip row, whose four words (address, L, S, row0) every workgroup reads from the table the
// entry has checked and copied.  The grid is the longest row's (streamgrid.h, SG_STITCH_RAGGED); a shorter row's surplus
// workgroups leave at once.  The 16-byte paths are the row's own: its base and its rows of `seg` decide, not the launch.
__global__ __launch_bounds__(kThreads) void segments_gather_ragged_kernel(const long* __restrict__ table, long T, long stride,
                                                                          float* __restrict__ seg, int tvec) {
  const long* row = table + 4 * (long)blockIdx.y;
  const long total = row[2] * T;
  if ((long)blockIdx.x * (kThreads * 4) >= total) return;
  const float* audio = reinterpret_cast<const float*>(row[0]);
  float* out = seg + row[3] * T;
  const int vec4 = tvec && ((reinterpret_cast<uintptr_t>(audio) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  gather_row(audio, row[1], T, stride, total, out, vec4);
}

// `head`: the tail of the segment in front of segment 0 -- head[i] is its sample i + stride, i < V -- or nullptr where segment 0 is
// the clip's first (every entry but the streamed one).  A later segment's is inside `seg`.
__device__ __forceinline__ float stitch_one(const float* __restrict__ seg, const float* __restrict__ head, long n, long S, long T, long stride,
                                            long V, double gain, double step) {
  const long a = min(n / stride, S - 1);                          // the latest segment that covers n
  const long i = n - a * stride;
  const double cur = (double)seg[a * T + i];
  const float* tail = a > 0 ? seg + (a - 1) * T + stride : head;  // the previous segment's samples [stride, T)
  if (tail == nullptr || i >= V) return (float)(gain * cur);
  const double sn = sin(((double)i + 0.5) * step);
  const double w = sn * sn;
  return (float)(gain * (w * cur + (1.0 - w) * (double)tail[i]));
}

// One row of a stitch: seg[S, T] -> out[L_out].  The body of every stitch kernel of this file.
__device__ __forceinline__ void stitch_row(const float* __restrict__ seg, const float* __restrict__ head, long S, long T, long stride, long V,
                                           float gain, float* __restrict__ out, long L_out, int vec4) {
  const long quads = (L_out + 3) >> 2;
  const double step = V > 0 ? 3.14159265358979323846 / (2.0 * (double)V) : 0.0;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long)gridDim.x * blockDim.x) {
    const long n0 = q << 2;
    if (vec4 && n0 + 4 <= L_out) {
      const long a = min(n0 / stride, S - 1), i0 = n0 - a * stride;
      const long src = a * T + i0;
      float4 v;
      if (((a == 0 && head == nullptr) || i0 >= V) && a == min((n0 + 3) / stride, S - 1) && (src & 3) == 0) {     // plain run of one segment
        v = *reinterpret_cast<const float4*>(seg + src);
        v.x *= gain; v.y *= gain; v.z *= gain; v.w *= gain;
      } else {
        v.x = stitch_one(seg, head, n0, S, T, stride, V, gain, step);
        v.y = stitch_one(seg, head, n0 + 1, S, T, stride, V, gain, step);
        v.z = stitch_one(seg, head, n0 + 2, S, T, stride, V, gain, step);
        v.w = stitch_one(seg, head, n0 + 3, S, T, stride, V, gain, step);
      }
      *reinterpret_cast<float4*>(out + n0) = v;
    } else {
      for (long n = n0; n < min(n0 + 4, L_out); ++n) out[n] = stitch_one(seg, head, n, S, T, stride, V, gain, step);
    }
  }
}

__global__ __launch_bounds__(kThreads) void segments_stitch_kernel(const float* __restrict__ seg, long S, long T, long stride, long V,
                                                                   float gain, float* __restrict__ out, long L_out, int vec4, long ld) {
  stitch_row(seg + (long)blockIdx.y * S * T, nullptr, S, T, stride, V, gain, out + (long)blockIdx.y * ld, L_out, vec4);
}

__global__ __launch_bounds__(kThreads) void segments_stitch_ragged_kernel(const float* __restrict__ seg, const long* __restrict__ table,
                                                                          long T, long stride, long V, float gain) {
  const long* row = table + 4 * (long)blockIdx.y;
  const long L_out = row[1];
  if ((long)blockIdx.x * (kThreads * 4) >= L_out) return;
  float* out = reinterpret_cast<float*>(row[0]);
  const float* mine = seg + row[3] * T;
  const int vec4 = ((reinterpret_cast<uintptr_t>(mine) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  stitch_row(mine, nullptr, row[2], T, stride, V, gain, out, L_out, vec4);
}

// The streamed stitch: one window of a clip that goes through the pipeline in windows, K consecutive segments of each of C
// channels.  blockIdx.y = channel.  Segment 0 of the window cross-fades with `carry_in`, the raw tail the window before it left
// (nullptr: the window holds the clip's first segment), through the one row body, so a sample is the whole-clip stitch's at its
// position, bit for bit.  The window's own last tail -- seg[c, K - 1, stride .. T) as it stands, unscaled -- goes to `carry_out` for
// the window behind it: V floats per channel, written by the grid's first threads with plain stores.  The 16-byte paths are the
// row's own: its base in `seg` and in `out` decide, not the launch.
__global__ __launch_bounds__(kThreads) void segments_stitch_stream_kernel(const float* __restrict__ seg, long K, long T, long stride, long V,
                                                                          float gain, const float* __restrict__ carry_in,
                                                                          float* __restrict__ carry_out, float* __restrict__ out, long ld,
                                                                          long n_out) {
  const long c = blockIdx.y;
  const float* mine = seg + c * K * T;
  float* dst = out + c * ld;
  const int vec4 = ((reinterpret_cast<uintptr_t>(mine) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  stitch_row(mine, carry_in != nullptr ? carry_in + c * V : nullptr, K, T, stride, V, gain, dst, n_out, vec4);
  if (carry_out != nullptr) {
    const float* tail = mine + (K - 1) * T + stride;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (long)gridDim.x * blockDim.x) carry_out[c * V + i] = tail[i];
  }
}

int stream_grid(int64_t elems) { return p2phd::stream_grid_of(p2phd::SG_STITCH, P2PHD_F32, elems, 1).used; }     // (streamgrid.h)

// every row's first element must be 16-byte aligned for the float4 paths: the bases, and the row pitches when C > 1
bool rows_aligned(const void* a, const void* b, int64_t C, int64_t pitch_a, int64_t pitch_b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 && (C == 1 || ((pitch_a | pitch_b) & 3) == 0);
}

int gather_rows(const char* what, const float* audio, int64_t C, int64_t ld, int64_t L, int64_t T, int64_t stride, int64_t S, float* out,
                void* stream) {
  P2PHD_REQUIRE(L >= 0 && T >= 1 && S >= 1, "%s: need L >= 0, T >= 1, S >= 1 (L %lld, T %lld, S %lld)", what, (long long)L, (long long)T,
                (long long)S);
  P2PHD_REQUIRE(stride >= 1 && stride <= T, "%s: stride must be in [1, T], got %lld (T %lld)", what, (long long)stride, (long long)T);
  P2PHD_REQUIRE(C >= 1 && C <= 65535 && ld >= L, "%s: need 1 <= C <= 65535 and ld >= L (C %lld, ld %lld, L %lld)", what, (long long)C,
                (long long)ld, (long long)L);
  P2PHD_REQUIRE(S <= (int64_t(1) << 40) / T / C, "%s: C * S * T too large", what);
  P2PHD_REQUIRE(out && (audio || L == 0), "%s: null pointer", what);
  const int vec4 = (T & 3) == 0 && (stride & 3) == 0 && rows_aligned(audio, out, C, ld, S * T);
  hipLaunchKernelGGL(segments_gather_kernel, dim3(stream_grid(S * T), (unsigned)C), dim3(kThreads), 0, (hipStream_t)stream, audio, (long)L,
                     (long)T, (long)stride, (long)(S * T), out, vec4, (long)ld);
  ++p2phd::g_launch_count[p2phd::LC_STITCH];
  return p2phd::check_launch(what);
}

int stitch_rows(const char* what, const float* seg, int64_t C, int64_t S, int64_t T, int64_t stride, float gain, float* out, int64_t ld,
                int64_t L_out, void* stream) {
  P2PHD_REQUIRE(S >= 1 && T >= 1, "%s: need S >= 1 and T >= 1 (S %lld, T %lld)", what, (long long)S, (long long)T);
  const int64_t V = T - stride;
  P2PHD_REQUIRE(V >= 0 && V <= T / 2, "%s: the overlap T - stride must be in [0, T/2], got %lld (T %lld)", what, (long long)V, (long long)T);
  P2PHD_REQUIRE(C >= 1 && C <= 65535, "%s: need 1 <= C <= 65535, got %lld", what, (long long)C);
  P2PHD_REQUIRE(S <= (int64_t(1) << 40) / T / C, "%s: C * S * T too large", what);
  P2PHD_REQUIRE(L_out >= 0 && L_out <= (S - 1) * stride + T, "%s: L_out %lld is beyond the %lld samples the segments span", what,
                (long long)L_out, (long long)((S - 1) * stride + T));
  P2PHD_REQUIRE(ld >= L_out, "%s: ld %lld is shorter than L_out %lld", what, (long long)ld, (long long)L_out);
  if (L_out == 0) return P2PHD_OK;
  P2PHD_REQUIRE(seg && out, "%s: null pointer", what);
  const int vec4 = rows_aligned(seg, out, C, S * T, ld);
  hipLaunchKernelGGL(segments_stitch_kernel, dim3(stream_grid(L_out), (unsigned)C), dim3(kThreads), 0, (hipStream_t)stream, seg, (long)S,
                     (long)T, (long)stride, (long)V, gain, out, (long)L_out, vec4, (long)ld);
  ++p2phd::g_launch_count[p2phd::LC_STITCH];
  return p2phd::check_launch(what);
}

// ---- the ragged entries: N clip rows of their own base, length and segment count in one launch ----------------------------------
//
// The table (N x 4 int64: address, L, S, row0) is checked on the host, copied into a pinned slot the library owns and from there,
// on the launch's stream, into the caller's device buffer: the kernel reads what was checked, whatever the caller does with its
// own copy behind the call.  The slots are a ring; one is taken again when eight later tables have been queued, and only then --
// a caller that queues so many without ever synchronising -- does the host wait for the slot's own copy (an event behind it).
constexpr int kTableSlots = 8;
struct TableSlot { void* host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; int dev = -1; bool pending = false; };
TableSlot g_table_slots[kTableSlots];
int g_table_next = 0;
std::mutex g_table_mutex;

int ragged_grid(int64_t longest) { return p2phd::stream_grid_of(p2phd::SG_STITCH_RAGGED, P2PHD_F32, longest, 1).used; }     // (streamgrid.h)

// Every check of both entries -> the longest row's outputs in *longest (S * T of the gather, L of the stitch).
int check_table(const char* what, const int64_t* table, int64_t N, int64_t rows, int64_t T, int64_t stride, bool stitch, const void* seg,
                const void* table_dev, int64_t* longest) {
  P2PHD_REQUIRE(N >= 1 && N <= 65535, "%s: need 1 <= N <= 65535 clip rows, got %lld", what, (long long)N);
  P2PHD_REQUIRE(table && table_dev, "%s: null table", what);
  P2PHD_REQUIRE(T >= 1 && rows >= 1, "%s: need T >= 1 and rows >= 1 (T %lld, rows %lld)", what, (long long)T, (long long)rows);
  const int64_t V = T - stride;
  if (stitch)
    P2PHD_REQUIRE(V >= 0 && V <= T / 2, "%s: the overlap T - stride must be in [0, T/2], got %lld (T %lld)", what, (long long)V, (long long)T);
  else
    P2PHD_REQUIRE(stride >= 1 && stride <= T, "%s: stride must be in [1, T], got %lld (T %lld)", what, (long long)stride, (long long)T);
  P2PHD_REQUIRE(rows <= (int64_t(1) << 40) / T, "%s: rows * T too large", what);
  P2PHD_REQUIRE(seg != nullptr, "%s: null pointer", what);
  int64_t at = 0, most = 0;
  for (int64_t j = 0; j < N; ++j) {
    const int64_t addr = table[4 * j], L = table[4 * j + 1], S = table[4 * j + 2], row0 = table[4 * j + 3];
    P2PHD_REQUIRE(L >= 0 && S >= 1, "%s: row %lld needs L >= 0 and S >= 1 (L %lld, S %lld)", what, (long long)j, (long long)L, (long long)S);
    P2PHD_REQUIRE(row0 == at && S <= rows - at, "%s: row %lld starts at segment row %lld with %lld of them, expected a start at %lld and an end within %lld",
                  what, (long long)j, (long long)row0, (long long)S, (long long)at, (long long)rows);
    P2PHD_REQUIRE(addr != 0 || L == 0, "%s: row %lld has a null address and L %lld", what, (long long)j, (long long)L);
    P2PHD_REQUIRE((addr & 3) == 0, "%s: row %lld's address is not a float's", what, (long long)j);
    if (stitch)
      P2PHD_REQUIRE(L <= (S - 1) * stride + T, "%s: row %lld's L %lld is beyond the %lld samples its segments span", what, (long long)j, (long long)L,
                    (long long)((S - 1) * stride + T));
    at += S;
    most = std::max(most, stitch ? L : S * T);
  }
  P2PHD_REQUIRE(at == rows, "%s: the rows close at segment row %lld, not at %lld", what, (long long)at, (long long)rows);
  *longest = most;
  return P2PHD_OK;
}

// The checked table -> a pinned slot -> table_dev, on `stream`.  Nothing is waited for (but see above).
int send_table(const char* what, const int64_t* table, int64_t N, void* table_dev, hipStream_t stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  P2PHD_REQUIRE(hipStreamIsCapturing(stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone,
                "%s: not inside a stream capture (a replay would read a table slot that has been reused since)", what);
  const size_t bytes = (size_t)N * 4 * sizeof(int64_t);
  int dev = 0;
  std::lock_guard<std::mutex> lock(g_table_mutex);
  TableSlot& s = g_table_slots[g_table_next];
  g_table_next = (g_table_next + 1) % kTableSlots;
  bool ok = hipGetDevice(&dev) == hipSuccess;
  if (ok && s.pending) { ok = hipEventSynchronize(s.ev) == hipSuccess; s.pending = false; }
  if (ok && s.ev != nullptr && s.dev != dev) { (void)hipEventDestroy(s.ev); s.ev = nullptr; }
  if (ok && s.ev == nullptr) { ok = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) == hipSuccess; s.dev = dev; if (!ok) s.ev = nullptr; }
  if (ok && s.cap < bytes) {
    if (s.host != nullptr) (void)hipHostFree(s.host);
    s.host = nullptr; s.cap = 0;
    const size_t want = std::max<size_t>(bytes, 4096);
    ok = hipHostMalloc(&s.host, want, hipHostMallocDefault) == hipSuccess;
    if (ok) s.cap = want; else s.host = nullptr;
  }
  if (ok) {
    memcpy(s.host, table, bytes);
    ok = hipMemcpyAsync(table_dev, s.host, bytes, hipMemcpyHostToDevice, stream) == hipSuccess;
    if (ok) { ok = hipEventRecord(s.ev, stream) == hipSuccess; s.pending = ok; }
  }
  if (!ok) {
    (void)hipGetLastError();
    p2phd::set_error("%s: the table of %lld rows could not be sent to the device", what, (long long)N);
    return P2PHD_ELAUNCH;
  }
  return P2PHD_OK;
}

}  // namespace

extern "C" int64_t p2phd_segments_ragged_table_bytes(int64_t N) { return N >= 1 && N <= 65535 ? N * 4 * (int64_t)sizeof(int64_t) : 0; }

extern "C" int p2phd_segments_gather_ragged(const int64_t* table, int64_t N, int64_t T, int64_t stride, int64_t rows, float* seg, void* table_dev,
                                            void* stream) {
  const char* what = "segments_gather_ragged";
  int64_t longest = 0;
  if (int rc = check_table(what, table, N, rows, T, stride, false, seg, table_dev, &longest)) return rc;
  if (int rc = send_table(what, table, N, table_dev, (hipStream_t)stream)) return rc;
  const int tvec = (T & 3) == 0 && (stride & 3) == 0;
  hipLaunchKernelGGL(segments_gather_ragged_kernel, dim3(ragged_grid(longest), (unsigned)N), dim3(kThreads), 0, (hipStream_t)stream,
                     static_cast<const long*>(table_dev), (long)T, (long)stride, seg, tvec);
  ++p2phd::g_launch_count[p2phd::LC_STITCH];
  return p2phd::check_launch(what);
}

extern "C" int p2phd_segments_stitch_ragged(const float* seg, const int64_t* table, int64_t N, int64_t rows, int64_t T, int64_t stride, float gain,
                                            void* table_dev, void* stream) {
  const char* what = "segments_stitch_ragged";
  int64_t longest = 0;
  if (int rc = check_table(what, table, N, rows, T, stride, true, seg, table_dev, &longest)) return rc;
  if (longest == 0) return P2PHD_OK;                              // every clip is empty: nothing to write
  if (int rc = send_table(what, table, N, table_dev, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(segments_stitch_ragged_kernel, dim3(ragged_grid(longest), (unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, seg,
                     static_cast<const long*>(table_dev), (long)T, (long)stride, (long)(T - stride), gain);
  ++p2phd::g_launch_count[p2phd::LC_STITCH];
  return p2phd::check_launch(what);
}

extern "C" int p2phd_segments_stitch_stream(const float* seg, int64_t C, int64_t K, int64_t T, int64_t stride, float gain,
                                            const float* carry_in, float* carry_out, int first, float* out, int64_t ld, int64_t n_out,
                                            void* stream) {
  const char* what = "segments_stitch_stream";
  P2PHD_REQUIRE(K >= 1 && T >= 1, "%s: need K >= 1 and T >= 1 (K %lld, T %lld)", what, (long long)K, (long long)T);
  const int64_t V = T - stride;
  P2PHD_REQUIRE(V >= 0 && V <= T / 2, "%s: the overlap T - stride must be in [0, T/2], got %lld (T %lld)", what, (long long)V, (long long)T);
  P2PHD_REQUIRE(C >= 1 && C <= 65535, "%s: need 1 <= C <= 65535, got %lld", what, (long long)C);
  P2PHD_REQUIRE(K <= (int64_t(1) << 40) / T / C, "%s: C * K * T too large", what);
  P2PHD_REQUIRE(n_out >= 0 && n_out <= (K - 1) * stride + T, "%s: n_out %lld is beyond the %lld samples the segments span", what,
                (long long)n_out, (long long)((K - 1) * stride + T));
  P2PHD_REQUIRE(ld >= n_out, "%s: ld %lld is shorter than n_out %lld", what, (long long)ld, (long long)n_out);
  const bool head = first == 0 && V > 0;                          // the window's segment 0 has a segment in front of it to fade with
  P2PHD_REQUIRE(!head || carry_in != nullptr, "%s: a window behind the first needs carry_in (V %lld)", what, (long long)V);
  if (carry_out != nullptr && V > 0) {
    const auto overlaps = [&](const void* p, int64_t floats) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(carry_out), b = reinterpret_cast<uintptr_t>(p);
      return p != nullptr && floats > 0 && a < b + (uintptr_t)floats * 4 && b < a + (uintptr_t)(C * V) * 4;
    };
    P2PHD_REQUIRE(!overlaps(carry_in, C * V) && !overlaps(seg, C * K * T) && !overlaps(out, n_out > 0 ? (C - 1) * ld + n_out : 0),
                  "%s: carry_out overlaps carry_in, seg or out (two carry buffers take turns)", what);
  }
  if (n_out == 0) return P2PHD_OK;
  P2PHD_REQUIRE(seg && out, "%s: null pointer", what);
  const int grid = p2phd::stream_grid_of(p2phd::SG_STITCH_STREAM, P2PHD_F32, n_out, 1).used;     // (streamgrid.h)
  hipLaunchKernelGGL(segments_stitch_stream_kernel, dim3(grid, (unsigned)C), dim3(kThreads), 0, (hipStream_t)stream, seg, (long)K, (long)T,
                     (long)stride, (long)V, gain, head ? carry_in : static_cast<const float*>(nullptr), V > 0 ? carry_out : static_cast<float*>(nullptr),
                     out, (long)ld, (long)n_out);
  ++p2phd::g_launch_count[p2phd::LC_STITCH];
  return p2phd::check_launch(what);
}

extern "C" int p2phd_segments_gather(const float* audio, int64_t L, int64_t T, int64_t stride, int64_t S, float* out, void* stream) {
  return gather_rows("segments_gather", audio, 1, L, L, T, stride, S, out, stream);
}

extern "C" int p2phd_segments_stitch(const float* seg, int64_t S, int64_t T, int64_t stride, float gain, float* out, int64_t L_out,
                                     void* stream) {
  return stitch_rows("segments_stitch", seg, 1, S, T, stride, gain, out, L_out, L_out, stream);
}

extern "C" int p2phd_segments_gather_planar(const float* audio, int64_t C, int64_t ld, int64_t L, int64_t T, int64_t stride, int64_t S,
                                            float* out, void* stream) {
  return gather_rows("segments_gather_planar", audio, C, ld, L, T, stride, S, out, stream);
}

extern "C" int p2phd_segments_stitch_planar(const float* seg, int64_t C, int64_t S, int64_t T, int64_t stride, float gain, float* out,
                                            int64_t ld, int64_t L_out, void* stream) {
  return stitch_rows("segments_stitch_planar", seg, C, S, T, stride, gain, out, ld, L_out, stream);
}
