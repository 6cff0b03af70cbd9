// Weight packs of the convolution family: master f32 tensor -> the packed matrix a gather-GEMM (gconv.hip) reads, and the inverse for
// the slabs the weight gradient (wgrad.hip) leaves.  One kernel per index map that is worth its own access pattern; the `*_map`
// predicates say which map a launch has, the launchers at the end pick by them.
#include "common.h"
#include "convplan.h"
#include "convdev.h"

namespace {

using p2phd::GDesc;

// ------------------------------------------------------------------------------------------------------
// weight packing: master f32 tensor (generic strides) -> Wp[rows_pad][KK] of T, zero padded
// and the inverse for gradients (packed f32 -> master layout, overwrite)
// ------------------------------------------------------------------------------------------------------
// One thread owns one (packed row, channel) pair and walks the taps with counters: its master-tensor reads are the
// contiguous R*S block of that pair (consecutive lanes = consecutive channels, so a wave covers one contiguous span), its
// packed writes are channel-contiguous per tap.  No integer division per element; block = 64 channels x 4 rows.
template <typename T>
__global__ __launch_bounds__(256) void pack_kernel(GDesc d, p2phd::WMap m, const float* __restrict__ w, T* __restrict__ wp,
                                                   int rows_pad) {
  const int row = blockIdx.y * 4 + threadIdx.y;
  if (row >= rows_pad) return;
  const int T_taps = d.nth * d.ntw, Cp = d.Cp_in, KK = d.KK, ntw = d.ntw;
  T* orow = wp + (size_t)row * KK;
  const bool row_ok = row < m.rows;
  const long roff = row_ok ? (long)(row % m.row_mod) * m.s_row + (long)(row / m.row_mod) * m.s_rowq : 0;
  for (int c = blockIdx.x * 64 + threadIdx.x; c < Cp; c += gridDim.x * 64) {
    const bool ok = row_ok && c < m.inner;
    const float* src = w + roff + (ok ? (long)(c % m.c_mod) * m.s_inner + (long)(c / m.c_mod) * m.s_innerq : 0);
    int ta = 0, tb = 0;
    for (int t0 = 0; t0 < T_taps; t0 += 16) {                   // 16 independent (clamped, unconditional) loads in flight
      float v[16];
      int ta2 = ta, tb2 = tb;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        v[i] = src[((d.wr0 + ta2 * d.wr_step) * m.S + d.ws0 + tb2 * d.ws_step) * m.s_tap];
        if (t0 + i + 1 < T_taps && ++tb2 == ntw) { tb2 = 0; ++ta2; }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (t0 + i < T_taps) orow[(t0 + i) * Cp + c] = from_f<T>(ok ? v[i] : 0.f);
      ta = ta2; tb = tb2;                                       // = tap t0 + 16 when there is another batch
    }
  }
  // zero tail of the padded K extent
  for (int kk = T_taps * Cp + blockIdx.x * 64 + threadIdx.x; kk < KK; kk += gridDim.x * 64) orow[kk] = from_f<T>(0.f);
}

// Dense variants for the common case "every tap of a plain [rows][inner][R][S] master tensor, in order" (all stride-1
// forward packs and weight gradients, i.e. almost all of the parameter bytes): the R*S values of a (row, channel) pair
// and of its 63 neighbours form ONE contiguous run of the master tensor, which is moved with coalesced accesses and
// re-ordered to / from the tap-major packed layout through a small LDS tile (T_taps is coprime to the bank count or small,
// so the strided side of the tile costs at most a few-way conflict on 16 KiB).
template <typename T>
__global__ __launch_bounds__(256) void pack_dense_kernel(GDesc d, p2phd::WMap m, const float* __restrict__ w, T* __restrict__ wp,
                                                         int rows_pad) {
  __shared__ float tile[4][64 * 16];
  const int T_taps = d.nth * d.ntw, Cp = d.Cp_in, KK = d.KK;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int row = blockIdx.y * 4 + ty, c0 = blockIdx.x * 64;
  const bool row_ok = row < m.rows;
  const int ncols = max(0, min(64, m.inner - c0));
  if (row_ok) {
    const float* src = w + (long)row * m.s_row + (long)c0 * T_taps;
    for (int i = tx; i < ncols * T_taps; i += 64) tile[ty][i] = src[i];
  }
  __syncthreads();
  if (row < rows_pad) {
    T* orow = wp + (size_t)row * KK;
    const int c = c0 + tx;
    if (c < Cp) {
      const bool ok = row_ok && tx < ncols;
      for (int t = 0; t < T_taps; ++t) orow[t * Cp + c] = from_f<T>(ok ? tile[ty][tx * T_taps + t] : 0.f);
    }
    if (blockIdx.x == 0)
      for (int kk = T_taps * Cp + tx; kk < KK; kk += 64) orow[kk] = from_f<T>(0.f);
  }
}

// TT = compile-time tap count (9: 3x3, 16: 4x4) so that exactly TT loads per slab are issued; 0 = any count <= 16
// (loads clamped to the last tap: up to 16 issued)
template <int TT>
__global__ __launch_bounds__(256) void unpack_dense_kernel(GDesc d, p2phd::WMap m, const float* __restrict__ dwp,
                                                           float* __restrict__ dw, int splits, long slab_elems, int accumulate) {
  __shared__ float tile[4][64 * 16];
  const int T_taps = TT > 0 ? TT : d.nth * d.ntw, Cp = d.Cp_in;
  constexpr int NV = TT > 0 ? TT : 16;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int row = blockIdx.y * 4 + ty, c0 = blockIdx.x * 64;
  const bool row_ok = row < m.rows;
  const int ncols = max(0, min(64, m.inner - c0));
  if (row_ok && tx < ncols) {
    float v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.f;
    const float* srow = dwp + (size_t)row * d.KK + c0 + tx;
    for (int z = 0; z < splits; ++z) {                           // fixed order: reproducible
      const float* src = srow + (size_t)z * slab_elems;
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] += src[(size_t)min(i, T_taps - 1) * Cp];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (i < T_taps) tile[ty][tx * T_taps + i] = v[i];
  }
  __syncthreads();
  if (row_ok) {
    float* dst = dw + (long)row * m.s_row + (long)c0 * T_taps;
    for (int i = tx; i < ncols * T_taps; i += 64) dst[i] = accumulate ? dst[i] + tile[ty][i] : tile[ty][i];
  }
}

// Transposing variant for master tensors laid out [inner][rows][R*S] (the input-gradient pack of a Conv2d: packed rows =
// input channels, packed inner = output channels): a block moves a 64 (inner) x 16 (rows) x R*S brick through LDS, so
// both the master reads (R*S * 16 contiguous floats per inner index) and the packed writes (64 consecutive inner
// indices) are coalesced; the generic kernel reads this case with one cache line per lane.
template <typename T>
__global__ __launch_bounds__(256) void pack_transposed_kernel(GDesc d, p2phd::WMap m, const float* __restrict__ w, T* __restrict__ wp,
                                                              int rows_pad) {
  constexpr int RB = 16;
  __shared__ float tile[64][RB * 16 + 1];
  __shared__ int tapidx[16];
  const int T_taps = d.nth * d.ntw, Cp = d.Cp_in, KK = d.KK, RS = (int)m.s_row;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int k0 = blockIdx.x * 64, row0 = blockIdx.y * RB;
  if (ty == 0 && tx < T_taps) {
    const int ta = tx / d.ntw, tb = tx - ta * d.ntw;
    tapidx[tx] = (d.wr0 + ta * d.wr_step) * m.S + d.ws0 + tb * d.ws_step;
  }
  const int nrows = max(0, min(RB, m.rows - row0));
  // 4 x 4 unconditional (clamped) loads in flight per thread and pass: a load inside a data-dependent branch is
  // serialised by its own s_waitcnt
  const int run = nrows * RS;                                    // contiguous floats per inner index (<= 256)
#pragma unroll
  for (int kb = 0; kb < (run > 0 ? 64 : 0); kb += 16) {          // run == 0: a block of padding rows reads nothing
    float v[4][4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = kb + 4 * kk + ty;
      const float* src = w + (long)min(k0 + k, m.inner - 1) * m.s_inner + (long)row0 * RS;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[kk][q] = src[min(tx + 64 * q, max(run - 1, 0))];
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = kb + 4 * kk + ty;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (tx + 64 * q < run) tile[k][tx + 64 * q] = v[kk][q];
    }
  }
  __syncthreads();
  const bool k_ok = k0 + tx < m.inner;
  if (k0 + tx < Cp) {
    for (int r = ty; r < RB; r += 4) {
      const int row = row0 + r;
      if (row >= rows_pad) break;
      T* orow = wp + (size_t)row * KK + k0 + tx;
      const bool ok = k_ok && r < nrows;
      for (int t = 0; t < T_taps; ++t) orow[(size_t)t * Cp] = from_f<T>(ok ? tile[tx][r * RS + tapidx[t]] : 0.f);
    }
  }
  if (blockIdx.x == 0) {                                          // zero tail of the padded K extent
    for (int r = ty; r < RB; r += 4) {
      const int row = row0 + r;
      if (row >= rows_pad) break;
      for (int kk = T_taps * Cp + tx; kk < KK; kk += 64) wp[(size_t)row * KK + kk] = from_f<T>(0.f);
    }
  }
}

inline bool transposed_map(const GDesc& d, const p2phd::WMap& m) {
  const int T_taps = d.nth * d.ntw;
  if (!(T_taps <= 16 && m.s_tap == 1 && m.s_row >= 1 && m.s_row <= 16 && m.c_mod >= m.inner && m.row_mod >= m.rows && m.inner > 0 && m.rows > 0 &&
        m.s_inner >= (long)m.rows * m.s_row))
    return false;
  for (int t = 0; t < T_taps; ++t) {                             // every tap must address inside the R*S block
    const int ta = t / d.ntw, tb = t - ta * d.ntw;
    const int idx = (d.wr0 + ta * d.wr_step) * m.S + d.ws0 + tb * d.ws_step;
    if (idx < 0 || idx >= m.s_row) return false;
  }
  return true;
}

inline bool dense_map(const GDesc& d, const p2phd::WMap& m) {
  const int T_taps = d.nth * d.ntw;
  return T_taps <= 16 && m.s_tap == 1 && m.c_mod >= m.inner && m.row_mod >= m.rows && m.s_inner == T_taps && d.wr0 == 0 && d.wr_step == 1 &&
         d.ws0 == 0 && d.ws_step == 1 && d.ntw == m.S && m.inner > 0 && m.rows > 0;
}

// ---- K-major master weights [rows = K][tap][inner = C] (p2phd_conv_desc::w_layout = 1) ------------------------------------------
// forward pack / weight gradient: the packed row [tap][Cp] is the master row (Cp == C, taps in order)
inline bool kmajor_dense_map(const GDesc& d, const p2phd::WMap& m) {
  const int T_taps = d.nth * d.ntw;
  return m.s_inner == 1 && m.s_tap == m.inner && m.s_row == (long)T_taps * m.inner && d.Cp_in == m.inner && m.c_mod >= m.inner &&
         m.row_mod >= m.rows && d.wr0 == 0 && d.wr_step == 1 && d.ws0 == 0 && d.ws_step == 1 && d.ntw == m.S && m.inner > 0 && m.rows > 0;
}
// input-gradient pack: packed rows = C (master inner index), packed inner = K (master rows): a transpose per tap
inline bool kmajor_transposed_map(const GDesc& d, const p2phd::WMap& m) {
  const int T_taps = d.nth * d.ntw;
  return T_taps <= 16 && m.s_row == 1 && m.s_tap == m.rows && m.s_inner == (long)T_taps * m.rows && m.c_mod >= m.inner &&
         m.row_mod >= m.rows && d.ntw * d.nth == T_taps && m.inner > 0 && m.rows > 0;
}

// wp[row][kk] = T(w[row][kk]) for kk < T_taps * C, zero in the K tail and in the padding rows: a cast, float4 in / 8 or 16 bytes out
template <typename T>
__global__ __launch_bounds__(256) void pack_kmajor_dense_kernel(const float* __restrict__ w, T* __restrict__ wp, int rows, int rows_pad,
                                                                int row_len, int KK) {
  const long total4 = (long)rows_pad * (KK / 4);
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
    const int row = (int)(e / (KK / 4)), k4 = (int)(e - (long)row * (KK / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows && k4 < row_len) v = *reinterpret_cast<const float4*>(w + (size_t)row * row_len + k4);    // row_len % 8 == 0
    T* o = wp + (size_t)row * KK + k4;
    if constexpr (sizeof(T) == 2) {
      bf16x4 b = {(bf16_t)v.x, (bf16_t)v.y, (bf16_t)v.z, (bf16_t)v.w};
      *reinterpret_cast<bf16x4*>(o) = b;
    } else {
      *reinterpret_cast<float4*>(o) = v;
    }
  }
}

// wp[c][t'][k] = T(w[k][tap(t')][c]): per packed tap a 64 (k) x 64 (c) tile through LDS.  Round 5: 16-byte accesses on both sides --
// the tile's rows are read as float4 runs along c (one 256-byte master row per 16 lanes), and every thread writes whole 16-byte
// pieces of eight consecutive k of one packed row (the first version moved 4 bytes in and 2 bytes out per lane and instruction:
// 13.5 us for 32 MB on the trunk layer).  Callers guarantee K-major shapes (kmajor_transposed_map: C and K multiples of 64 here,
// so a tile is whole unless it hangs over rows_pad / Cp, which the scalar tail below handles).
template <typename T>
__global__ __launch_bounds__(256) void pack_kmajor_transposed_kernel(GDesc d, p2phd::WMap m, const float* __restrict__ w, T* __restrict__ wp,
                                                                     int rows_pad) {
  __shared__ float tile[64][65];
  const int T_taps = d.nth * d.ntw, Cp = d.Cp_in, KK = d.KK;
  const int tid = threadIdx.y * 64 + threadIdx.x;                // (64, 4) threads
  const int k0 = blockIdx.x * 64, c0 = blockIdx.y * 64, tp = blockIdx.z;
  const int ta = tp / d.ntw, tb = tp - ta * d.ntw;
  const long tap = ((long)(d.wr0 + ta * d.wr_step) * m.S + d.ws0 + tb * d.ws_step) * m.s_tap;   // master offset of this packed tap
  // master element (k, c): w[k * s_inner + tap + c]   (m.rows = C, m.inner = K)
  const bool whole = k0 + 64 <= m.inner && c0 + 64 <= m.rows && c0 + 64 <= rows_pad && k0 + 64 <= Cp &&
                     ((m.s_inner | tap | (long)c0) & 3) == 0 && ((uintptr_t)w & 15) == 0;
  if (whole) {
    const int c4 = (tid & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kr = (tid >> 4) + 16 * i;
      const float4 v = *reinterpret_cast<const float4*>(w + (size_t)(k0 + kr) * m.s_inner + tap + c0 + c4);
      tile[kr][c4] = v.x; tile[kr][c4 + 1] = v.y; tile[kr][c4 + 2] = v.z; tile[kr][c4 + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int kr = threadIdx.y + 4 * i, k = k0 + kr, c = c0 + (int)threadIdx.x;
      tile[kr][threadIdx.x] = (k < m.inner && c < m.rows) ? w[(size_t)k * m.s_inner + tap + c] : 0.f;
    }
  }
  __syncthreads();
  constexpr int EP = 16 / (int)sizeof(T);                        // elements per 16-byte piece (8 for the 16-bit types, 4 for f32)
  constexpr int PPR = 64 / EP;                                   // pieces per packed row of the tile
  if (whole) {
    for (int q = tid; q < 64 * PPR; q += 256) {
      const int cr = q / PPR, kp = (q - cr * PPR) * EP;           // packed row c0 + cr, k = k0 + kp .. + EP - 1
      T v[EP];
#pragma unroll
      for (int e = 0; e < EP; ++e) v[e] = from_f<T>(tile[kp + e][cr]);
      *reinterpret_cast<uint4*>(wp + (size_t)(c0 + cr) * KK + (size_t)tp * Cp + k0 + kp) = *reinterpret_cast<const uint4*>(v);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = c0 + threadIdx.y + 4 * i, k = k0 + (int)threadIdx.x;
      if (c < rows_pad && k < Cp) wp[(size_t)c * KK + (size_t)tp * Cp + k] = from_f<T>(tile[threadIdx.x][threadIdx.y + 4 * i]);
    }
  }
  if (blockIdx.x == 0 && tp == 0) {                                // zero tail of the padded K extent of these 64 rows
    for (int r = threadIdx.y; r < 64; r += 4) {
      const int c = c0 + r;
      if (c >= rows_pad) break;
      for (int kk = T_taps * Cp + threadIdx.x; kk < KK; kk += 64) wp[(size_t)c * KK + kk] = from_f<T>(0.f);
    }
  }
}

// dw[row][kk] (+)= sum_z slab[z][row][kk], kk < T_taps * C: the weight gradient of a K-major layer lands with whole rows
__global__ __launch_bounds__(256) void unpack_kmajor_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int rows, int row_len,
                                                            int KK, int splits, long slab_elems, int accumulate) {
  const int r4 = row_len / 4;
  const long total4 = (long)rows * r4;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total4; e += (long)gridDim.x * 256) {
    const int row = (int)(e / r4), k4 = (int)(e - (long)row * r4) * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int z = 0; z < splits; ++z) {                           // fixed order: reproducible
      const float4 v = *reinterpret_cast<const float4*>(dwp + (size_t)z * slab_elems + (size_t)row * KK + k4);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    float4* o = reinterpret_cast<float4*>(dw + (size_t)row * row_len + k4);
    if (accumulate) { const float4 p = *o; a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w; }
    *o = a;
  }
}

// Packed weights of a merged sub-pixel launch (stride 2, transposed form):
//   Wp[(cls, k)][(dh, dw)][c] = w(k, c, r, s)  with  r = pi + pad - 2 dh,  s = pj + pad - 2 dw  (0 when outside the kernel)
template <typename T>
__global__ void pack_merged_kernel(GDesc d, const float* __restrict__ w, T* __restrict__ wp, int rows_pad, int K, int C, int R, int S,
                                   int pad, long s_k, long s_c) {
  const long total = (long)rows_pad * d.KK;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int row = (int)(e / d.KK);
    const int kk = (int)(e - (long)row * d.KK);
    const int t = kk / d.Cp_in, c = kk - t * d.Cp_in;
    float v = 0.f;
    if (row < 4 * d.cls_cp && t < d.nth * d.ntw && c < C) {
      const int cls = row / d.cls_cp, k = row - cls * d.cls_cp;
      const int pi = cls >> 1, pj = cls & 1;
      const int tt = d.cls_skip && pi == 1 ? ((t & 1) << 1 | (t >> 1)) : t;    // K position -> tap (GDesc::cls_skip)
      const int ta = tt / d.ntw, tb = tt - ta * d.ntw;
      const int dh = d.dh0 + ta * d.dh_step, dw = d.dw0 + tb * d.dw_step;
      const int r = pi + pad - 2 * dh, s2 = pj + pad - 2 * dw;
      if (k < K && r >= 0 && r < R && s2 >= 0 && s2 < S) v = w[k * s_k + c * s_c + r * S + s2];
    }
    wp[e] = from_f<T>(v);
  }
}

__global__ __launch_bounds__(256) void unpack_grad_kernel(GDesc d, p2phd::WMap m, const float* __restrict__ dwp,
                                                          float* __restrict__ dw, int splits, long slab_elems, int accumulate) {
  // same ownership as pack_kernel: thread = (row, channel), taps walked with counters; the split slabs are summed in
  // a fixed order (reproducible), reads are channel-contiguous, the R*S results of a pair land in one contiguous block
  const int row = blockIdx.y * 4 + threadIdx.y;
  if (row >= m.rows) return;
  const int T_taps = d.nth * d.ntw, Cp = d.Cp_in, ntw = d.ntw;
  const float* srow = dwp + (size_t)row * d.KK;
  const long roff = (long)(row % m.row_mod) * m.s_row + (long)(row / m.row_mod) * m.s_rowq;
  for (int c = blockIdx.x * 64 + threadIdx.x; c < m.inner; c += gridDim.x * 64) {
    float* dst = dw + roff + (long)(c % m.c_mod) * m.s_inner + (long)(c / m.c_mod) * m.s_innerq;
    int ta = 0, tb = 0;
    for (int t0 = 0; t0 < T_taps; t0 += 16) {                   // 16 taps at a time: that many independent loads in flight
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = 0.f;
      for (int z = 0; z < splits; ++z) {
        const float* src = srow + (size_t)z * slab_elems + c;
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] += src[(size_t)min(t0 + i, T_taps - 1) * Cp];      // unconditional, clamped
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (t0 + i < T_taps) {
          float* o = dst + ((d.wr0 + ta * d.wr_step) * m.S + d.ws0 + tb * d.ws_step) * m.s_tap;
          *o = accumulate ? *o + v[i] : v[i];
          if (++tb == ntw) { tb = 0; ++ta; }
        }
      }
    }
  }
}

// ---- fp8 (OCP e4m3) weight pack of a dense direct plan: wp8[row][tap][Cp] = e4m3(w * 448 / amax), scale = amax / 448 ----
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ w, long n, unsigned* __restrict__ amax_bits) {
  // float4 pieces, four in flight per thread (n is a multiple of 4 and w 16-byte aligned: flat Adam buffer slices)
  float m = 0.f;
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  const float4* w4 = reinterpret_cast<const float4*>(w);
  for (long e0 = (long)blockIdx.x * 256 + threadIdx.x; e0 < n4; e0 += 4 * stride) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = w4[min(e0 + u * stride, n4 - 1)];
#pragma unroll
    for (int u = 0; u < 4; ++u) m = fmaxf(m, fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
  }
  for (long e = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) m = fmaxf(m, fabsf(w[e]));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(amax_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));   // non-negative floats order like their bits
}
__global__ void fp8_scale_kernel(const unsigned* __restrict__ amax_bits, float* __restrict__ scale2) {
  const float a = fmaxf(__uint_as_float(*amax_bits), 1e-30f);
  scale2[0] = a / 448.f;                                                      // de-quantisation factor (read by the conv epilogue)
  scale2[1] = 448.f / a;
}
__global__ __launch_bounds__(256) void pack_fp8_kernel(GDesc d, p2phd::WMap m, const float* __restrict__ w, unsigned char* __restrict__ wp,
                                                       int rows_pad, const float* __restrict__ scale2) {
  // thread = (row, 4 consecutive channels): reads their 4 x T_taps master values (one contiguous run, consecutive threads
  // continue it), writes one packed dword per tap (consecutive threads -> consecutive dwords of the [tap][channel] row)
  const int T_taps = d.nth * d.ntw, Cp = d.Cp_in, KK = d.KK;
  const float q = scale2[1];
  const int c4n = Cp / 4;
  const long total = (long)rows_pad * c4n;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int row = (int)(e / c4n), c = (int)(e - (long)row * c4n) * 4;
    const bool row_ok = row < m.rows;
    // element (row, channel cc, tap t) of the master tensor: PyTorch layout s_inner = T_taps, s_tap = 1; K-major s_inner = 1, s_tap = C
    const float* src = w + (row_ok ? (long)row * m.s_row : 0) + (long)min(c, max(m.inner - 4, 0)) * m.s_inner;
    for (int t0 = 0; t0 < T_taps; t0 += 4) {
      float v[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) v[i][u] = src[i * m.s_inner + (long)min(t0 + u, T_taps - 1) * m.s_tap];   // unconditional, clamped
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (t0 + u >= T_taps) break;
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = (row_ok && c + i < m.inner) ? v[i][u] * q : 0.f;
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], pk, true);
        *reinterpret_cast<int*>(wp + (size_t)row * KK + (size_t)(t0 + u) * Cp + c) = pk;
      }
    }
  }
}

}  // namespace

namespace p2phd {

// dw (+)= the `splits` packed slabs of a weight gradient (dwp, slab_elems floats apart), summed in slab order, in the master layout
void launch_unpack_grad(const GDesc& d, const WMap& m, const float* dwp, float* dw, int splits, long slab_elems, int accumulate,
                        hipStream_t st) {
  if (kmajor_dense_map(d, m)) {
    const int row_len = d.nth * d.ntw * m.inner;
    const long total4 = (long)m.rows * (row_len / 4);
    hipLaunchKernelGGL(unpack_kmajor_kernel, dim3((unsigned)std::min<long>((total4 + 255) / 256, 8192)), dim3(256), 0, st, dwp, dw, m.rows,
                       row_len, d.KK, splits, slab_elems, accumulate);
  } else if (dense_map(d, m)) {
    const dim3 grid((unsigned)((m.inner + 63) / 64), (unsigned)((m.rows + 3) / 4));
    const int tt = d.nth * d.ntw;
    if (tt == 9) hipLaunchKernelGGL(unpack_dense_kernel<9>, grid, dim3(64, 4), 0, st, d, m, dwp, dw, splits, slab_elems, accumulate);
    else if (tt == 16) hipLaunchKernelGGL(unpack_dense_kernel<16>, grid, dim3(64, 4), 0, st, d, m, dwp, dw, splits, slab_elems, accumulate);
    else hipLaunchKernelGGL(unpack_dense_kernel<0>, grid, dim3(64, 4), 0, st, d, m, dwp, dw, splits, slab_elems, accumulate);
  } else {
    const dim3 grid((unsigned)std::min((m.inner + 63) / 64, 64), (unsigned)((m.rows + 3) / 4));
    hipLaunchKernelGGL(unpack_grad_kernel, grid, dim3(64, 4), 0, st, d, m, dwp, dw, splits, slab_elems, accumulate);
  }
}

int launch_pack_merged(const GDesc& d, int dtype, const float* w, void* wp, int rows_pad, int K, int C, int R, int S, int pad,
                       long s_k, long s_c, hipStream_t st) {
  const long total = (long)rows_pad * d.KK;
  const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
  ++g_launch_count[LC_WPACK_MERGED];
  FOR_ELEM(dtype, T, hipLaunchKernelGGL(pack_merged_kernel<T>, dim3(blocks), dim3(256), 0, st, d, w, (T*)wp, rows_pad, K, C, R, S, pad, s_k, s_c));
  return check_launch("pack_weights(merged)");
}

int launch_pack(const GDesc& d, const WMap& m, int dtype, const float* w, void* wp, int rows_pad, hipStream_t st) {
  if (rows_pad <= 0) return P2PHD_OK;
  if (kmajor_dense_map(d, m) && d.KK % 4 == 0) {
    const int row_len = d.nth * d.ntw * m.inner;
    const long total4 = (long)rows_pad * (d.KK / 4);
    const dim3 grid((unsigned)std::min<long>((total4 + 255) / 256, 8192));
    ++g_launch_count[LC_WPACK_KMAJOR];
    FOR_ELEM(dtype, T, hipLaunchKernelGGL(pack_kmajor_dense_kernel<T>, grid, dim3(256), 0, st, w, (T*)wp, m.rows, rows_pad, row_len, d.KK));
    return check_launch("pack_weights(k-major)");
  }
  if (kmajor_transposed_map(d, m)) {
    const dim3 grid((unsigned)((std::max(m.inner, d.Cp_in) + 63) / 64), (unsigned)((rows_pad + 63) / 64), (unsigned)(d.nth * d.ntw));
    ++g_launch_count[LC_WPACK_KMAJOR_T];
    FOR_ELEM(dtype, T, hipLaunchKernelGGL(pack_kmajor_transposed_kernel<T>, grid, dim3(64, 4), 0, st, d, m, w, (T*)wp, rows_pad));
    return check_launch("pack_weights(k-major transposed)");
  }
  if (dense_map(d, m)) {
    const dim3 dgrid((unsigned)((d.Cp_in + 63) / 64), (unsigned)((rows_pad + 3) / 4));
    ++g_launch_count[LC_WPACK_DENSE];
    FOR_ELEM(dtype, T, hipLaunchKernelGGL(pack_dense_kernel<T>, dgrid, dim3(64, 4), 0, st, d, m, w, (T*)wp, rows_pad));
    return check_launch("pack_weights(dense)");
  }
  if (transposed_map(d, m)) {
    const dim3 tgrid((unsigned)((d.Cp_in + 63) / 64), (unsigned)((rows_pad + 15) / 16));
    ++g_launch_count[LC_WPACK_TRANSPOSED];
    FOR_ELEM(dtype, T, hipLaunchKernelGGL(pack_transposed_kernel<T>, tgrid, dim3(64, 4), 0, st, d, m, w, (T*)wp, rows_pad));
    return check_launch("pack_weights(transposed)");
  }
  const dim3 grid((unsigned)std::min((d.Cp_in + 63) / 64, 64), (unsigned)((rows_pad + 3) / 4));
  ++g_launch_count[LC_WPACK_GENERIC];
  FOR_ELEM(dtype, T, hipLaunchKernelGGL(pack_kernel<T>, grid, dim3(64, 4), 0, st, d, m, w, (T*)wp, rows_pad));
  return check_launch("pack_weights");
}

int launch_pack_fp8(const GDesc& d, const WMap& m, const float* w, void* wp8, int rows_pad, float* scale2, unsigned* amax_bits,
                    hipStream_t st) {
  (void)hipMemsetAsync(amax_bits, 0, sizeof(unsigned), st);
  ++g_launch_count[LC_WPACK_FP8];                                  // the quantiser with its amax and scale kernels: one family
  const long n = (long)m.rows * m.s_row;
  hipLaunchKernelGGL(amax_kernel, dim3((unsigned)std::max<long>(1, std::min<long>((n / 4 + 1023) / 1024, 2048))), dim3(256), 0, st, w, n, amax_bits);
  hipLaunchKernelGGL(fp8_scale_kernel, dim3(1), dim3(1), 0, st, amax_bits, scale2);
  const long total = (long)rows_pad * (d.Cp_in / 4);
  hipLaunchKernelGGL(pack_fp8_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 8192)), dim3(256), 0, st, d, m, w,
                     (unsigned char*)wp8, rows_pad, scale2);
  return check_launch("pack_weights(fp8)");
}

}  // namespace p2phd
