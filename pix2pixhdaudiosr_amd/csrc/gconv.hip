// Convolution family of the pix2pixHD generator / discriminator for gfx950, as implicit GEMMs on MFMA.
//
// Reference layers covered (models/networks.py): Conv2d 7x7 s1 behind ReflectionPad2d(3) (:190,207),
// Conv2d 3x3 s2 p1 (:194), Conv2d 3x3 s1 behind ReflectionPad2d(1) (:231,246), ConvTranspose2d 3x3 s2 p1
// op1 (:205), Conv2d 4x4 s2/s1 p2 (:342-361), each with forward, input gradient and weight gradient.
//
// One primitive serves all of them: a GATHER CONVOLUTION over NHWC activations
//     out[n, ho*om+oo, wo*om'+oo', k] = sum_{tap t} sum_c in[n, ho*s + dh(t), wo*s + dw(t), c] * Wp[k][t][c]
// with zero or reflect boundary handling folded into the gather index.  Forward convs, the input gradient of
// stride-1 convs and of ConvTranspose2d are single launches; ConvTranspose2d forward and the input gradient
// of stride-2 convs are run as stride^2 sub-pixel classes (each a stride-1 gather with its own tap subset and
// an interleaved output lattice), so no zero-stuffed tensor and no col2im scatter ever exists.
//
// GEMM view: M = output pixels (tiles never straddle samples), N = output channels, K = taps x channels.
// 128 x BN x (128 bytes of K) tiles; 4 wavefronts; A (gathered pixels) and B (packed weights, K-contiguous
// rows) are staged straight global -> LDS with global_load_lds_dwordx4 in 16-byte pieces (coalesced along the
// channel axis = the frequency-major NHWC inner dimension), double-buffered with the next tile's loads issued
// before the MFMAs of the current one; LDS rows are 128 B with a 16-byte-chunk XOR swizzle ((row>>1)&7), applied
// to the per-lane SOURCE address because the LDS side of a direct load is lane-linear, so the ds_read_b128
// fragment reads of v_mfma_f32_32x32x16_bf16 are bank-conflict free.  fp32 mode (parity runs) uses the exact
// v_mfma_f32_32x32x2_f32 on the same tiles.  The epilogue adds bias, leaves the per-wave (sum, M2) partials InstanceNorm
// needs in the wave's own slot of a table (merged with Chan's update by a small kernel: no float atomics), applies an
// optional activation, stages the tile in LDS and writes whole 16-byte pieces of NHWC rows.  Round 3: the launch is a 1-D
// grid over tiles whose last, almost empty round is cut along K (split-K tail, launch_gconv_cfg).
//
// This file: the gather convolution -- kernel, tile chooser, launcher.  The weight gradient is wgrad.hip, the weight packs and
// the unpack of its result wpack.hip, the small kernels around a launch (reflect expand / fold, bias gradient, sum merge) convaux.hip.
#include "common.h"
#include "convplan.h"
#include "convdev.h"
#include "waitcheck.h"
#include <cmath>
#include <utility>
#include <vector>
#include <type_traits>

namespace {

using p2phd::GDesc;
using p2phd::GconvTile;

// OCP e4m3 operands (block-scaled v_mfma_scale_f32_32x32x64_f8f6f4, unit scales): 16 per 16-byte piece; results leave as bf16
struct fp8_t { unsigned char v; };
template <> struct Elem<fp8_t> { static constexpr int EPP = 16; };
template <typename T> struct OutOf { typedef T type; };
template <> struct OutOf<fp8_t> { typedef bf16_t type; };

// ------------------------------------------------------------------------------------------------------
// gather convolution
// ------------------------------------------------------------------------------------------------------
#ifdef P2PHD_PROBE
// experiment builds only (tools/ablate_gconv.sh): per-wave cycle totals of the main loop's wait / barrier / compute parts
constexpr int kProbeSlots = 65536;
__device__ unsigned long long g_probe[kProbeSlots * 8];   // one record per workgroup (wave 0): no atomics in the timed path
#endif

template <typename T, int BM, int BN, int MR, int NR, int NSTAGE, int HALO = 0>
__global__ __launch_bounds__((BM / (MR * 32)) * (BN / (NR * 32)) * 64) void gconv_kernel(const GDesc d, const T* __restrict__ in, const T* __restrict__ wp,
                                                    const float* __restrict__ bias,
                                                    const typename OutOf<T>::type* __restrict__ addend,
                                                    typename OutOf<T>::type* __restrict__ out, float* __restrict__ stats) {
  typedef typename OutOf<T>::type TO;                          // output element (fp8 operands produce bf16)
  constexpr int EPPO = Elem<TO>::EPP;
  constexpr int EPP = Elem<T>::EPP;
  constexpr int BK = 8 * EPP;
  constexpr int WGM = BM / (MR * 32), WGN = BN / (NR * 32);
  constexpr int NT = WGM * WGN * 64;                          // threads: one wave per (MR*32) x (NR*32) sub-tile
  static_assert(NT == BM * 2 || NT == BM, "tile config");
  constexpr int STAGE = (BM + BN) * kRowBytes;
  constexpr int RS = NT / 8;                                  // row distance between a thread's pieces
  constexpr int NB = BN * 8 / NT;                             // B pieces per thread per step
  constexpr int NA = BM * 8 / NT;                             // A pieces per thread per step (4, or 8 with one wave per SIMD)
  static_assert(NB >= 1 && (NA == 4 || NA == 8), "piece distribution");
  constexpr int NLOADS = NA + NB;                             // direct-to-LDS loads per thread per stage

  // descriptor fields used in loops live in registers (a by-value struct that is captured by reference ends
  // up in scratch memory)
  const int Cp = d.Cp_in, KK = d.KK, Wg = d.Wg, T_taps = d.nth * d.ntw, npix = d.Hg * d.Wg;
  const int Cp_out = d.Cp_out, Kout = d.Kout, act = d.act, cls_cp = d.cls_cp, n_extent = d.n_extent, stats_slots = d.stats_slots;

  extern __shared__ float4 smem_raw[];
  char* smem = reinterpret_cast<char*>(smem_raw);
  int* tab = reinterpret_cast<int*>(smem);                    // [T_taps][BM] gathered input pixel (or -1)
  int2* rinfo = reinterpret_cast<int2*>(smem + (HALO ? 0 : ((T_taps * BM * 4 + 15) & ~15)));   // [BM] {sample or -1, ho << 16 | wo}  (HALO: no gather table)
  char* stages = reinterpret_cast<char*>(rinfo + BM);
#ifdef P2PHD_PROBE
  const unsigned long long pr_t0 = __builtin_readcyclecounter();
#endif

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  // M tiling: per sample (tiles never straddle samples; needed for the InstanceNorm sums) or, when no statistics
  // are wanted and the per-sample pixel count does not fill whole tiles, flat over all N * npix pixels
  const bool flat = d.flat_m != 0;
  const int mtiles = (npix + BM - 1) / BM;
  // 1-D launch: workgroups [0, sk_first) are whole tiles (tile = id); from sk_first on, the LAST tiles of the grid -- the
  // ones that would have run as an almost empty extra round of the 256 CUs -- are cut along K into sk_parts workgroups each
  // (workgroup sk_first + part * tail + i works on tile sk_first + i, K slabs [part * sk_steps, ...)): see launch_gconv_cfg.
  int tile_id = (int)blockIdx.x, sk_part = -1, sk_tile = 0;
  if (tile_id >= d.sk_first) {
    const int r = tile_id - d.sk_first;
    sk_part = r / d.sk_tail;
    sk_tile = r - sk_part * d.sk_tail;
    tile_id = d.sk_first + sk_tile;
  }
  const int bx = tile_id % d.grid_m;
  int by = tile_id / d.grid_m;
  if (d.cls_skip != 0) by = (d.n_extent + BN - 1) / BN - 1 - by;    // deepest tiles (class (1,1): 4 taps) first, the 1-tap class last
  const int n = flat ? 0 : bx / mtiles;
  const int p_base = flat ? bx * BM : (bx - n * mtiles) * BM;
  const int p_end = flat ? d.N * npix : npix;                 // rows >= p_end are padding
  const int n0 = by * BN;

  f32x16 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int lr = lane & 31, lh = lane >> 5;
#ifdef P2PHD_PROBE
  unsigned long long pr_t1_ = 0, pr_wait_ = 0, pr_bar_ = 0, pr_comp_ = 0;
  int nsteps_ = 0;
#ifdef P2PHD_PROBE_FINE
  unsigned long long pf_a = 0, pf_b = 0;
#endif
#endif
  if constexpr (HALO != 0) {
#include "gconv_halo.inc"
  } else {
  {  // row table (the only integer divisions of the kernel: one or two per tile row), then the gather table
    // input pixel index (or -1) per (tap, tile row): each thread walks its row's taps with counters
    const int Hin = d.Hin, Win = d.Win, sh = d.sh, sw = d.sw, ntw = d.ntw, pad_mode = d.pad_mode;
    const int dh0 = d.dh0, dhs = d.dh_step, dw0 = d.dw0, dws = d.dw_step;
    const int r = tid % BM;
    int p = p_base + r, nn = -1, ho = 0, wo = 0;
    if (p < p_end) {
      nn = n;
      if (flat) { nn = p / npix; p -= nn * npix; }
      ho = p / Wg; wo = p - ho * Wg;
    }
    if (tid < BM) rinfo[r] = make_int2(nn, (ho << 16) | wo);
    constexpr int TPR = NT / BM;                              // threads per row (2)
    int ta = 0, tb = tid / BM;
    while (tb >= ntw) { tb -= ntw; ++ta; }
    const bool swap_taps = d.cls_skip != 0 && ((n0 / cls_cp) >> 1) == 1;   // 2 x 2 taps in the K order of a pi = 1 class row
    for (int t = tid / BM; t < T_taps; t += TPR) {
      if (swap_taps) { ta = t & 1; tb = t >> 1; }
      int off = -1;
      if (nn >= 0) {
        int hi = ho * sh + dh0 + ta * dhs;
        int wi = wo * sw + dw0 + tb * dws;
        if (pad_mode == 1) { hi = reflect_idx(hi, Hin); wi = reflect_idx(wi, Win); }
        if (pad_mode == 2) {
          // adjoint of ReflectionPad2d(1) in front of a 3x3 conv, on the EXACT grid: the gathered tensor is dy extended
          // by two virtual rows / columns holding dy[0] + dy[2] and dy[H-3] + dy[H-1] (reflect_expand_kernel); output
          // row 1 reads the first through its tap -1 (where plain zero padding reads dy[2]), row H-2 the second
          // through its tap +1 (instead of dy[H-3]); everything else is the zero-padded transposed conv
          const int Hr = Hin - 2, Wr = Win - 2;
          if (ho == 1 && hi == 2) hi = Hr; else if (ho == Hr - 2 && hi == Hr - 3) hi = Hr + 1; else if (hi >= Hr) hi = -1;
          if (wo == 1 && wi == 2) wi = Wr; else if (wo == Wr - 2 && wi == Wr - 3) wi = Wr + 1; else if (wi >= Wr) wi = -1;
        }
        if (pad_mode == 3) {
          // the same adjoint with dy left as the PLAIN [N, Hin, Win] tensor: the pair-sum rows / columns sit in an extras block
          // behind it (written by the InstanceNorm backward that produced dy, norm.hip): rx_base + n * EX + entry
          const int Hr = Hin, Wr = Win;
          if (ho == 1 && hi == 2) hi = Hr; else if (ho == Hr - 2 && hi == Hr - 3) hi = Hr + 1; else if (hi >= Hr) hi = -1;
          if (wo == 1 && wi == 2) wi = Wr; else if (wo == Wr - 2 && wi == Wr - 3) wi = Wr + 1; else if (wi >= Wr) wi = -1;
          if (hi >= 0 && wi >= 0) {
            if (hi < Hr && wi < Wr) off = (nn * Hr + hi) * Wr + wi;
            else off = d.rx_base + nn * (2 * (Wr + 2) + 2 * Hr) + (hi >= Hr ? (hi - Hr) * (Wr + 2) + wi : 2 * (Wr + 2) + (wi - Wr) * Hr + hi);
          }
        } else if (hi >= 0 && hi < Hin && wi >= 0 && wi < Win) off = (nn * Hin + hi) * Win + wi;
      }
      tab[t * BM + r] = off;
      tb += TPR;
      while (tb >= ntw) { tb -= ntw; ++ta; }
    }
  }
  __syncthreads();
#ifdef P2PHD_PROBE_FINE
  pf_a = __builtin_readcyclecounter();
#endif

  // Direct global -> LDS staging (buffer_load_dwordx4 ... lds): one wave instruction fills 8 consecutive 128-byte
  // tile rows linearly (lane l -> row l>>3, slot l&7).  The bank-conflict swizzle therefore sits on the SOURCE:
  // the lane that owns slot s of row r fetches logical chunk s ^ ((r>>1)&7), and fragment reads undo it.
  // Buffer addressing keeps the per-piece address a 32-bit offset (one VALU add per piece and K step) and gives
  // zero padding for free: an out-of-image piece uses an offset beyond num_records, which loads zeros.
  constexpr unsigned kOOB = 0xFFFFFFF0u;
  constexpr int SZ = (int)sizeof(T);
  const int rbase = tid >> 3;                                 // rows rbase + RS i
  const int kchunk = (tid & 7) ^ ((rbase >> 1) & 7);          // logical 16-byte chunk of the K slab
  const int CpB = Cp * SZ;
  int nsteps_all = KK / BK;
  if (d.cls_skip != 0) {                                       // stop behind the taps of the tile's highest class
    const int cls_hi = min(3, (n0 + BN - 1) / cls_cp);
    const int ktaps = ((cls_hi >> 1) + 1) * ((cls_hi & 1) + 1);
    nsteps_all = min(nsteps_all, (ktaps * Cp + BK - 1) / BK);
  }
  const int s_begin = sk_part < 0 ? 0 : sk_part * d.sk_steps;     // first K slab of this workgroup
  const int nsteps = sk_part < 0 ? nsteps_all : min(d.sk_steps, nsteps_all - s_begin);
  int a_t, a_cB;
  {
    const long kb = (long)kchunk * EPP * SZ + (long)s_begin * kRowBytes;   // byte position of this thread's chunk in the K row
    a_t = (int)(kb / CpB);
    a_cB = (int)(kb - (long)a_t * CpB);
  }
  int cur_t = -1;
  unsigned aoffb[NA], va[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) aoffb[i] = kOOB;
  unsigned boffb[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) boffb[i] = (unsigned)(((size_t)(n0 + rbase + RS * i) * KK + kchunk * EPP) * SZ);
  const unsigned tab_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) int*)tab;
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, (int)d.in_bytes, 0x00020000);
  const auto rsB = __builtin_amdgcn_make_buffer_rsrc((void*)wp, 0, (int)d.w_bytes, 0x00020000);

  // byte offsets of this thread's four A pieces for the next K slab
  auto prepare = [&]() {
    if (a_t != cur_t) {
      cur_t = a_t;
      if (a_t < T_taps) {
        // asm: a C++ LDS read here would make hipcc drain the LDS-DMA queue (see compute)
        int ro[NA];
        const unsigned ta = tab_base + (unsigned)(a_t * BM + rbase) * 4u;
#pragma unroll
        for (int i = 0; i < NA; ++i) asm volatile("ds_read_b32 %0, %1" : "=v"(ro[i]) : "v"(ta + (unsigned)(RS * i * 4)));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NA; ++i) aoffb[i] = ro[i] >= 0 ? (unsigned)ro[i] * (unsigned)CpB : kOOB;
      } else {
#pragma unroll
        for (int i = 0; i < NA; ++i) aoffb[i] = kOOB;
      }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) va[i] = aoffb[i] == kOOB ? kOOB : aoffb[i] + (unsigned)a_cB;
    a_cB += kRowBytes;
    while (a_cB >= CpB) { a_cB -= CpB; ++a_t; }
  };
  // piece j of a tile: 0..NA-1 = A rows rbase + RS j, NA.. = B rows; tile = K-slab index (scalar offset of B)
  P2PHD_CW_DECL;
  auto issue_piece = [&](int slot, int tile, int j) {
    char* A = stages + slot * STAGE + (8 * wave) * kRowBytes;
    P2PHD_CW_ISSUE(slot);                                      // (check build: tag = the ring slot the piece fills)
    if (j < NA) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr)(A + RS * j * kRowBytes), 16, (int)va[j], 0, 0, 0);
    } else {
      char* B = A + BM * kRowBytes;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_ptr)(B + RS * (j - NA) * kRowBytes), 16, (int)boffb[j - NA],
                                               tile * kRowBytes, 0, 0);
    }
  };

  // Fragment reads are inline-asm ds_read_b128: hipcc cannot prove a C++ LDS read independent of the LDS-DMA still in
  // flight and would drain it (s_waitcnt vmcnt(0)) in front of every K step; the waits here are counted by hand.
  // byte offset inside a stage of the fragment of k-step ks: row * 128 + (((2 ks + lh) ^ ((row >> 1) & 7)) << 4)
  //   = (offset of k-step 0) ^ (ks << 5): one address register per fragment row, the k-step is an XOR at the use
  unsigned fa[MR], fb[NR];
  {
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const int row = wm * (MR * 32) + i * 32 + lr;
      fa[i] = row * kRowBytes + ((lh ^ ((row >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int row = wn * (NR * 32) + j * 32 + lr;
      fb[j] = BM * kRowBytes + row * kRowBytes + ((lh ^ ((row >> 1) & 7)) << 4);
    }
  }
  const unsigned frag_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)stages;

  // ---- main loop -------------------------------------------------------------------------------------------
  // NSTAGE-slot LDS ring; tile t lives in slot t % NSTAGE.  ONE workgroup barrier per K slab, placed in front of the
  // slab's LAST MFMA cluster (k-step 3), after the wave has (a) every fragment of the slab in registers
  // (lgkmcnt(0): its LDS reads of the slot are complete) and (b) its own LDS-DMA pieces of the NEXT tile landed
  // (counted vmcnt).  Past that barrier
  //   * the next tile is readable: its first fragments are fetched while the last cluster of this slab runs, so the
  //     matrix pipe never waits for a barrier + LDS round trip at a slab boundary;
  //   * this slab's slot is free: tile s + NSTAGE is issued into it at once (half now, half one k-step later), giving
  //     the DMA more than a full slab of MFMA work to land, even on the 2-slot ring of the 256-wide tiles.
  // The later tiles stay in flight ACROSS the barrier (raw s_barrier; __syncthreads() would drain them).
  // fragment buffers: two (ping-pong over the k-steps), or one per k-step for the e4m3 operands, whose block-scaled MFMA
  // consumes the fragments of TWO k-steps at once (see mfma_one)
  constexpr int NFB = sizeof(T) == 1 ? 4 : 2;
  uint4 af[NFB][MR], bfr[NFB][NR];
  auto read_frags = [&](unsigned so_, int ks, int buf) {
    const unsigned so = so_ + frag_base;
#pragma unroll
    for (int i = 0; i < MR; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(af[buf][i]) : "v"((fa[i] ^ (unsigned)(ks << 5)) + so));
#pragma unroll
    for (int j = 0; j < NR; ++j) asm volatile("ds_read_b128 %0, %1" : "=v"(bfr[buf][j]) : "v"((fb[j] ^ (unsigned)(ks << 5)) + so));
  };
  // One MFMA cluster (MR x NR tiles, one k-step); `h0` / `h1` are issued in the shadow of its first / second MFMA
  // (fragment reads, LDS-DMA issue), so the matrix pipe already has work when the wave turns to them.
  auto mfma_one = [&](int buf, int i, int j) {
    if constexpr (sizeof(T) == 1) {
      // (block-scaled form: see mfma8 below)
      (void)buf; (void)i; (void)j;
    } else if constexpr (sizeof(T) == 2) {
      acc[i][j] = p2phd_mfma_32x32x16(*reinterpret_cast<bf16x8*>(&af[buf][i]),
                                                          *reinterpret_cast<bf16x8*>(&bfr[buf][j]), acc[i][j]);
    } else {
      // exact f32 MFMA; any k permutation is fine as long as A and B share it
      const f32x4 a4 = *reinterpret_cast<f32x4*>(&af[buf][i]);
      const f32x4 b4 = *reinterpret_cast<f32x4*>(&bfr[buf][j]);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], b4[e], acc[i][j], 0, 0, 0);
    }
  };
  // Block-scaled MFMA of the e4m3 operands (round 3): v_mfma_scale_f32_32x32x64_f8f6f4 runs at TWICE the bf16 rate (the
  // non-scaled 32x32x16_fp8_fp8 runs AT the bf16 rate).  It takes 32 bytes of K per lane: the 16-byte fragments of two
  // consecutive k-steps side by side (any K permutation is fine as long as A and B share it).  Scales: e8m0 = 127 (1.0)
  // for every 32-element block -- the layer's scale is applied once in the epilogue, as before, so the numbers are those
  // of the non-scaled form.  A pair of k-steps (2q, 2q+1) is complete at the odd k-step, where its MR x NR MFMAs go out
  // (H1 = all of them; spreading them over both k-steps of a pair measured slower).  Position p of k-step ks:
  constexpr int NT8 = MR * NR, H1 = NT8;
  auto mfma8 = [&](int ks, int p) {
    if constexpr (sizeof(T) == 1) {
      const int idx = (ks & 1) ? p : H1 + p;
      if (p < H1 && idx < NT8) {
        const int lo = (ks & 1) ? ks - 1 : ((ks + 2) & 3), hi = lo + 1;
        const int i = idx / NR, j = idx % NR;
        typedef __attribute__((ext_vector_type(8))) int i32x8;
        const uint4 a0 = af[lo][i], a1 = af[hi][i], b0 = bfr[lo][j], b1 = bfr[hi][j];
        const i32x8 av = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
        const i32x8 bv = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc[i][j], 0, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
      }
    }
  };
  constexpr bool kScaled = sizeof(T) == 1;
  if constexpr (kScaled) {                                     // (the first slab's k-step 0 multiplies zeros)
#pragma unroll
    for (int i = 0; i < MR; ++i) af[2][i] = af[3][i] = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < NR; ++j) bfr[2][j] = bfr[3][j] = make_uint4(0, 0, 0, 0);
  }
  // the MFMAs of a cluster after its first `skip`
  auto mfma_rest = [&](int buf, int skip) {
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j)
        if (i * NR + j >= skip) mfma_one(buf, i, j);
  };

#pragma unroll
  for (int t = 0; t < NSTAGE; ++t) {
    if (t < nsteps) {
      prepare();
#pragma unroll
      for (int j = 0; j < NLOADS; ++j) issue_piece(t, s_begin + t, j);
    }
  }
#ifdef P2PHD_PROBE_FINE
  pf_b = __builtin_readcyclecounter();
#endif
  if (nsteps >= NSTAGE) {
    P2PHD_CW_WAIT(CW_GCONV, (NSTAGE - 1) * NLOADS, 1u << 0);   // slot 0 is read behind the barrier
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 1) * NLOADS) : "memory");
  } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  read_frags(0u, 0, 0);

  int cur = 0;
  bool pend = false;                              // second half of a tile's pieces still to be issued (at k-step 0)
  int pend_slot = 0, pend_tile = 0;
#ifdef P2PHD_PROBE
  unsigned long long pr_wait = 0, pr_bar = 0, pr_comp = 0;
  const unsigned long long pr_t1 = __builtin_readcyclecounter();
#endif
  for (int s = 0; s < nsteps; ++s) {
    const unsigned so = (unsigned)(cur * STAGE);
    const int nslot = cur == NSTAGE - 1 ? 0 : cur + 1;
#ifdef P2PHD_PROBE
    const unsigned long long pt0 = __builtin_readcyclecounter();
#endif
    // Each k-step: its fragments were fetched behind the previous cluster and have had that cluster's time to land.
    // The first MFMA goes out at once; the next fragment reads and the LDS-DMA issue follow in its shadow (written out
    // inline: a closure that captures the unrolled `ks` turns the fragment-address arrays into scratch).
    const bool has_next = s + 1 < nsteps;
    const bool issue_new = s + NSTAGE < nsteps;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int buf = sizeof(T) == 1 ? ks : (ks & 1);
      const int nbuf = sizeof(T) == 1 ? ((ks + 1) & 3) : (buf ^ 1);   // where the next k-step's fragments go
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (ks == 3 && has_next) {
        // slab boundary: every LDS read of this slot is complete; own pieces of the next tile must have landed
#ifdef P2PHD_PROBE
        const unsigned long long pt1 = __builtin_readcyclecounter();
#endif
        if (NSTAGE > 2 && s + NSTAGE - 1 < nsteps) {
          P2PHD_CW_WAIT(CW_GCONV, (NSTAGE - 2) * NLOADS, 1u << nslot);   // the next slab's slot is read behind the barrier
          asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 2) * NLOADS) : "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef P2PHD_PROBE
        const unsigned long long pt2 = __builtin_readcyclecounter();
        pr_wait += pt2 - pt1;
#endif
        __builtin_amdgcn_s_barrier();
#ifdef P2PHD_PROBE
        pr_bar += __builtin_readcyclecounter() - pt2;
#endif
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kScaled) mfma8(ks, 0); else mfma_one(buf, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (ks < 3) read_frags(so, ks + 1, nbuf);
      else if (has_next) read_frags((unsigned)(nslot * STAGE), 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kScaled) mfma8(ks, 1); else if constexpr (MR * NR > 1) mfma_one(buf, 1 / NR, 1 % NR);
      __builtin_amdgcn_sched_barrier(0);
      if (ks == 0 && pend) {
#pragma unroll
        for (int j = 1; j < NLOADS; j += 2) issue_piece(pend_slot, pend_tile, j);
        pend = false;
      }
      if (ks == 3 && issue_new) {
        prepare();
#pragma unroll
        for (int j = 0; j < NLOADS; j += 2) issue_piece(cur, s_begin + s + NSTAGE, j);
        pend = true; pend_slot = cur; pend_tile = s_begin + s + NSTAGE;
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (kScaled) {
#pragma unroll
        for (int p = 2; p < H1; ++p) mfma8(ks, p);
      } else {
        mfma_rest(buf, MR * NR > 1 ? 2 : 1);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#ifdef P2PHD_PROBE
    pr_comp += __builtin_readcyclecounter() - pt0;
#endif
    cur = nslot;
  }
  if constexpr (kScaled) {                                     // second half of the last slab's pair (2,3)
#pragma unroll
    for (int p = 0; p < H1; ++p) mfma8(0, p);
  }
#ifdef P2PHD_PROBE
  pr_t1_ = pr_t1; pr_wait_ = pr_wait; pr_bar_ = pr_bar; pr_comp_ = pr_comp; nsteps_ = nsteps;
#endif
  P2PHD_CW_DONE();
  }  // !HALO
#ifdef P2PHD_PROBE
  const unsigned long long pr_t2 = __builtin_readcyclecounter();
#endif
  __syncthreads();

  if (sk_part >= 0) {
    // Split tile: every part stores its raw accumulators (float4 pieces, lane-interleaved: coalesced), takes a ticket of
    // the tile, and the part that arrives LAST adds all parts in index order -- a fixed summation order whatever the
    // timing -- and carries on into the normal epilogue.  sc1 stores / loads: the parts run on different XCDs.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // partials travel as 16-byte pieces, lane-interleaved (coalesced), through buffer instructions with the sc0 sc1 cache
    // policy on BOTH sides: write-through stores, and loads that are served from memory, not from this XCD's L2 -- an
    // agent-scope acquire followed by plain loads read stale partials of the previous launch here (measured: wrong sums in
    // the tail tiles), the per-XCD L2s are not coherent with each other.  Compiler-visible builtins: the waits are its.
    constexpr int NQ = MR * NR * 4;                            // 16-byte pieces per thread
    constexpr int kSc = 0x11;                                  // aux: bit 0 = sc0, bit 4 = sc1
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    const size_t part_bytes = (size_t)BM * BN * 4;
    const auto rsP = __builtin_amdgcn_make_buffer_rsrc((void*)(d.sk_part + (size_t)sk_tile * d.sk_parts * (size_t)(BM * BN)), 0,
                                                       (int)(d.sk_parts * part_bytes), 0x00020000);
    const int lane_off = tid * 16;
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const u32x4 v = {__float_as_uint(acc[i][j][4 * q]), __float_as_uint(acc[i][j][4 * q + 1]),
                           __float_as_uint(acc[i][j][4 * q + 2]), __float_as_uint(acc[i][j][4 * q + 3])};
          __builtin_amdgcn_raw_buffer_store_b128(v, rsP, (int)(sk_part * part_bytes) + ((i * NR + j) * 4 + q) * NT * 16 + lane_off, 0, kSc);
        }
    if (!p2phd::fold_arrive_last(d.sk_ticket + sk_tile, (unsigned)d.sk_parts)) return;
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    // pieces in flight per batch: all of a part where the registers allow, 8 for the 128-accumulator tile (it spills otherwise)
    constexpr int CH = MR * NR > 6 ? 8 : NQ;
    static_assert(NQ % CH == 0, "piece batches");
    for (int pp = 0; pp < d.sk_parts; ++pp) {
#pragma unroll
      for (int q0 = 0; q0 < NQ; q0 += CH) {
        u32x4 v[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) v[q] = __builtin_amdgcn_raw_buffer_load_b128(rsP, (int)(pp * part_bytes) + (q0 + q) * NT * 16 + lane_off, 0, kSc);
#pragma unroll
        for (int q = 0; q < CH; ++q) {
          const int ij = (q0 + q) >> 2, qq = (q0 + q) & 3;
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[ij / NR][ij % NR][4 * qq + e] += __uint_as_float(v[q][e]);
        }
        __builtin_amdgcn_sched_barrier(0);                      // keep the batches apart (hoisting every load at once spills)
      }
    }
    __syncthreads();
  }

  // ---- epilogue: bias, InstanceNorm partial sums, activation, LDS-staged coalesced store ----
  constexpr int CROW = BN * (int)sizeof(TO) + 16;           // padded C-tile row
  float oscale = 1.f;                                        // fp8: de-quantisation factor of the packed weights
  if constexpr (sizeof(T) == 1) oscale = *d.out_scale;
  char* ct = stages;
  // The epilogue is VALU-bound (64-192 accumulators per lane, two waves per SIMD), so its per-element work is chosen
  // ONCE per tile: ACT = tanh | slope family (ReLU / LeakyReLU as one select) | identity (every layer that wants
  // statistics: its activation runs after the normalisation), and FULL = every tile row is a pixel of the sample (no
  // row masks in the sums; all tiles but a sample's last).  A per-element switch costs a dozen scalar branches per
  // value and keeps the tanh expansion in every element's path.
  const float neg_slope = act == P2PHD_ACT_RELU ? 0.f : (act == P2PHD_ACT_LRELU ? 0.2f : 1.f);
  constexpr int ACT_IDENT = -1;
  auto stage_tile = [&](auto act_tag, auto full_tag) {
    constexpr int ACT = decltype(act_tag)::value;
    constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int col = wn * (NR * 32) + j * 32 + lr;
      int k = n0 + col, kcls = 0;
      if (cls_cp > 0) {                                        // merged sub-pixel classes share bias / statistics of channel k
        if (k >= n_extent) k = Kout;
        else { kcls = (k >= cls_cp) + (k >= 2 * cls_cp) + (k >= 3 * cls_cp); k -= kcls * cls_cp; }
      }
      const float bv = (bias != nullptr && k < Kout) ? bias[k] : 0.f;
      float s1 = 0.f;
#pragma unroll
      for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = wm * (MR * 32) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
          if constexpr (sizeof(T) == 1) acc[i][j][e] *= oscale;
          float v = acc[i][j][e] + bv;
          if (FULL || p_base + row < p_end) s1 += v;
          if constexpr (ACT == P2PHD_ACT_TANH) v = tanhf(v);
          else if constexpr (ACT != ACT_IDENT) v = v > 0.f ? v : neg_slope * v;   // none / ReLU / LeakyReLU(0.2) as one select
          *reinterpret_cast<TO*>(ct + row * CROW + col * (int)sizeof(TO)) = from_f<TO>(v);
        }
      }
      if (stats != nullptr) {
        // InstanceNorm partial of this wave's MR*32 rows: (sum, sum of squared deviations from the wave's OWN mean),
        // stored plainly in the wave's slot of a [N][slots][classes][Cp][2] table that a small kernel merges with Chan's
        // update.  No float atomics (bit-reproducible), and no E[x^2] - E[x]^2 cancellation: a dB spectrogram puts
        // |mean| / sigma up to 25 in front of the first InstanceNorm, which costs that formula 3 digits in fp32.
        s1 += __shfl_xor(s1, 32);
        const int first = p_base + wm * (MR * 32);
        const int cnt = FULL ? MR * 32 : min(max(p_end - first, 0), MR * 32);
        const float mean_w = cnt > 0 ? s1 / (float)cnt : 0.f;
        float m2 = 0.f;
#pragma unroll
        for (int i = 0; i < MR; ++i) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int row = wm * (MR * 32) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            const float dlt = acc[i][j][e] + bv - mean_w;
            if (FULL || p_base + row < p_end) m2 += dlt * dlt;
          }
        }
        m2 += __shfl_xor(m2, 32);
        if (lh == 0 && k < Kout && cnt > 0) {                  // waves past the sample's last row own no slot
          const int slot = first / (MR * 32);
          const int ncls = cls_cp > 0 ? 4 : 1;
          float* sp = stats + 2 * ((((size_t)n * stats_slots + slot) * ncls + kcls) * Cp_out + k);
          sp[0] = s1;
          sp[1] = m2;
        }
      }
    }
  };
  {
    typedef std::true_type Y;
    typedef std::false_type N_;
    typedef std::integral_constant<int, P2PHD_ACT_TANH> Tanh;
    typedef std::integral_constant<int, P2PHD_ACT_RELU> Slope;
    typedef std::integral_constant<int, ACT_IDENT> Ident;
    if constexpr (MR * NR <= 6) {
      const bool full = p_base + BM <= p_end;
      if (act == P2PHD_ACT_TANH) stage_tile(Tanh{}, N_{});
      else if (act == P2PHD_ACT_NONE) { if (full) stage_tile(Ident{}, Y{}); else stage_tile(Ident{}, N_{}); }
      else { if (full) stage_tile(Slope{}, Y{}); else stage_tile(Slope{}, N_{}); }
    } else {
      // the 128-accumulator tile keeps two instances: more straight-line copies cost it registers (it spills)
      if (act == P2PHD_ACT_TANH) stage_tile(Tanh{}, N_{});
      else stage_tile(Slope{}, N_{});
    }
  }
#ifdef P2PHD_PROBE_FINE
  const unsigned long long pf_c = __builtin_readcyclecounter();
#endif
  __syncthreads();
#ifdef P2PHD_PROBE_FINE
  const unsigned long long pf_d = __builtin_readcyclecounter();
#endif
  constexpr int CPR = BN / EPPO;                             // 16-byte pieces per C-tile row
  const int Hout = d.Hout, Wout = d.Wout, ohm = d.oh_mul, oho = d.oh_off, owm = d.ow_mul, owo = d.ow_off;
  if constexpr (MR * NR <= 6 && sizeof(T) != 1) {
    if (d.bs_out != nullptr || d.as_x != nullptr) {
      // Store loop with the consumer's InstanceNorm-backward sums riding on it (GDesc::bs_out) -- or, for a producer
      // without normalisation, just its activation derivative applied to the stored gradient (GDesc::as_x).  A thread keeps ONE
      // piece column (8 / 4 channels) for all its rows, so the channel constants are loaded once and the sums stay in
      // registers; they are folded over the threads of a column through LDS in a fixed order (no atomics) and leave as
      // this tile's row of the partial table.
      constexpr int RG = NT / CPR;                           // threads per piece column (the last NT % CPR threads idle)
      const int pcb = tid % CPR, rgb = tid / CPR;
      const int kb = n0 + pcb * EPPO;
      int kch = kb, clsb = 0;
      if (cls_cp > 0) { clsb = (kb >= cls_cp) + (kb >= 2 * cls_cp) + (kb >= 3 * cls_cp); kch = kb - clsb * cls_cp; }
      const bool col_ok = kb < n_extent && rgb < RG;
      float a1[EPPO], a2[EPPO], mean_b[EPPO], rstd_b[EPPO];
#pragma unroll
      for (int e = 0; e < EPPO; ++e) {
        a1[e] = a2[e] = 0.f;
        const bool ch_ok = col_ok && kch + e < Kout && d.bs_out != nullptr;
        const float2 ms = ch_ok ? *reinterpret_cast<const float2*>(d.bs_stats + 2 * ((size_t)n * Cp_out + kch + e)) : make_float2(0.f, 0.f);
        mean_b[e] = ms.x;
        rstd_b[e] = ch_ok ? rsqrtf(fmaxf(ms.y * d.bs_inv_hw, 0.f) + d.bs_eps) : 0.f;
      }
      const bool act_only = d.bs_out == nullptr;
      const TO* bsy = reinterpret_cast<const TO*>(act_only ? d.as_x : d.bs_y);
      const float slope_b = d.bs_slope;
      if (col_ok) {
        // U rows at a time: their pre-normalisation pieces (and addends) are all requested before the first one is used --
        // a load consumed in the iteration that issues it costs a memory round trip per row
        constexpr int U = 4;
        for (int row0 = rgb; row0 < BM; row0 += RG * U) {
          uint4 yv[U], av[U];
          size_t opx[U];
          bool ok[U];
          int rowu[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int row = row0 + u * RG;
            rowu[u] = min(row, BM - 1);
            const int2 ri = rinfo[rowu[u]];
            int ho = ri.y >> 16, wo = ri.y & 0xFFFF;
            ok[u] = row < BM && ri.x >= 0;
            if (cls_cp > 0) {
              ho = 2 * ho + (clsb >> 1); wo = 2 * wo + (clsb & 1);
              ok[u] = ok[u] && ho < Hout && wo < Wout;
            }
            opx[u] = ok[u] ? ((size_t)ri.x * Hout + (ho * ohm + oho)) * Wout + (wo * owm + owo) : 0;   // clamped: always loadable
            yv[u] = *reinterpret_cast<const uint4*>(bsy + opx[u] * Cp_out + kch);
            if (addend != nullptr) av[u] = *reinterpret_cast<const uint4*>(addend + opx[u] * Cp_out + kch);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            uint4 v = *reinterpret_cast<const uint4*>(ct + rowu[u] * CROW + pcb * 16);
            if (addend != nullptr) {
              TO* vv = reinterpret_cast<TO*>(&v);
              const TO* aa = reinterpret_cast<const TO*>(&av[u]);
#pragma unroll
              for (int e = 0; e < EPPO; ++e) vv[e] = from_f<TO>(to_f(vv[e]) + to_f(aa[e]));
            }
            const TO* yy = reinterpret_cast<const TO*>(&yv[u]);
            if (act_only) {
              TO* vv = reinterpret_cast<TO*>(&v);
#pragma unroll
              for (int e = 0; e < EPPO; ++e) vv[e] = from_f<TO>(to_f(vv[e]) * (to_f(yy[e]) > 0.f ? 1.f : slope_b));
              *reinterpret_cast<uint4*>(out + opx[u] * Cp_out + kch) = v;
              continue;
            }
            *reinterpret_cast<uint4*>(out + opx[u] * Cp_out + kch) = v;
            const TO* gg = reinterpret_cast<const TO*>(&v);      // the ROUNDED gradient: what the apply pass will read
#pragma unroll
            for (int e = 0; e < EPPO; ++e) {
              const float yh = (to_f(yy[e]) - mean_b[e]) * rstd_b[e];
              const float gp = to_f(gg[e]) * (yh > 0.f ? 1.f : slope_b);
              a1[e] += gp; a2[e] += gp * yh;
            }
          }
        }
      }
      if (act_only) return;
      __syncthreads();                                        // every thread is done with the C tile
      float* red = reinterpret_cast<float*>(ct);              // [NT][2 * EPPO]
#pragma unroll
      for (int e = 0; e < EPPO; ++e) { red[tid * (2 * EPPO) + e] = a1[e]; red[tid * (2 * EPPO) + EPPO + e] = a2[e]; }
      __syncthreads();
      const int tile_in_sample = bx - n * mtiles;
      for (int t = tid; t < 2 * BN; t += NT) {
        const int col = t >> 1, which = t & 1, pc = col / EPPO, e = col - pc * EPPO;
        float sum = 0.f;
        for (int rg = 0; rg < RG; ++rg) sum += red[(rg * CPR + pc) * (2 * EPPO) + which * EPPO + e];
        if (n0 + col < n_extent)
          d.bs_out[(((size_t)n * mtiles + tile_in_sample) * n_extent + n0 + col) * 2 + which] = sum;
      }
      return;
    }
  }
  // U pieces per thread at a time: their row records, staged pieces (and addends) are all requested before the first one
  // is used -- one piece per iteration costs two LDS round trips and a branch per 16 bytes stored (2 waves per SIMD: nobody
  // to hide them behind)
  {
    constexpr int TOTAL = BM * CPR, U = 4;
    for (int q0 = tid; q0 < TOTAL; q0 += NT * U) {
      int2 ri[U];
      int rowu[U], pcu[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = min(q0 + u * NT, TOTAL - 1);
        rowu[u] = q / CPR; pcu[u] = q - rowu[u] * CPR;
        ri[u] = rinfo[rowu[u]];
      }
      uint4 v[U], av[U];
      size_t off[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int k = n0 + pcu[u] * EPPO;
        ok[u] = q0 + u * NT < TOTAL && ri[u].x >= 0 && k < n_extent;
        int ho = ri[u].y >> 16, wo = ri[u].y & 0xFFFF;
        if (cls_cp > 0) {                                        // class (pi,pj) -> output pixel (2 ho + pi, 2 wo + pj)
          const int cls = (k >= cls_cp) + (k >= 2 * cls_cp) + (k >= 3 * cls_cp);
          k -= cls * cls_cp;
          ho = 2 * ho + (cls >> 1); wo = 2 * wo + (cls & 1);
          ok[u] = ok[u] && ho < Hout && wo < Wout;
        }
        off[u] = ok[u] ? (((size_t)ri[u].x * Hout + (ho * ohm + oho)) * Wout + (wo * owm + owo)) * Cp_out + k : 0;   // clamped: always loadable
        v[u] = *reinterpret_cast<const uint4*>(ct + rowu[u] * CROW + pcu[u] * 16);
        if (addend != nullptr) av[u] = *reinterpret_cast<const uint4*>(addend + off[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (addend != nullptr) {
          TO* vv = reinterpret_cast<TO*>(&v[u]);
          const TO* aa = reinterpret_cast<const TO*>(&av[u]);
#pragma unroll
          for (int e = 0; e < EPPO; ++e) vv[e] = from_f<TO>(to_f(vv[e]) + to_f(aa[e]));
        }
        if (ok[u]) *reinterpret_cast<uint4*>(out + off[u]) = v[u];
      }
    }
  }
#ifdef P2PHD_PROBE
#ifdef P2PHD_PROBE_DRAIN
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // include the completion of this tile's stores
#endif
  const unsigned long long pr_t3 = __builtin_readcyclecounter();
  if (tid == 0) {
    const unsigned wg = (unsigned)blockIdx.x % kProbeSlots;
    unsigned long long* r = g_probe + (size_t)wg * 8;
#ifdef P2PHD_PROBE_FINE
    // prologue: table build | descriptor + fragment addresses + DMA issue | first wait + barrier + first fragments;
    // epilogue: statistics + LDS staging | barrier | store loop (the barrier after the K loop is in the first)
    r[0] += pf_a - pr_t0; r[1] += pf_b - pf_a; r[2] += pr_t1_ - pf_b; r[3] += pr_t2 - pr_t1_;
    r[4] += pf_c - pr_t2; r[5] += pf_d - pf_c; r[6] += 1ull; r[7] += pr_t3 - pf_d;
#else
    r[0] += pr_wait_; r[1] += pr_bar_; r[2] += pr_comp_; r[3] += (unsigned long long)nsteps_;
    r[4] += pr_t1_ - pr_t0; r[5] += pr_t3 - pr_t2; r[6] += 1ull; r[7] += pr_t3 - pr_t0;
#endif
  }
#endif
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
// measurement hook (p2phd_probe_gconv): events around matching launches, on the launch stream
struct GconvProbe {
  bool on = false;
  int cp = 0, kk = 0, hg = 0, wg = 0;
  int pad_mode = -1, esize = 0;                  // -1 / 0 = any: tells the forward (reflect gather) from the input gradient (pad_mode 2)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};
GconvProbe g_probe_cfg;

template <typename T, int BM, int BN, int MR, int NR, int NSTAGE, int HALO = 0>
int launch_gconv_cfg(const GDesc& d_in, const void* in, const void* wp, const float* bias, const void* addend, void* out,
                     float* stats, hipStream_t st, int* slot_rows) {
  GDesc d = d_in;
  // InstanceNorm partials: one slot per wave row block (MR * 32 rows) of a sample, see the epilogue
  d.stats_slots = (d.Hg * d.Wg + MR * 32 - 1) / (MR * 32);
  if (slot_rows) *slot_rows = p2phd::gconv_slot_rows(BM, MR, d.bs_out != nullptr);
  constexpr int STAGE = (BM + BN) * kRowBytes;
  constexpr int CT = BM * (BN * (int)sizeof(typename OutOf<T>::type) + 16);
  const int tab = (HALO ? 0 : ((d.nth * d.ntw * BM * 4 + 15) & ~15)) + BM * 8;        // gather table + row table
  constexpr int RING = HALO ? 2 * (20 * 20 * kRowBytes) + 2 * BN * kRowBytes : NSTAGE * STAGE;   // (HALO: two halo grids + two weight slabs, gconv_halo.inc)
  const size_t lds = tab + (size_t)(RING > CT ? RING : CT);
  auto kern = gconv_kernel<T, BM, BN, MR, NR, NSTAGE, HALO>;
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  const int npix = d.Hg * d.Wg;
  const int mtiles = d.flat_m ? (int)(((long)d.N * npix + BM - 1) / BM) : ((npix + BM - 1) / BM) * d.N;
  const int ntiles = (d.n_extent + BN - 1) / BN;
  // 1-D grid over tiles (tile = n_tile * mtiles + m_tile).  Split-K tail ("stream-K" for the last round only): with one
  // workgroup per CU a grid of T tiles runs in ceil(T / CUs) rounds, and the last round of e.g. 561 or 269 tiles keeps
  // 49 / 13 CUs busy for a whole tile time.  Those tail tiles are cut along K into P = floor(CUs / tail) parts that fill
  // the round; the part that finishes last adds the partials in a fixed order (gconv_kernel).  Partials live in the
  // library's reduction scratch (common.h), so no entry point needs a bigger workspace.
  const int TT = mtiles * ntiles;
  d.grid_m = mtiles;
  d.sk_first = TT; d.sk_tail = 1; d.sk_parts = 1; d.sk_steps = 0; d.sk_part = nullptr; d.sk_ticket = nullptr;
  int wgs = TT;
  // CUs this launch can occupy: the device's count (cached per device), or what the caller states with
  // p2phd_set_option("cus", n) when the step runs on a CU-masked stream (opt.comm_cus leaves some to the RCCL kernels)
  const int cus = p2phd::g_opt_cus > 0 ? p2phd::g_opt_cus : p2phd::device_cus();
  if (p2phd::g_opt_splitk_tail != 0 && d.cls_skip == 0 && HALO == 0) {        // (tap-skipping tiles differ in depth: their order balances the rounds)
    const int nsteps = d.KK / (8 * Elem<T>::EPP);
    const int full = TT / cus * cus, tail = TT - full;
    // Cost model in microseconds (layer tables of profiles/r03_*): a K slab of a BM x BN tile at the rate one CU sustains in
    // this loop, a fixed prologue + epilogue, one partial store per part and one partial load per part by the finisher
    // (sc1 traffic of 4 BM BN bytes each).  The finisher term grows with P, so the best P is about sqrt(K time / load time):
    // deep reductions (the 256 -> 512 layers) split 4-7 ways, short ones not at all.
    const double area = (double)BM * BN / 65536.0;
    const double t_slab = (double)BM * BN * 128.0 / 6.0e6, c0 = 8.0 + 16.0 * area, c_io = 4.0 * area;
    const double t_tile = c0 + nsteps * t_slab;
    // (a sparse last round runs faster per tile than a full one -- fewer CUs on the memory system, higher clock --, which
    // is why the measured gain of filling it is smaller than a whole tile time)
    const double now = (double)(full / cus) * t_tile + (tail > 0 ? 0.75 * t_tile : 0.0);
    int bestP = 1;
    double best = now;
    const int pmax = tail > 0 ? std::min(cus / tail, nsteps / 4) : 1;
    for (int P = 2; P <= pmax; ++P) {
      const int steps = (nsteps + P - 1) / P;
      const int Pe = (nsteps + steps - 1) / steps;               // no empty parts
      const double t = (double)(full / cus) * t_tile + c0 + steps * t_slab + c_io + Pe * c_io;
      if (t < best) { best = t; bestP = Pe; }
    }
    if (p2phd::g_opt_splitk_tail == 2 && pmax >= 2) {            // tests: split as deep as allowed whatever the model says
      const int steps = (nsteps + pmax - 1) / pmax;
      bestP = (nsteps + steps - 1) / steps;
      best = 0.0;
    }
    if (bestP >= 2 && best < 0.95 * now) {
      const p2phd::FoldScratch fs = p2phd::fold_scratch(p2phd::FOLD_GCONV, st);
      const int steps = (nsteps + bestP - 1) / bestP;
      if (fs.part != nullptr && (size_t)tail * bestP * BM * BN <= fs.floats && tail <= fs.tickets) {   // (more tail tiles than tickets -- chips beyond 256 CUs -- simply run unsplit)
        d.sk_first = full; d.sk_tail = tail; d.sk_parts = bestP; d.sk_steps = steps; d.sk_part = fs.part; d.sk_ticket = fs.ticket;
        wgs = full + tail * bestP;
      }
    }
  }
#ifdef P2PHD_CHECK_WAITS
  d.cw_inject = p2phd::g_opt_cw_inject;
#endif
  dim3 grid((unsigned)wgs);
  const bool probe = g_probe_cfg.on && d.Cp_in == g_probe_cfg.cp && d.KK == g_probe_cfg.kk && d.Hg == g_probe_cfg.hg &&
                     d.Wg == g_probe_cfg.wg && (g_probe_cfg.pad_mode < 0 || d.pad_mode == g_probe_cfg.pad_mode) &&
                     (g_probe_cfg.esize == 0 || (int)sizeof(T) == g_probe_cfg.esize) && g_probe_cfg.ev.size() < 4096;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (probe) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, st); }
  typedef typename OutOf<T>::type TO;
  hipLaunchKernelGGL(kern, grid, dim3((BM / (MR * 32)) * (BN / (NR * 32)) * 64), lds, st, d, (const T*)in, (const T*)wp, bias, (const TO*)addend, (TO*)out, stats);
  ++p2phd::g_launch_count[p2phd::LC_GCONV];
  if (HALO != 0) ++p2phd::g_launch_count[p2phd::LC_HALO];
  if (d.cls_skip != 0) ++p2phd::g_launch_count[p2phd::LC_CLS_SKIP];
  if (d.sk_parts > 1) ++p2phd::g_launch_count[p2phd::LC_SPLITK];
  if (BM == 256 && BN == 256) ++p2phd::g_launch_count[p2phd::LC_TILE256];
  if (BM == 128 && BN == 192) ++p2phd::g_launch_count[p2phd::LC_TILE128X192];
  if (probe) { (void)hipEventRecord(e1, st); g_probe_cfg.ev.emplace_back(e0, e1); }
  return p2phd::check_launch("gconv");
}

// Dispatch: the instantiations each element type can reach, keyed by the tile gconv_choose_tile returns.  A tile that is
// not listed for its type is an error, never a fall-back to another tile.
typedef int (*GconvLaunch)(const GDesc&, const void*, const void*, const float*, const void*, void*, float*, hipStream_t, int*);
struct GconvRow { int bm, bn, mr, nr, nstage, halo; GconvLaunch launch; };
#define GCONV_ROW(T, BM, BN, MR, NR, NS, HALO) {BM, BN, MR, NR, NS, HALO, launch_gconv_cfg<T, BM, BN, MR, NR, NS, HALO>}
#define GCONV_ROWS_EVERY_TYPE(T) \
  GCONV_ROW(T, 128, 128, 2, 2, 2, 0), GCONV_ROW(T, 128, 64, 2, 1, 2, 0), GCONV_ROW(T, 128, 32, 1, 1, 2, 0), \
  GCONV_ROW(T, 256, 128, 2, 2, 3, 0), GCONV_ROW(T, 256, 128, 2, 2, 2, 0), GCONV_ROW(T, 256, 64, 2, 1, 3, 0), GCONV_ROW(T, 256, 64, 2, 1, 2, 0)
const GconvRow kTilesF32[] = {GCONV_ROWS_EVERY_TYPE(float)};
const GconvRow kTilesFp8[] = {GCONV_ROWS_EVERY_TYPE(fp8_t), GCONV_ROW(fp8_t, 256, 192, 2, 3, 2, 0)};   // (256 x 256 spills with the two-MFMA fp8 fragments)
const GconvRow kTiles16[] = {GCONV_ROWS_EVERY_TYPE(bf16_t), GCONV_ROW(bf16_t, 256, 192, 2, 3, 2, 0), GCONV_ROW(bf16_t, 256, 256, 4, 2, 2, 0),
                             GCONV_ROW(bf16_t, 256, 192, 2, 3, 2, 1), GCONV_ROW(bf16_t, 256, 128, 2, 2, 2, 1), GCONV_ROW(bf16_t, 128, 192, 2, 3, 2, 0)};
#undef GCONV_ROWS_EVERY_TYPE
#undef GCONV_ROW

template <size_t ROWS>
int launch_gconv_tile(const GconvRow (&table)[ROWS], int dtype, GDesc d, const void* in, const void* wp, const float* bias, const void* addend,
                      void* out, float* stats, hipStream_t st, int* slot_rows) {
  if (d.n_extent == 0) d.n_extent = d.Cp_out;
  const GconvTile t = p2phd::gconv_choose_tile(d, dtype, stats != nullptr);
  if (t.bm == 0) return P2PHD_EINVAL;                            // (refused: error text set by the chooser)
  d.flat_m = t.flat_m;
  for (const GconvRow& r : table)
    if (r.bm == t.bm && r.bn == t.bn && r.mr == t.mr && r.nr == t.nr && r.nstage == t.nstage && r.halo == t.halo)
      return r.launch(d, in, wp, bias, addend, out, stats, st, slot_rows);
  p2phd::set_error("gconv: no %d x %d tile (waves %d x %d, %d ring slots, halo %d) for dtype %d", t.bm, t.bn, t.mr, t.nr, t.nstage, t.halo, dtype);
  return P2PHD_EINVAL;
}

}  // namespace

namespace p2phd {

// ---- the tile of a gather-GEMM launch ------------------------------------------------------------------------------------
namespace {
// The 160 KiB of LDS beside the tables of a 256-row tile (gather table of `taps` offsets per row + row table, launch_gconv_cfg)
struct LdsBudget {
  long tables;
  explicit LdsBudget(int taps) : tables((long)taps * 256 * 4 + 16 + 256 * 8) {}
  bool holds(long bytes) const { return bytes + tables <= 160 * 1024; }
  bool ring(int slots, int bn) const { return holds((long)slots * (256 + bn) * kRowBytes); }          // `slots` stages of the A and B tiles
  bool c_tile(int bn, int out_bytes) const { return holds(256 * ((long)bn * out_bytes + 16)); }       // the output tile staged for the store loop
};

// Workgroups one round of the chip runs, as the two cost comparisons below count them: one 8-wave or 192-wide workgroup per CU;
// the light 128 x 128 workgroups go two to a CU.  A literal, NOT the device's CU count (that belongs to the split-K tail of
// launch_gconv_cfg): replacing it would move layers between tiles on other chips or under the "cus" option, which is a change
// of behaviour with its own measurements.
constexpr double kWgsPerRound = 256.0;
double rounds(long wgs, double per_round) { return std::ceil(wgs / per_round); }

// The HALO main loop (gconv_halo.inc): 3 x 3 taps within one pixel of the centre on a 16-wide plane whose height is a multiple
// of 16, gathered tensor of the same size, 64-channel chunks, full K rows (no padding tail), per-sample M tiles
bool gconv_halo_ok(const GDesc& d, bool flat_m) {
  const bool taps = d.nth == 3 && d.ntw == 3 && d.sh == 1 && d.sw == 1 &&
                    ((d.dh0 == -1 && d.dh_step == 1) || (d.dh0 == 1 && d.dh_step == -1)) &&
                    ((d.dw0 == -1 && d.dw_step == 1) || (d.dw0 == 1 && d.dw_step == -1));
  return g_opt_gconv_halo != 0 && taps && d.cls_cp == 0 && d.Wg == 16 && d.Hg % 16 == 0 && d.Hg >= 16 && d.Hin == d.Hg && d.Win == d.Wg &&
         d.Cp_in % 64 == 0 && d.KK == 9 * d.Cp_in && (d.pad_mode == 0 || d.pad_mode == 1 || d.pad_mode == 3) && !flat_m &&
         d.oh_mul == 1 && d.ow_mul == 1 && d.oh_off == 0 && d.ow_off == 0;
}
}  // namespace

long gconv_mtiles256(const GDesc& d, bool flat_m) {
  const int npix = d.Hg * d.Wg;
  return flat_m ? ((long)d.N * npix + 255) / 256 : (long)((npix + 255) / 256) * d.N;
}

bool gconv_256x192_fills_chip(const GDesc& d, bool flat_m) {
  return gconv_mtiles256(d, flat_m) * ((d.n_extent ? d.n_extent : d.Cp_out) / kGconvCols192) >= 192;
}

GconvTile gconv_choose_tile(const GDesc& d, int dtype, bool stats_wanted) {
  // what the operand type fixes: 16-bit (bf16 / fp16), fp8 (bf16 outputs) or f32
  const bool h16 = dtype == P2PHD_BF16, fp8 = dtype == P2PHD_FP8_INTERNAL, f32 = !h16 && !fp8;
  const int epp = fp8 ? 16 : (h16 ? 8 : 4), out_bytes = f32 ? 4 : 2;   // elements per 16-byte piece of K; bytes of an output element
  const int k = d.n_extent ? d.n_extent : d.Cp_out;              // GEMM N extent
  if (d.cls_skip != 0) {                                         // (planned for this tile: merged_plan)
    if (h16) return GconvTile{256, 192, 2, 3, 2, 0, 0};
    set_error("gconv: a tap-skipping merged plan reached a non-16-bit launch");
    return GconvTile{};
  }
  const int force = g_opt_gconv_bm;                              // 0 = heuristic
  const bool fused = d.bs_out != nullptr || d.as_x != nullptr;   // fused store loop of the input gradient (sums / activation backward)
  const int npix = d.Hg * d.Wg;
  // no per-sample sums wanted: M tiles may straddle samples
  const bool flat_m = !stats_wanted && d.bs_out == nullptr && npix % 256 != 0;
  const long mt256 = gconv_mtiles256(d, flat_m);
  const LdsBudget lds(d.nth * d.ntw);
  // N tile: the 128-wide tile has the best MFMA density (64x64 per wave) and reads the gathered A operand once;
  // narrower tiles only for layers that would leave most of it empty
  const int bn = k > 64 ? 128 : (k > 32 ? 64 : 32);

  // ---- eligibility, each stated once ----
  // a sample (or, flat, the batch) has enough pixels to fill 256-row tiles
  const bool enough_px = flat_m ? (long)d.N * npix >= 2048 : (npix >= 256 && (npix % 256 == 0 || npix >= 2048));
  // short reductions (<= 4 K steps: the folded 2-channel layers, the 4-channel D input) are all prologue and epilogue:
  // keep the light 128-row kernel there, several of which fit on a CU and overlap each other's fixed costs
  const bool short_k = d.KK <= 4 * 8 * epp;
  // a wide output whose 256 x 256 grid still fills most of the chip
  const bool wide = enough_px && k >= 256 && (k % 256 == 0 || k >= 1024) && mt256 * ((k + 255) / 256) >= 160;
  // 256 x 256 (8 waves of 128 x 64, 2-slot ring): 16-bit only (it spills with the two-MFMA fp8 fragments, f32 never takes it),
  // and its 128-accumulator waves have no fused store loop
  const bool fits256 = h16 && lds.ring(2, 256) && lds.c_tile(256, 2) && !fused;
  const bool take256 = force == 512 ? fits256 && k > 128 : ((force == 0 || force == 192) && fits256 && wide);   // (192 forces its own tile only)
  // 256 x 192 (8 waves of 64 x 96, 2-slot ring): 16-bit and fp8, outputs the tile divides
  const bool fits192 = !f32 && k % kGconvCols192 == 0 && lds.ring(2, kGconvCols192);
  // 256 x {128, 64}: 3-slot ring when it fits beside the gather table, else 2-slot (258: experiments, 256 rows on the 2-slot ring)
  const bool ring3 = bn >= 64 && lds.ring(3, bn) && force != 258;
  const bool ring2 = bn >= 64 && lds.ring(2, bn) && lds.c_tile(bn, out_bytes);
  // 256-row tiles (8 waves) halve the weight traffic per FLOP: when a sample has enough pixels to fill them and the grid
  // still covers the chip
  const bool rows256 = (ring3 || ring2) && (force == 256 || force == 258 ||
                                            (force != 128 && enough_px && !short_k && mt256 * ((k + bn - 1) / bn) >= 192));

  // ---- the tiles, first match wins ----
  if (force == 192 && fits192) return GconvTile{256, 192, 2, 3, 2, 0, flat_m};
  // 256 x 192 where the 256 x 256 grid would leave CUs idle that a 192-wide N tile fills (the residual trunk: 768 = 4 x 192 ->
  // 64 x 4 = 256 workgroups instead of 64 x 3 = 192); fp8 has no 256 x 256 tile and takes it whenever it divides a wide output.
  // With the HALO loop where the plane allows.
  if (force == 0 && fits192 && (take256 || (fp8 && wide))) {
    const long wg256 = mt256 * ((k + 255) / 256), wg192 = mt256 * (k / kGconvCols192);
    const double c256 = rounds(wg256, kWgsPerRound) * 256.0 * 256.0, c192 = rounds(wg192, kWgsPerRound) * 256.0 * 192.0 / 0.95;
    if (fp8 || c192 < c256) return GconvTile{256, 192, 2, 3, 2, h16 && gconv_halo_ok(d, flat_m) ? 1 : 0, flat_m};
  }
  // ... and for 192- / 384-wide outputs (the 96-channel layers and the merged sub-pixel launches of the up path), where
  // 128-wide tiles would gather the A operand once more and pad the last tile; wider ones only with a fused store loop
  if (force == 0 && fits192 && !take256 && enough_px && !short_k && (k <= 384 || fused) && gconv_256x192_fills_chip(d, flat_m))
    return GconvTile{256, 192, 2, 3, 2, 0, flat_m};
  if (take256) return GconvTile{256, 256, 4, 2, 2, 0, flat_m};
  if (rows256 && bn == 128) {
    // the HALO loop on 128-wide tiles: 16-wide planes whose 192- / 256-wide grids leave CUs idle
    // (configs[4]'s 2048-channel trunk at B = 8; the 768-channel trunk below B = 27)
    if (h16 && force == 0 && k % 128 == 0 && gconv_halo_ok(d, flat_m)) return GconvTile{256, 128, 2, 2, 2, 1, flat_m};
    return GconvTile{256, 128, 2, 2, ring3 ? 3 : 2, 0, flat_m};
  }
  if (rows256 && bn == 64) return GconvTile{256, 64, 2, 1, ring3 ? 3 : 2, 0, flat_m};
  // 128 x 192 (4 waves of 64 x 96): planes too small for 256-row tiles whose 128 x 128 grid would run a second, half-empty
  // round (the 1536-channel trunk of the two-scale generator at 16 x 8: 32 x 12 = 384 tiles -> 32 x 8 = 256)
  if (h16 && force == 0 && g_opt_tile128x192 != 0 && !flat_m && !short_k && k % 192 == 0 && k >= 384) {
    const long mt128 = (long)((npix + 127) / 128) * d.N;
    const long wg128 = mt128 * ((k + 127) / 128), wg192 = mt128 * (k / 192);
    if (rounds(wg192, kWgsPerRound) * 192.0 < rounds(wg128, 2 * kWgsPerRound) * 2.0 * 128.0 && wg192 >= 192)
      return GconvTile{128, 192, 2, 3, 2, 0, flat_m};
  }
  if (bn == 128) return GconvTile{128, 128, 2, 2, 2, 0, flat_m};
  if (bn == 64) return GconvTile{128, 64, 2, 1, 2, 0, flat_m};
  return GconvTile{128, 32, 1, 1, 2, 0, flat_m};
}

}  // namespace p2phd

namespace p2phd {

int launch_gconv(const GDesc& d_in, int dtype, const void* in, const void* wp, const float* bias, const void* addend,
                 void* out, float* stats, hipStream_t st, int* slot_rows) {
  if (d_in.N == 0 || d_in.Hg * d_in.Wg == 0) return P2PHD_OK;
  GDesc d = d_in;
  {
    const size_t esz = dtype == P2PHD_FP8_INTERNAL ? 1 : (dtype == P2PHD_BF16 ? 2 : 4);
    size_t ib = (size_t)d.N * d.Hin * d.Win * d.Cp_in * esz;
    if (d.pad_mode == 3) ib += (size_t)d.N * (2 * (d.Win + 2) + 2 * d.Hin) * d.Cp_in * esz;   // + the reflection extras behind the tensor
    const size_t wb = (size_t)round_up(d.cls_cp > 0 ? 4 * d.cls_cp : d.Cp_out, 128) * d.KK * esz;   // packed rows are padded to 128
    P2PHD_REQUIRE(ib < 0xFFFFFFF0ull && wb < 0xFFFFFFF0ull, "gconv: tensor larger than 4 GiB");
    d.in_bytes = (unsigned)ib;
    d.w_bytes = (unsigned)wb;
  }
  P2PHD_REQUIRE(d.Cp_in % 8 == 0 && d.Cp_out % 8 == 0, "gconv: channel pitch must be a multiple of 8");
  P2PHD_REQUIRE((long)d.N * d.Hin * d.Win < (1l << 31) && (long)d.N * d.Hout * d.Wout < (1l << 31), "gconv: too many pixels");
  if (dtype == P2PHD_FP8_INTERNAL) {
    P2PHD_REQUIRE(d.Cp_in % 16 == 0 && d.KK % 128 == 0 && d.out_scale != nullptr, "gconv(fp8): channel pitch %% 16, GEMM-K %% 128 and a scale are required");
    return launch_gconv_tile(kTilesFp8, dtype, d, in, wp, bias, addend, out, stats, st, slot_rows);
  }
  if (dtype == P2PHD_BF16) return launch_gconv_tile(kTiles16, dtype, d, in, wp, bias, addend, out, stats, st, slot_rows);
  if (dtype == P2PHD_F32) return launch_gconv_tile(kTilesF32, dtype, d, in, wp, bias, addend, out, stats, st, slot_rows);
  set_error("gconv: unsupported dtype %d", dtype);
  return P2PHD_EUNSUPPORTED;
}

}  // namespace p2phd

// Wait checker (-DP2PHD_CHECK_WAITS build, libp2phd_hip_chk.so): out[0] = bit mask of the kernel families (1 gather-GEMM generic
// loop, 2 HALO loop, 4 weight gradient, 8 its f32 form) in which a relaxed s_waitcnt vmcnt(n) left a piece in flight that
// targets a buffer read behind the following barrier, out[1] = relaxed waits checked, out[2] = first offender
// (family << 16 | n << 8 | buffer tag), out[3] = LDS-DMA pieces logged.  Synchronises the device.  Returns P2PHD_EUNSUPPORTED in
// the product build (which carries no instrumentation).  The gather-GEMM (this file) and the weight gradient (wgrad.hip) keep a
// flag each: masks are OR-ed, counts added, and the first offender is the gather-GEMM's if it has one, else the weight
// gradient's -- "first" holds within each of the two groups of families, not in time across them.
extern "C" int p2phd_wait_check(unsigned* out4, int reset) {
#ifdef P2PHD_CHECK_WAITS
  P2PHD_REQUIRE(out4 != nullptr, "wait_check: null pointer");
  unsigned wg[4];                                                  // the weight gradient's copy of the flag (waitcheck.h)
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_cw_flag), sizeof(unsigned) * 4) != hipSuccess ||
      !p2phd::wgrad_wait_flag(wg, 0)) {
    p2phd::set_error("wait_check: cannot read the device flag");
    return P2PHD_ELAUNCH;
  }
  out4[0] |= wg[0]; out4[1] += wg[1]; out4[3] += wg[3];
  if (out4[2] == 0) out4[2] = wg[2];
  if (reset) {
    const unsigned z[4] = {0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_cw_flag), z, sizeof(z)) != hipSuccess || !p2phd::wgrad_wait_flag(nullptr, 1)) { p2phd::set_error("wait_check: reset failed"); return P2PHD_ELAUNCH; }
  }
  return P2PHD_OK;
#else
  (void)out4; (void)reset;
  p2phd::set_error("wait_check: this library was built without -DP2PHD_CHECK_WAITS (load libp2phd_hip_chk.so)");
  return P2PHD_EUNSUPPORTED;
#endif
}

extern "C" int p2phd_probe_gconv_ex(int enable, int cin_pitch, int kk, int hg, int wg, int pad_mode, int elem_bytes) {
  for (auto& e : g_probe_cfg.ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  g_probe_cfg.ev.clear();
  g_probe_cfg.on = enable != 0;
  g_probe_cfg.cp = cin_pitch; g_probe_cfg.kk = kk; g_probe_cfg.hg = hg; g_probe_cfg.wg = wg;
  g_probe_cfg.pad_mode = pad_mode; g_probe_cfg.esize = elem_bytes;
  return P2PHD_OK;
}

extern "C" int p2phd_probe_gconv(int enable, int cin_pitch, int kk, int hg, int wg) {
  return p2phd_probe_gconv_ex(enable, cin_pitch, kk, hg, wg, -1, 0);
}

extern "C" int p2phd_probe_read(float* ms_out, int cap) {
  int n = 0;
  for (auto& e : g_probe_cfg.ev) {
    if (n >= cap) break;
    if (hipEventSynchronize(e.second) != hipSuccess) break;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.first, e.second) != hipSuccess) break;
    if (ms_out) ms_out[n] = ms;
    ++n;
  }
  return n;
}

#ifdef P2PHD_PROBE
namespace p2phd { int wgrad_probe_add(unsigned long long* out8, int reset); }
extern "C" int p2phd_debug_probe(unsigned long long* out8, int reset) {
  static unsigned long long host[kProbeSlots * 8];
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_probe), sizeof(host)) != hipSuccess) return -1;
  for (int k = 0; k < 8; ++k) out8[k] = 0;
  for (int i = 0; i < kProbeSlots; ++i)
    for (int k = 0; k < 8; ++k) out8[k] += host[(size_t)i * 8 + k];
  if (reset) {
    void* dp = nullptr;
    if (hipGetSymbolAddress(&dp, HIP_SYMBOL(g_probe)) != hipSuccess || hipMemset(dp, 0, sizeof(host)) != hipSuccess) return -1;
  }
  return p2phd::wgrad_probe_add(out8, reset);                     // + the records of the weight gradient's own array (wgrad.hip)
}
#endif
