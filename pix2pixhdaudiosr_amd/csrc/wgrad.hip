// Weight gradient of the convolution family (gconv.hip describes the gather convolution and the layers it covers).
//
// The weight gradient is a second kernel: M = out channels, N = taps x in channels, reduction over pixels.
// Both operands then have the reduction index as the slow LDS dimension; bf16 fragments are fetched with the
// gfx950 transposing read ds_read_b64_tr_b16, so no transposed copy of the activations is made.
// The kernel leaves one packed f32 slab per pixel split; launch_unpack_grad (wpack.hip) sums them into the master layout.
#include "common.h"
#include "convplan.h"
#include "convdev.h"
#include "waitcheck.h"
#include <cmath>

namespace {

using p2phd::GDesc;

#ifdef P2PHD_PROBE
// experiment builds only (tools/ablate_gconv.sh): this code object's own record array, as gconv.hip has one (p2phd_debug_probe adds the two)
constexpr int kProbeSlots = 65536;
__device__ unsigned long long g_probe[kProbeSlots * 8];
#endif

// ------------------------------------------------------------------------------------------------------
// weight gradient:  dWp[split][m][t*Cg + c] = sum_{p in split} rows[p][m] * gather[pix(p,t)][c]
//   rows   : [N*Hg*Wg][Cp_r]   the tensor on the pixel grid (dy for Conv2d, x for ConvTranspose2d)
//   gather : [N,Hin,Win,Cp_in] the tensor reached through the taps
// Tile TM x 256 (TM = 128, or 32 for folded 2-channel layers), 64 (bf16) / 32 (f32) pixels per K step, 8 waves,
// 3-slot LDS ring fed by buffer_load ... lds with the next-but-one tile's pieces issued between MFMA clusters.
// The pixel reduction is split over blockIdx.z; every split writes its own slab (plain stores) and the unpack
// kernel adds the slabs in a fixed order: no float atomics, bit-reproducible gradients.
// ------------------------------------------------------------------------------------------------------
template <typename T, int TM>
__global__ __launch_bounds__(512) void wgrad_kernel(const GDesc d, const T* __restrict__ rows, const T* __restrict__ gat,
                                                    float* __restrict__ dwp, int Cp_r, int steps_per_split, long slab_elems,
                                                    unsigned rows_bytes, int grid_nx, int grid_my, int grid_sp, int xcd_order) {
  constexpr int EPP = Elem<T>::EPP;
  constexpr int SZ = (int)sizeof(T);
  constexpr int NT = 512;
  constexpr int BKP = SZ == 2 ? 64 : 32;                    // pixels per K-step
  constexpr int TN = 256;
  static_assert(TM == 256 || TM == 128 || TM == 32, "row tile");
  constexpr int WAVES_M = TM == 32 ? 1 : 2, WAVES_N = 8 / WAVES_M;
  constexpr int MI = TM / WAVES_M / 32, NI = TN / WAVES_N / 32;
  // LDS image: both operands are stored as PANELS of [BKP pixel rows][128 bytes] (64 bf16 / 32 f32 columns), the same
  // shape as the gconv tiles: a wave instruction of the direct-to-LDS load fills 8 rows of one panel linearly and
  // every thread owns ONE pixel row (all its pieces are that pixel at different column panels), so the gather
  // coordinates are advanced once per thread and K step.
  constexpr int PANEL = BKP * 128;
  constexpr int CPP = 128 / SZ;                             // columns per panel
  constexpr int GROUPS = NT / (8 * BKP);                    // 1 (bf16) / 2 (f32) thread groups per row set
  constexpr int NPG = TN / CPP;                             // gather panels: 4 / 8
  constexpr int PPT = NPG / GROUPS;                         // gather pieces per thread
  static_assert(PPT == 4, "four gather pieces per thread");
  constexpr bool kNarrowA = TM == 32 && SZ == 2;            // rows tile [64][64 B]: half-panel rows, own mapping
  constexpr int NPA = kNarrowA ? 1 : (TM / CPP);            // rows-operand panels
  constexpr int PPTA = kNarrowA ? 1 : (NPA >= GROUPS ? NPA / GROUPS : 1);
  constexpr int TILEA = kNarrowA ? BKP * 64 : NPA * PANEL;
  constexpr int TILE = NPG * PANEL;
  constexpr int STAGE = TILE + TILEA;
  constexpr int NSTAGE = TM == 256 ? 2 : 3;
  constexpr int NLOADS = PPT + PPTA;
  constexpr unsigned kOOB = 0xFFFFFFF0u;

  extern __shared__ float4 smem_raw[];
  char* smem = reinterpret_cast<char*>(smem_raw);
  // loop-resident descriptor fields in registers (see gconv_kernel)
  const int Hg = d.Hg, Wg = d.Wg, Hin = d.Hin, Win = d.Win, Cpi = d.Cp_in, sh = d.sh, sw = d.sw, pad_mode = d.pad_mode, KK = d.KK;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  // 1-D launch of grid_nx (column tiles) x grid_my (row tiles) x grid_sp (pixel splits) workgroups.  Which tile a workgroup
  // takes decides what shares an XCD's L2: workgroups are dealt round-robin over the 8 XCDs (speed only, never
  // correctness), so physical id -> logical index L puts a CONTIGUOUS run of L on each XCD (bijective chunk remap), and L
  // orders the tiles so that neighbours stream the same bytes at the same time: same pixel split first, then the same
  // input-channel slice (column tiles jx = tap * slices + slice read the same pixels of the gathered tensor through
  // different taps), then tap, then row tile (same rows-operand panel).  The 243 workgroups of a trunk layer then read
  // each activation panel from memory about twice instead of 8 times (measured: DESIGN section 6).
  int bx, by, bz;
  {
    const int W = grid_nx * grid_my * grid_sp;
    int L = (int)blockIdx.x;
    if (xcd_order) {
      const int q = W >> 3, r = W & 7, xcd = L & 7, k = L >> 3;
      L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
      by = L % grid_my;
      const int u = L / grid_my;
      const int slices = (d.Cp_in * SZ) % (TN * SZ) == 0 ? d.Cp_in / TN : 0;
      if (slices > 0 && grid_nx % slices == 0 && grid_nx * TN == d.KK) {
        const int taps = grid_nx / slices;
        const int t = u % taps, v = u / taps;
        bx = t * slices + v % slices;
        bz = v / slices;
      } else {
        bx = u % grid_nx;
        bz = u / grid_nx;
      }
    } else {
      bx = L % grid_nx;
      by = (L / grid_nx) % grid_my;
      bz = L / (grid_nx * grid_my);
    }
  }
  const int j0 = bx * TN;                                   // first kk column
  const int m0 = by * TM;                                   // first output row
  const int npix = Hg * Wg;
  const long P = (long)d.N * npix;
  const int total_steps = (int)((P + BKP - 1) / BKP);
  const int s_begin = bz * steps_per_split;
  int s_end = s_begin + steps_per_split;
  if (s_end > total_steps) s_end = total_steps;
  const int nsteps = s_end - s_begin;                       // >= 1 by construction of the grid

  // this thread's pixel row, slot and panel group; bf16 tiles are read back with the transposing ds_read_b64_tr_b16,
  // whose 32-lane half touches 4 pixel rows x 64 B at a 128-byte row pitch: rows 2,3 (mod 4) are moved to the other
  // half of the row by XORing the 16-byte chunk index with 4 (applied to the SOURCE column, the LDS side is linear)
  const int row = (tid >> 3) & (BKP - 1), slot = tid & 7, grp = tid / (8 * BKP);
  const int chunk = SZ == 2 ? (slot ^ (((row >> 1) & 1) << 2)) : slot;
  const int wrow8 = 8 * (wave % (BKP / 8));                 // first tile row of this wave's instruction
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const auto rsG = __builtin_amdgcn_make_buffer_rsrc((void*)gat, 0, (int)d.in_bytes, 0x00020000);
  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)rows, 0, (int)rows_bytes, 0x00020000);

  // gather pieces: column -> (tap, channel), fixed per thread
  const int T_taps = d.nth * d.ntw;
  int g_dh[PPT], g_dw[PPT];
  unsigned g_cB[PPT];
  bool g_ok[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int kk = j0 + (grp * PPT + j) * CPP + chunk * EPP;
    const int t = kk / Cpi;
    g_ok[j] = t < T_taps;
    const int ta = t / d.ntw, tb = t - ta * d.ntw;
    g_dh[j] = d.dh0 + ta * d.dh_step; g_dw[j] = d.dw0 + tb * d.dw_step;
    g_cB[j] = (unsigned)((kk - t * Cpi) * SZ);
  }
  unsigned g_offB[PPT];                                       // (dh * Win + dw) * bytes per pixel + channel offset, mod 2^32
#pragma unroll
  for (int j = 0; j < PPT; ++j) g_offB[j] = (unsigned)(g_dh[j] * Win + g_dw[j]) * (unsigned)(Cpi * SZ) + g_cB[j];
  const bool same_tap = g_ok[0] && g_ok[PPT - 1] && g_dh[0] == g_dh[PPT - 1] && g_dw[0] == g_dw[PPT - 1] &&
                        (j0 + (grp * PPT) * CPP + chunk * EPP) / Cpi == (j0 + (grp * PPT + PPT - 1) * CPP + chunk * EPP) / Cpi;
  // rows-operand pieces
  unsigned a_cB[PPTA];
  bool a_ok[PPTA];
  int rowA = row;
  int waveA8 = wrow8;
  if constexpr (kNarrowA) {
    const int tidA = tid & 255;
    rowA = tidA >> 2;
    const int mcol = m0 + (tidA & 3) * EPP;
    a_ok[0] = mcol < Cp_r; a_cB[0] = (unsigned)(mcol * SZ);
    waveA8 = 16 * (wave & 3);
  } else {
#pragma unroll
    for (int j = 0; j < PPTA; ++j) {
      const int panel = NPA >= GROUPS ? grp * PPTA + j : 0;
      const int mcol = m0 + panel * CPP + chunk * EPP;
      a_ok[j] = mcol < Cp_r; a_cB[j] = (unsigned)(mcol * SZ);
    }
  }
  const unsigned CpiB = (unsigned)(Cpi * SZ), CprB = (unsigned)(Cp_r * SZ);

  // pixel of this thread's row, advanced by BKP per K step
  long pcur = (long)s_begin * BKP + row;
  int pn, ph, pw;
  {
    const long nn = pcur / npix;
    const int rem = (int)(pcur - nn * npix);
    pn = (int)nn; ph = rem / Wg; pw = rem - ph * Wg;
  }
  long pA = (long)s_begin * BKP + rowA;
  unsigned aB = (unsigned)pA * CprB;                          // byte offset of this thread's rows-operand pixel, advanced per step
  unsigned vG[PPT], vA[PPTA];
  // one K step moves the pixel by BKP: as (samples, rows, columns) so the walk is three adds with carries, no loops
  const int adv_n = BKP / npix, adv_rem = BKP - adv_n * npix;
  const int adv_h = adv_rem / Wg, adv_w = adv_rem - adv_h * Wg;
  const bool reflect = pad_mode == 1;
  // 24-bit multiplies are full rate (v_mad_u32_u24); the host guarantees N * Hin * Win < 2^31 and Hin, Win < 2^24
  auto pix_off = [&](int dh, int dw) -> unsigned {
    int hi = __mul24(ph, sh) + dh, wi = __mul24(pw, sw) + dw;
    if (reflect) {                                              // branch-free |.| and mirror at the far edge
      hi = hi < 0 ? -hi : hi; hi = hi >= Hin ? 2 * (Hin - 1) - hi : hi;
      wi = wi < 0 ? -wi : wi; wi = wi >= Win ? 2 * (Win - 1) - wi : wi;
    }
    const bool ok = (unsigned)hi < (unsigned)Hin && (unsigned)wi < (unsigned)Win;
    const unsigned pix = (unsigned)(__mul24(pn, Hin) + hi) * (unsigned)Win + (unsigned)wi;
    return ok ? pix * CpiB : kOOB;
  };
  auto prepare = [&]() {
    if (pcur < P) {
      if (same_tap) {
        const unsigned o = pix_off(g_dh[0], g_dw[0]);
#pragma unroll
        for (int j = 0; j < PPT; ++j) vG[j] = o == kOOB ? kOOB : o + g_cB[j];
      } else if (!reflect) {
        // zero padding: every tap is the un-shifted pixel plus a per-piece constant; only the bounds test is per tap
        const int hb = __mul24(ph, sh), wb = __mul24(pw, sw);
        const unsigned baseB = ((unsigned)(__mul24(pn, Hin) + hb) * (unsigned)Win + (unsigned)wb) * CpiB;
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const bool ok = g_ok[j] && (unsigned)(hb + g_dh[j]) < (unsigned)Hin && (unsigned)(wb + g_dw[j]) < (unsigned)Win;
          vG[j] = ok ? baseB + g_offB[j] : kOOB;
        }
      } else {
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
          const unsigned o = g_ok[j] ? pix_off(g_dh[j], g_dw[j]) : kOOB;
          vG[j] = o == kOOB ? kOOB : o + g_cB[j];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < PPT; ++j) vG[j] = kOOB;
    }
#pragma unroll
    for (int j = 0; j < PPTA; ++j) vA[j] = (a_ok[j] && pA < P) ? aB + a_cB[j] : kOOB;
    pcur += BKP; pA += BKP; aB += (unsigned)BKP * CprB;
    pw += adv_w;
    const int cw = pw >= Wg ? 1 : 0;
    pw -= cw ? Wg : 0;
    ph += adv_h + cw;
    const int ch = ph >= Hg ? 1 : 0;
    ph -= ch ? Hg : 0;
    pn += adv_n + ch;
  };
  // piece j of a tile: 0..3 gather panels, 4.. rows-operand panels
  P2PHD_CW_DECL;
  auto issue_piece = [&](int slot_, int j) {
    char* A = smem + slot_ * STAGE;
    P2PHD_CW_ISSUE(slot_);
    if (j < PPT) {
      char* G = A + TILEA + (grp * PPT + j) * PANEL + wrow8 * 128;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsG, (lds_ptr)G, 16, (int)vG[j], 0, 0, 0);
    } else {
      char* Aw;
      if constexpr (kNarrowA) Aw = A + waveA8 * 64;
      else Aw = A + (NPA >= GROUPS ? grp * PPTA + (j - PPT) : 0) * PANEL + waveA8 * 128;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_ptr)Aw, 16, (int)vA[j - PPT], 0, 0, 0);
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  // transposing LDS read: 16-lane group g reads a 4-pixel x 16-channel block, lane i gets channel i; lane 4q+p of the
  // group supplies row (8h + q), 8-byte column unit u = 4*(g&1) + p of the 32-column block (u>>1 = 16-B chunk)
  const int g16 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, pq = i16 & 3, hh = g16 >> 1;
  const int u8 = 4 * (g16 & 1) + pq;
  const int swzq = ((q4 >> 1) & 1) << 2;
  constexpr int RPA = kNarrowA ? 64 : 128;                  // row pitch of the rows-operand tile
  unsigned ta_off[MI], tg_off[NI];                          // byte offsets (within a stage) of the sub = 0 reads
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int mb = wm * (MI * 32) + i * 32;
    if constexpr (kNarrowA) ta_off[i] = (unsigned)((8 * hh + q4) * 64 + ((u8 >> 1) << 4) + 8 * (u8 & 1));
    else ta_off[i] = (unsigned)((mb / CPP) * PANEL + (8 * hh + q4) * 128 + (((((mb % CPP) >> 3) + (u8 >> 1)) ^ swzq) << 4) + 8 * (u8 & 1));
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int nb = wn * (NI * 32) + j * 32;
    tg_off[j] = (unsigned)(TILEA + (nb / CPP) * PANEL + (8 * hh + q4) * 128 + (((((nb % CPP) >> 3) + (u8 >> 1)) ^ swzq) << 4) + 8 * (u8 & 1));
  }

  if constexpr (SZ == 2) {
    // Same pipeline as gconv_kernel's main loop: one barrier per K step, in front of its last MFMA cluster; the next
    // tile's first fragments and the LDS-DMA of tile s + NSTAGE (into the slot just drained) go out in the MFMA shadow.
    uint2 af[2][MI][2], gf[2][NI][2];
    // the k sub-step and the second half of a fragment ride on the instruction's immediate offset: one address VGPR
    // per fragment and K step instead of one add per read (`sub` is a literal after unrolling, the switch folds away)
#define P2PHD_TR_READ(dst, addr, OFF) \
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF))
#define P2PHD_TR_PAIR(lo, hi, addr, SUB, PITCH)                                                        \
  do {                                                                                                 \
    P2PHD_TR_READ(lo, addr, 16 * (SUB) * (PITCH));                                                     \
    P2PHD_TR_READ(hi, addr, 16 * (SUB) * (PITCH) + 4 * (PITCH));                                       \
  } while (0)
    auto read_frags = [&](unsigned so, int sub, int buf) {
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const unsigned ad = so + ta_off[i];
        switch (sub) {
          case 0: P2PHD_TR_PAIR(af[buf][i][0], af[buf][i][1], ad, 0, RPA); break;
          case 1: P2PHD_TR_PAIR(af[buf][i][0], af[buf][i][1], ad, 1, RPA); break;
          case 2: P2PHD_TR_PAIR(af[buf][i][0], af[buf][i][1], ad, 2, RPA); break;
          default: P2PHD_TR_PAIR(af[buf][i][0], af[buf][i][1], ad, 3, RPA); break;
        }
      }
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const unsigned ad = so + tg_off[j];
        switch (sub) {
          case 0: P2PHD_TR_PAIR(gf[buf][j][0], gf[buf][j][1], ad, 0, 128); break;
          case 1: P2PHD_TR_PAIR(gf[buf][j][0], gf[buf][j][1], ad, 1, 128); break;
          case 2: P2PHD_TR_PAIR(gf[buf][j][0], gf[buf][j][1], ad, 2, 128); break;
          default: P2PHD_TR_PAIR(gf[buf][j][0], gf[buf][j][1], ad, 3, 128); break;
        }
      }
    };
    static_assert(BKP / 16 <= 4, "sub-step switch covers 4 k sub-steps");
    auto mfma_one = [&](int buf, int i, int j) {
      bf16x8 a8, g8;
      uint2* ap = reinterpret_cast<uint2*>(&a8);
      uint2* gp = reinterpret_cast<uint2*>(&g8);
      ap[0] = af[buf][i][0]; ap[1] = af[buf][i][1];
      gp[0] = gf[buf][j][0]; gp[1] = gf[buf][j][1];
      acc[i][j] = p2phd_mfma_32x32x16(a8, g8, acc[i][j]);
    };
    constexpr int NSUB = BKP / 16;
#ifdef P2PHD_PROBE
    const unsigned long long pr_t0 = __builtin_readcyclecounter();
    unsigned long long pr_wait = 0, pr_bar = 0;
#endif
#pragma unroll
    for (int t = 0; t < NSTAGE; ++t) {
      if (t < nsteps) {
        prepare();
#pragma unroll
        for (int j = 0; j < NLOADS; ++j) issue_piece(t, j);
      }
    }
    if (nsteps >= NSTAGE) {
      P2PHD_CW_WAIT(CW_WGRAD, (NSTAGE - 1) * NLOADS, 1u << 0);
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 1) * NLOADS) : "memory");
    } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    read_frags(sbase, 0, 0);
    int cur = 0;
    bool pend = false;
    int pend_slot = 0;
    for (int s = 0; s < nsteps; ++s) {
      const unsigned so = sbase + (unsigned)(cur * STAGE);
      const int nslot = cur == NSTAGE - 1 ? 0 : cur + 1;
      const bool has_next = s + 1 < nsteps;
      const bool issue_new = s + NSTAGE < nsteps;
#pragma unroll
      for (int sub = 0; sub < NSUB; ++sub) {
        const int buf = sub & 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (sub == NSUB - 1 && has_next) {
#ifdef P2PHD_PROBE
          const unsigned long long q0 = __builtin_readcyclecounter();
#endif
          if (NSTAGE > 2 && s + NSTAGE - 1 < nsteps) {
            P2PHD_CW_WAIT(CW_WGRAD, (NSTAGE - 2) * NLOADS, 1u << nslot);
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NSTAGE - 2) * NLOADS) : "memory");
          } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef P2PHD_PROBE
          const unsigned long long q1 = __builtin_readcyclecounter();
#endif
          __builtin_amdgcn_s_barrier();
#ifdef P2PHD_PROBE
          pr_wait += q1 - q0; pr_bar += __builtin_readcyclecounter() - q1;
#endif
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_one(buf, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (sub < NSUB - 1) read_frags(so, sub + 1, buf ^ 1);
        else if (has_next) read_frags(sbase + (unsigned)(nslot * STAGE), 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (MI * NI > 1) mfma_one(buf, 1 / NI, 1 % NI);
        __builtin_amdgcn_sched_barrier(0);
        if (sub == 0 && pend) {
#pragma unroll
          for (int j = 1; j < NLOADS; j += 2) issue_piece(pend_slot, j);
          pend = false;
        }
        if (sub == NSUB - 1 && issue_new) {
          prepare();
#pragma unroll
          for (int j = 0; j < NLOADS; j += 2) issue_piece(cur, j);
          pend = true; pend_slot = cur;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            if (i * NI + j >= (MI * NI > 1 ? 2 : 1)) mfma_one(buf, i, j);
        __builtin_amdgcn_sched_barrier(0);
      }
      cur = nslot;
    }
#ifdef P2PHD_PROBE
    if (tid == 0) {
      const unsigned wg = (unsigned)blockIdx.x % kProbeSlots;
      unsigned long long* r = g_probe + (size_t)wg * 8;
      r[0] += pr_wait; r[1] += pr_bar; r[2] += __builtin_readcyclecounter() - pr_t0; r[3] += (unsigned long long)nsteps;
      r[6] += 1ull;
    }
#endif
  } else {
    // f32 (parity runs): plain LDS reads; hipcc drains the DMA queue in front of them, which is correct, just slower
    auto compute = [&](int slot_, bool pf, int pf_slot) {
      if (pf) {
        prepare();
#pragma unroll
        for (int j = 0; j < NLOADS; ++j) issue_piece(pf_slot, j);
      }
      const char* A = smem + slot_ * STAGE;
      const char* G = A + TILEA;
      const int lr = lane & 31, lh = lane >> 5;
#pragma unroll 4
      for (int s2 = 0; s2 < BKP / 2; ++s2) {
        const int prow = 2 * s2 + lh;
        float af[MI], gf[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const int col = wm * (MI * 32) + i * 32 + lr;
          af[i] = *reinterpret_cast<const float*>(A + (col / CPP) * PANEL + prow * 128 + (col % CPP) * 4);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          const int col = wn * (NI * 32) + j * 32 + lr;
          gf[j] = *reinterpret_cast<const float*>(G + (col / CPP) * PANEL + prow * 128 + (col % CPP) * 4);
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], gf[j], acc[i][j], 0, 0, 0);
      }
    };
    constexpr int D = NSTAGE - 1;
#pragma unroll
    for (int t = 0; t < D; ++t) {
      if (t < nsteps) {
        prepare();
#pragma unroll
        for (int j = 0; j < NLOADS; ++j) issue_piece(t, j);
      }
    }
    int cur = 0, nxt = D;
    for (int s = 0; s < nsteps; ++s) {
      if (D >= 2 && s + 1 < nsteps) {
        P2PHD_CW_WAIT(CW_WGRAD_F32, NLOADS, 1u << cur);          // this step's slot is read behind the barrier
        asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NLOADS) : "memory");
      } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      compute(cur, s + D < nsteps, nxt);
      cur = cur == NSTAGE - 1 ? 0 : cur + 1;
      nxt = nxt == NSTAGE - 1 ? 0 : nxt + 1;
    }
  }

  P2PHD_CW_DONE();
  float* slab = dwp + (size_t)bz * slab_elems;
  const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = j0 + wn * (NI * 32) + j * 32 + lr;
      if (col >= KK) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row_o = m0 + wm * (MI * 32) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        slab[(size_t)row_o * KK + col] = acc[i][j][e];
      }
    }
}

}  // namespace

namespace p2phd {

template <typename T, int TM>
void launch_wgrad_cfg(const GDesc& d, const void* rows, const void* gat, float* dwp, int Cp_r, int mrows, int sps, int splits,
                      long slab_elems, unsigned rows_bytes, hipStream_t st) {
  constexpr int bkp = sizeof(T) == 2 ? 64 : 32;
  constexpr int tilea = (TM == 32 && sizeof(T) == 2) ? bkp * 64 : (TM * (int)sizeof(T) / 128 > 0 ? TM * (int)sizeof(T) / 128 : 1) * bkp * 128;
  constexpr int lds = (TM == 256 ? 2 : 3) * (256 * (int)sizeof(T) / 128 * bkp * 128 + tilea);
  auto kern = wgrad_kernel<T, TM>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  const int nx = (d.KK + 255) / 256, my = mrows / TM;
  ++p2phd::g_launch_count[p2phd::LC_WGRAD];
  hipLaunchKernelGGL(kern, dim3((unsigned)(nx * my * splits)), dim3(512), lds, st, d, (const T*)rows, (const T*)gat, dwp, Cp_r, sps, slab_elems,
                     rows_bytes, nx, my, splits, p2phd::g_opt_wgrad_xcd);
}

// Split plan of the pixel reduction: shared by the workspace query and the launch.
void wgrad_split_plan(const GDesc& d, int dtype, int M_rows, int M_rows_pad, int* tm, int* mrows, int* splits, int* sps) {
  const long P = (long)d.N * d.Hg * d.Wg;
  const int bkp = dtype == P2PHD_BF16 ? 64 : 32;
  const int total_steps = (int)std::max<long>(1, (P + bkp - 1) / bkp);
  // row tile: 32 for folded 2-channel layers, 256 (wave tile 128 x 64: twice the MFMA work per LDS-DMA piece) when
  // the output rows fill it, else 128
  *tm = M_rows <= 32 ? 32 : ((M_rows % 256 == 0 || M_rows >= 1024) ? 256 : 128);
  if (g_opt_wgrad_tm == 128 && *tm == 256) *tm = 128;
  *mrows = *tm == 32 ? 32 : round_up(M_rows_pad, *tm);
  const int tiles = (*mrows / *tm) * ((d.KK + 255) / 256);
  // Split of the pixel reduction over blockIdx.z: one 8-wave workgroup per CU, so the grid runs in
  // ceil(tiles * sp / 256) rounds of ceil(total_steps / sp) K steps; every extra split costs one more slab to write
  // and to sum.  Pick the cheapest under a 256 MiB workspace.
  const double t_step = *tm == 256 ? 0.9e-6 : (*tm == 128 ? 0.5e-6 : 0.25e-6);
  const double slab_bytes = (double)*mrows * d.KK * sizeof(float);
  int best = 1;
  double best_cost = 1e30;
  for (int sp = 1; sp <= 512; ++sp) {
    if (sp > 1 && (total_steps / sp < 4 || slab_bytes * sp > (double)(256u << 20))) break;
    const double rounds = std::ceil((double)tiles * sp / 256.0);
    const double cost = rounds * std::ceil((double)total_steps / sp) * t_step + sp * slab_bytes * 2.0 / 4.0e12 + 2e-6;
    if (cost < best_cost) { best_cost = cost; best = sp; }
  }
  *sps = (total_steps + best - 1) / best;
  *splits = (total_steps + *sps - 1) / *sps;
}

size_t wgrad_workspace_floats(const GDesc& d, int dtype, int M_rows, int M_rows_pad) {
  int tm, mrows, splits, sps;
  wgrad_split_plan(d, dtype, M_rows, M_rows_pad, &tm, &mrows, &splits, &sps);
  return (size_t)splits * mrows * d.KK;
}

int launch_wgrad(const GDesc& d_in, const WMap& m, int dtype, const void* rows, int Cp_r, int M_rows, int M_rows_pad,
                 const void* gat, float* dwp, float* dw, int accumulate, hipStream_t st) {
  // dwp: wgrad_workspace_floats() floats; dw: master-layout gradient (overwritten)
  GDesc d = d_in;
  const long P = (long)d.N * d.Hg * d.Wg;
  const size_t esz = dtype == P2PHD_BF16 ? 2 : 4;
  const size_t gb = (size_t)d.N * d.Hin * d.Win * d.Cp_in * esz, rbytes = (size_t)P * Cp_r * esz;
  P2PHD_REQUIRE(gb < 0xFFFFFFF0ull && rbytes < 0xFFFFFFF0ull, "wgrad: tensor larger than 4 GiB");
  d.in_bytes = (unsigned)gb;
  int tm, mrows, splits, sps;
  wgrad_split_plan(d, dtype, M_rows, M_rows_pad, &tm, &mrows, &splits, &sps);
  const long slab = (long)mrows * d.KK;
  if (P == 0) {
    (void)hipMemsetAsync(dwp, 0, sizeof(float) * (size_t)slab, st);
    splits = 1;
  } else if (dtype == P2PHD_BF16 || dtype == P2PHD_F32) {
    FOR_ELEM(dtype, T, {
      if (tm == 32) launch_wgrad_cfg<T, 32>(d, rows, gat, dwp, Cp_r, mrows, sps, splits, slab, (unsigned)rbytes, st);
      else if (tm == 256) launch_wgrad_cfg<T, 256>(d, rows, gat, dwp, Cp_r, mrows, sps, splits, slab, (unsigned)rbytes, st);
      else launch_wgrad_cfg<T, 128>(d, rows, gat, dwp, Cp_r, mrows, sps, splits, slab, (unsigned)rbytes, st);
    });
  } else {
    set_error("wgrad: unsupported dtype %d", dtype);
    return P2PHD_EUNSUPPORTED;
  }
  if (int rc = check_launch("wgrad")) return rc;
  if (m.rows > 0 && m.inner > 0) launch_unpack_grad(d, m, dwp, dw, splits, slab, accumulate, st);
  return check_launch("unpack_grad");
}

#ifdef P2PHD_CHECK_WAITS
bool wgrad_wait_flag(unsigned* out4, int reset) {
  if (out4 != nullptr && hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_cw_flag), sizeof(unsigned) * 4) != hipSuccess) return false;
  const unsigned z[4] = {0, 0, 0, 0};
  return !reset || hipMemcpyToSymbol(HIP_SYMBOL(g_cw_flag), z, sizeof(z)) == hipSuccess;
}
#endif

#ifdef P2PHD_PROBE
int wgrad_probe_add(unsigned long long* out8, int reset) {
  static unsigned long long host[kProbeSlots * 8];
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_probe), sizeof(host)) != hipSuccess) return -1;
  for (int i = 0; i < kProbeSlots; ++i)
    for (int k = 0; k < 8; ++k) out8[k] += host[(size_t)i * 8 + k];
  void* dp = nullptr;
  if (reset && (hipGetSymbolAddress(&dp, HIP_SYMBOL(g_probe)) != hipSuccess || hipMemset(dp, 0, sizeof(host)) != hipSuccess)) return -1;
  return 0;
}
#endif

}  // namespace p2phd
