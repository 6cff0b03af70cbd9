// -DP2PHD_CHECK_WAITS (libp2phd_hip_chk.so, tests/test_gpu_waits.py): a checker for the hand-counted waits of the LDS-DMA
// pipelines.  `s_waitcnt vmcnt(n)` lets the wave's n YOUNGEST vector-memory operations stay in flight; a relaxed wait in
// front of a slab barrier is correct only if none of those n targets a buffer that ANY wave reads behind the barrier.  That is a
// statement about the issue order of every wave, and one wave that issued fewer pieces than its neighbours (round 4: the last
// halo rows belong to waves 0 and 1 only) breaks it without any test noticing on most runs.  In this build every wave logs the
// buffer id of each piece it issues (a 64-bit shift register of 4-bit tags, wave-uniform: scalar registers) and, at every
// relaxed wait, looks at the n youngest tags: a tag inside the `forbid` set raises a device flag (p2phd_wait_check).
// The product build compiles all of it away.
// The flag is a `__device__` array, and without relocatable device code two code objects cannot share one: gconv.hip and wgrad.hip
// each get their own copy (internal linkage), which p2phd_wait_check (gconv.hip) merges.
#pragma once
#include "common.h"

namespace {

#ifdef P2PHD_CHECK_WAITS
__device__ unsigned g_cw_flag[4];     // [0] violations (bit mask of kernel families), [1] relaxed waits checked, [2] first offending (family << 16 | n << 8 | tag), [3] pieces logged
#define P2PHD_CW_DECL unsigned long long cw_log = ~0ull; unsigned cw_pieces = 0
#define P2PHD_CW_ISSUE(tag) do { cw_log = (cw_log << 4) | (unsigned long long)((tag) & 15); ++cw_pieces; } while (0)
#define P2PHD_CW_WAIT(family, n, forbid)                                                                            \
  do {                                                                                                              \
    if ((lane) == 0) {                                                                                              \
      atomicAdd(&g_cw_flag[1], 1u);                                                                                 \
      for (int cw_k = 0; cw_k < (n) && cw_k < 16; ++cw_k) {                                                         \
        const unsigned cw_t = (unsigned)(cw_log >> (4 * cw_k)) & 15u;                                               \
        if (cw_t != 15u && (((forbid) >> cw_t) & 1u)) {                                                             \
          atomicOr(&g_cw_flag[0], 1u << (family));                                                                  \
          atomicCAS(&g_cw_flag[2], 0u, ((unsigned)(family) << 16) | ((unsigned)(n) << 8) | cw_t);                   \
        }                                                                                                           \
      }                                                                                                             \
    }                                                                                                               \
  } while (0)
#define P2PHD_CW_DONE() do { if ((lane) == 0 && cw_pieces) atomicAdd(&g_cw_flag[3], cw_pieces); } while (0)
#else
#define P2PHD_CW_DECL
#define P2PHD_CW_ISSUE(tag) do { } while (0)
#define P2PHD_CW_WAIT(family, n, forbid) do { } while (0)
#define P2PHD_CW_DONE() do { } while (0)
#endif
enum { CW_GCONV = 0, CW_HALO = 1, CW_WGRAD = 2, CW_WGRAD_F32 = 3 };

}  // namespace

#ifdef P2PHD_CHECK_WAITS
namespace p2phd {
// wgrad.hip: its copy of the flag -- copied to out4 (unless null), then cleared if `reset`; false: the runtime refused
bool wgrad_wait_flag(unsigned* out4, int reset);
}  // namespace p2phd
#endif
