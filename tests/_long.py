"""Cases, inputs and vectorised references of the tests that run the grid-stride kernels PAST their workgroup cap
(tests/test_long_host.py on the CPU, tests/test_gpu_long.py on the GPU).

A streaming kernel launches min(cdiv(items, 256), cap) workgroups and walks the rest with `e += gridDim.x * blockDim.x`.  Every
case here is about 2.5 trips of the whole grid plus an odd remainder: some threads take three trips, some two, and the last quad
or piece is incomplete.  The grids are the figures of the code as it stands (GRIDS below, pinned against p2phd_stream_grid by
test_long_host.py); the sizes are computed from those figures, never from the library, so a changed cap shows as a failing case
and not as a case that quietly runs one trip again.

Inputs identify their position: a 32-bit hash of the index (no period that could divide grid * 256), so an element taken from
another trip's position is another number.  The references are the existing restatements' definitions, vectorised: each is pinned
to its restatement at that restatement's small shapes by test_long_host.py."""
import ctypes

import numpy as np

F32, H16 = 0, 1                                                     # dtype codes of include/p2phd.h (H16: the library's 16-bit type)

# family -> (cap in workgroups, work units per thread and trip for (f32, 16-bit), items per thread for (f32, 16-bit)):
# wanted = cdiv(cdiv(work, items), 256), used = min(wanted, cap), unit_work = used * 256 * per-trip
GRIDS = {
    "segments_gather": (16384, (4, 4)), "segments_gather_planar": (16384, (4, 4)),
    "segments_stitch": (16384, (4, 4)), "segments_stitch_planar": (16384, (4, 4)),
    "pcm_decode": (16384, (1, 1)), "pcm_encode": (16384, (1, 1)), "pcm_encode_ex": (16384, (1, 1)),
    "stereo_matrix": (4096, (4, 4)), "stereo_matrix_scalar": (4096, (1, 1)),
    "loudness_blocks": (2048, (1, 1)), "loudness_short_term": (2048, (1, 1)),
    "avgpool3s2_fwd": (8192, (1, 1)), "avgpool3s2_bwd": (8192, (1, 1)), "nchw_to_nhwc": (8192, (1, 1)),
    "nhwc_to_nchw": (8192, (1, 1)), "nchw_cat_to_nhwc": (8192, (1, 1)),
    "act_bwd": (8192, (4, 8)),
    "adam_step": (4096, (4, 4)), "adam_step_dev": (4096, (4, 4)), "adam_step_scaled": (4096, (4, 4)),
    "timed_pack_pair": (16384, (4, 4)),
    "spectro_encode": (8192, (1, 1)), "spectro_encode_ex": (8192, (1, 1)), "spectro_stats": (1024, (1, 1)),
    "spectro_range_scalar": (1024, (1, 1)), "range_fold_scalar": (1024, (1, 1)),
}
# families whose thread has several pieces in flight, or whose grid is sized in another unit than a thread's piece:
#   grads_nonfinite: cdiv(n, 4) float4 on 2048 workgroups, four in flight -> a trip is used * 256 * 16 floats
#   loss_fwd / loss_bwd: the grid from P * Cp / 8 on 1024 / 2048 workgroups, four 16-byte pieces in flight -> used * 256 * 4 * epp
#   spectro_range / range_fold (aligned): n / 4 + n % 4 items on 1024 workgroups, a trip is used * 256 float4
#   pcm_peak: cdiv(frames / 4, 1024) on min(2048 / channels, scratch 5 * 65536 / (5 * channels)), a trip used * 256 * 16 frames


def cdiv(a, b):
    return -(-a // b)


def expected_grid(family, dtype, work, rows=1):
    """(unit_work, wanted, used) by today's figures."""
    e = 8 if dtype == H16 else 4
    if family == "pcm_peak":
        cap = min(max(1, 2048 // rows), (5 << 16) // (5 * rows))
        wanted = max(1, cdiv(work // 4, 1024))
        used = max(1, min(wanted, cap))
        return used * 256 * 16, wanted, used
    if family == "grads_nonfinite":
        items, cap, per = cdiv(work, 4), 2048, 16
    elif family in ("loss_fwd", "loss_bwd"):
        items, cap, per = work // 8, 1024 if family == "loss_fwd" else 2048, 4 * e
    elif family in ("spectro_range", "range_fold"):
        items, cap, per = work // 4 + work % 4, 1024, 4
    else:
        cap, pers = GRIDS[family]
        per = pers[1 if dtype == H16 else 0]
        items = work // per if family == "act_bwd" else cdiv(work, per)      # (act_bwd takes whole pieces only)
    wanted = max(1, cdiv(items, 256))
    used = min(wanted, cap)
    return used * 256 * per, wanted, used


ALL_FAMILIES = sorted(list(GRIDS) + ["pcm_peak", "grads_nonfinite", "loss_fwd", "loss_bwd", "spectro_range", "range_fold"])
REDUCING = {"pcm_peak", "grads_nonfinite", "loss_fwd", "spectro_stats", "spectro_range", "range_fold", "spectro_range_scalar",
            "range_fold_scalar"}


def stream_grid(lib, family, dtype, work, rows=1):
    """p2phd_stream_grid (host arithmetic, no device): (return code, unit_work, wanted, used)."""
    unit, wanted, used = ctypes.c_int64(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.p2phd_stream_grid(family.encode(), dtype, work, rows, ctypes.byref(unit), ctypes.byref(wanted), ctypes.byref(used))
    return rc, unit.value, wanted.value, used.value


def long_work(family, dtype=F32, rows=1, odd=1):
    """About 2.5 trips of the capped grid plus an odd remainder (in the family's unit of work)."""
    cap_unit = expected_grid(family, dtype, 1 << 36, rows)[0]
    return 2 * cap_unit + cap_unit // 2 + 2 * 1237 + odd


# (id, family, dtype, rows, work): the cases the GPU module runs.  work is odd, so the last quad / piece is incomplete.
CASES = [
    ("gather_vec_planar", "segments_gather_planar", F32, 2, None),    # work set below: S * T with T a multiple of 4
    ("gather_scalar", "segments_gather", F32, 1, None),               # odd T
    ("stitch_fade_vec", "segments_stitch", F32, 1, long_work("segments_stitch")),
    ("stitch_cat_scalar", "segments_stitch", F32, 1, long_work("segments_stitch")),
    ("pcm_decode", "pcm_decode", F32, 1, None),                       # frames * channels, 3 channels
    ("pcm_encode", "pcm_encode", F32, 1, None),
    ("pcm_encode_ex", "pcm_encode_ex", F32, 1, None),
    ("pcm_peak_c8", "pcm_peak", F32, 8, long_work("pcm_peak", rows=8)),
    ("stereo_vec", "stereo_matrix", F32, 2, long_work("stereo_matrix")),
    ("stereo_scalar", "stereo_matrix_scalar", F32, 2, long_work("stereo_matrix_scalar")),
    ("act_bwd_f32", "act_bwd", F32, 1, None),                          # a multiple of the piece
    ("act_bwd_h16", "act_bwd", H16, 1, None),
    ("nchw_to_nhwc", "nchw_to_nhwc", F32, 1, None),                    # elements C * HW
    ("nhwc_to_nchw", "nhwc_to_nchw", F32, 1, None),                    # 16-byte pieces HW * 2 (Cp = 8 in f32, 16 in 16-bit storage)
    ("stitch_planar", "segments_stitch_planar", F32, 2, long_work("segments_stitch_planar") + 2),
    ("loudness_blocks", "loudness_blocks", F32, 1, long_work("loudness_blocks")),
    ("loudness_short_term", "loudness_short_term", F32, 1, long_work("loudness_blocks") - 26),      # the same J hops: J - 29 blocks
    ("avgpool_fwd", "avgpool3s2_fwd", F32, 1, None),                   # pieces Ho * Wo * Cp / 4
    ("avgpool_bwd_f32", "avgpool3s2_bwd", F32, 1, None),               # pieces H * W * Cp / epp
    ("avgpool_bwd_h16", "avgpool3s2_bwd", H16, 1, None),
    ("nchw_cat_to_nhwc", "nchw_cat_to_nhwc", F32, 1, None),            # pieces HW * 2, as nhwc_to_nchw
    ("loss_fwd_f32", "loss_fwd", F32, 1, None), ("loss_fwd_h16", "loss_fwd", H16, 1, None),         # padded elements P * 72
    ("loss_bwd_f32", "loss_bwd", F32, 1, None), ("loss_bwd_h16", "loss_bwd", H16, 1, None),
    ("pack_pair", "timed_pack_pair", F32, 1, long_work("timed_pack_pair")),
    ("range_fold", "range_fold", F32, 1, long_work("range_fold")),
    ("range_fold_scalar", "range_fold_scalar", F32, 1, long_work("range_fold_scalar")),
    ("spectro_encode", "spectro_encode_ex", F32, 1, None),            # elements channels * M * F of the normalisation pass
    ("spectro_stats", "spectro_stats", F32, 1, None),                  # elements channels * mask_rows * F of the noise rows
    ("spectro_range", "spectro_range", F32, 1, None),                  # floats F * M
    ("adam_step", "adam_step", F32, 1, long_work("adam_step")),
    ("adam_step_dev", "adam_step_dev", F32, 1, long_work("adam_step_dev")),
    ("adam_step_scaled", "grads_nonfinite", F32, 1, long_work("grads_nonfinite")),   # (then Adam's own grid is past 5 trips)
]
# the shapes behind the cases whose work is a product
GATHER_VEC = dict(T=4096, stride=3072, S=cdiv(long_work("segments_gather_planar"), 4096))
GATHER_SCALAR = dict(T=4099, stride=4099, S=cdiv(long_work("segments_gather"), 4099))
PCM_CHANNELS = 3
PCM_FRAMES = cdiv(long_work("pcm_decode"), PCM_CHANNELS) | 1
LAYOUT_C = 5                                                        # valid channels, at channel offset 2 of the pitch
TO_NHWC_HW = cdiv(long_work("nchw_to_nhwc"), LAYOUT_C) | 1
TO_NCHW_HW = cdiv(long_work("nhwc_to_nchw"), 2) | 1
POOL_FWD = dict(N=1, C=8, H=2 * 1621 - 1, W=2 * 1619)                # Ho 1621 (odd H: the last window is whole), Wo 1619 (even W)
POOL_BWD = dict(N=1, H=1621, W=1619)                               # C = 8 in f32, 16 in 16-bit storage: two pieces per pixel
LOSS_C, LOSS_CP = 67, 72                                            # pad channels: the mask and the piece-column counter are at work
LOSS_P = {F32: cdiv(long_work("loss_bwd", F32), 72) | 1, H16: cdiv(long_work("loss_bwd", H16), 72) | 1}
SPECTRO = dict(B=1, C=2, F=2049, M=1281, mask_rows=160)
ACT_ELEMS = {F32: long_work("act_bwd", F32) // 4 * 4 + 4, H16: long_work("act_bwd", H16) // 8 * 8 + 8}


def case_work(cid):
    """The work of a case, in its family's unit."""
    for c in CASES:
        if c[0] == cid:
            break
    else:
        raise KeyError(cid)
    if c[4] is not None:
        return c[4]
    if cid == "gather_vec_planar":
        return GATHER_VEC["S"] * GATHER_VEC["T"]
    if cid == "gather_scalar":
        return GATHER_SCALAR["S"] * GATHER_SCALAR["T"]
    if cid == "nchw_to_nhwc":
        return LAYOUT_C * TO_NHWC_HW
    if cid == "nhwc_to_nchw":
        return 2 * TO_NCHW_HW
    if cid == "nchw_cat_to_nhwc":
        return 2 * TO_NCHW_HW
    if cid == "avgpool_fwd":
        return POOL_FWD["N"] * 1621 * 1619 * 2
    if cid.startswith("avgpool_bwd"):
        return POOL_BWD["N"] * POOL_BWD["H"] * POOL_BWD["W"] * 2
    if cid.startswith("loss_"):
        return LOSS_P[c[2]] * LOSS_CP
    if cid == "spectro_encode":
        return SPECTRO["C"] * SPECTRO["M"] * SPECTRO["F"]
    if cid == "spectro_stats":
        return SPECTRO["C"] * SPECTRO["mask_rows"] * SPECTRO["F"]
    if cid == "spectro_range":
        return SPECTRO["F"] * SPECTRO["M"]
    if cid.startswith("pcm_"):
        return PCM_FRAMES * PCM_CHANNELS
    return ACT_ELEMS[c[2]]


# ----------------------------------------------------------------------------------------------------------------------
# inputs that identify their position
# ----------------------------------------------------------------------------------------------------------------------
def index_hash(n, seed=0, start=0):
    """uint32[n]: a multiplicative / xor-shift hash (the finaliser of MurmurHash3) of start + i + a seed."""
    h = (np.arange(start, start + n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B1) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    for shift, mult in ((16, 0x85EBCA6B), (13, 0xC2B2AE35)):
        h ^= h >> np.uint64(shift)
        h = (h * np.uint64(mult)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def hashed_floats(n, seed=0, start=0):
    """float32[n] in [-1, 1): 24 bits of the hash, exact."""
    return ((index_hash(n, seed, start) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)).astype(np.float32)


def hashed_small_ints(n, seed=0, start=0, span=64):
    """float32[n] of integers in [-span, span): exact in bf16 and fp16 for span <= 128 (tests/_exact.py's operands)."""
    return ((index_hash(n, seed, start) >> np.uint32(7)) % np.uint32(2 * span)).astype(np.float32) - np.float32(span)


# ----------------------------------------------------------------------------------------------------------------------
# a strided launch, emulated: which elements a launch visits, and how often
# ----------------------------------------------------------------------------------------------------------------------
def strided(fn, work, grid, threads, unit, mutant=None):
    """Emulates `for (q = global thread; q * unit < work; q += grid * threads)`: calls fn(lo, hi, trip) for every trip with the
    first elements lo[] and the ends hi[] of the runs the threads take on that trip, in thread order.  `mutant` breaks the loop
    the way a kernel could be wrong:
      'stride'   the stride forgets the unit factor (a kernel written in elements: e += grid * threads with unit elements taken)
      'one'      one trip only
      'tail'     the partial last trip is dropped
    Returns the number of trips made."""
    G = grid * threads
    items = cdiv(work, unit)
    if mutant == "stride":                                            # element start g * unit + t * G instead of (g + t * G) * unit
        trips = cdiv(work, G)
        made = 0
        for t in range(trips):
            lo = np.arange(G, dtype=np.int64) * unit + t * G
            lo = lo[lo < work]
            if len(lo):
                fn(lo, np.minimum(lo + unit, work), t)
                made += 1
        return made
    trips = cdiv(items, G)
    if mutant == "one":
        trips = min(trips, 1)
    if mutant == "tail" and items % G:
        trips -= 1
    for t in range(trips):
        q = np.arange(t * G, min((t + 1) * G, items), dtype=np.int64)
        fn(q * unit, np.minimum((q + 1) * unit, work), t)
    return trips


def visits(work, grid, threads, unit, mutant=None):
    """int16[work]: how often every element is visited.  A correct launch visits each exactly once: a map kernel that misses one
    leaves the sentinel, an in-place one (Adam) or a reducing one that visits one twice applies or counts it twice."""
    count = np.zeros(work + 1, dtype=np.int32)

    def mark(lo, hi, trip):
        count[lo] += 1                                                # (the runs of one trip start at distinct elements; ends coincide only
        count[hi] -= 1                                                #  at `work`, whose slot is dropped below)
    strided(mark, work, grid, threads, unit, mutant)
    return np.cumsum(count[:-1]).astype(np.int16)


def strided_sum(x, grid, threads, unit, in_flight=1, mutant=None):
    """A reducing kernel emulated in int64 over integer data x: per-thread accumulators over the trips, `in_flight` pieces
    requested per trip with the index clamped to the last piece (as pcm_peak_kernel, loss_fwd_kernel), a clamped piece skipped.
      'clamp'    the clamped tail piece is counted
      'reset'    the accumulator is initialised inside the loop (only the last trip of a thread survives)"""
    x = np.asarray(x, dtype=np.int64)
    pieces = len(x) // unit
    G = grid * threads
    acc = np.zeros(G, dtype=np.int64)
    piece_sum = x[:pieces * unit].reshape(pieces, unit).sum(axis=1)
    for e0 in range(0, pieces, in_flight * G):
        g = np.arange(min(G, pieces - e0), dtype=np.int64)
        if mutant == "reset":
            acc[g] = 0
        for u in range(in_flight):
            e = e0 + g + u * G
            ok = e < pieces
            if mutant == "clamp":
                acc[g] += piece_sum[np.minimum(e, pieces - 1)]
            else:
                acc[g[ok]] += piece_sum[e[ok]]
    return int(acc.sum() + x[pieces * unit:].sum())


# ----------------------------------------------------------------------------------------------------------------------
# vectorised references (the definitions of the restatements, without their Python loops)
# ----------------------------------------------------------------------------------------------------------------------
def gather_vec(audio, T, stride, S):
    """_generate_ref.gather: seg[s, i] = audio[s * stride + i], zero beyond the end."""
    audio = np.asarray(audio)
    src = (np.arange(S, dtype=np.int64) * stride)[:, None] + np.arange(T, dtype=np.int64)[None, :]
    ok = src < len(audio)
    out = np.zeros((S, T), dtype=audio.dtype)
    out[ok] = audio[src[ok]]
    return out


def stitch_vec(seg, stride, gain, L_out):
    """What segments_stitch_kernel rounds once: for output n the latest segment a = min(n / stride, S - 1) that covers it, i = n -
    a * stride; outside an overlap gain * seg[a, i], inside gain * (w seg[a, i] + (1 - w) seg[a - 1, i + stride]) with w =
    sin^2(pi (i + 1/2) / (2 V)), in float64, rounded to float32 once.  (_generate_ref.stitch is the same sum as an overlap-add.)"""
    seg = np.asarray(seg, dtype=np.float32)
    S, T = seg.shape
    V = T - stride
    flat = seg.reshape(-1).astype(np.float64)
    n = np.arange(L_out, dtype=np.int64)
    a = np.minimum(n // stride, S - 1)
    i = n - a * stride
    out = np.float64(np.float32(gain)) * flat[a * T + i]
    fade = (a > 0) & (i < V)
    if fade.any():
        k = i[fade]
        w = np.sin((k.astype(np.float64) + 0.5) * (np.pi / (2.0 * V))) ** 2
        cur, prev = flat[a[fade] * T + k], flat[(a[fade] - 1) * T + k + stride]
        out[fade] = np.float64(np.float32(gain)) * (w * cur + (1.0 - w) * prev)
    return out.astype(np.float32)


def first_difference(got, want, unit_work):
    """The failure text of a whole-array comparison: first differing index, that index modulo unit_work, number of differences."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return f"first difference at {i} (mod unit_work {i % unit_work}, trip {i // unit_work}): got {got[i]!r}, want {want[i]!r}; {len(bad)} of {len(got)} differ"


def avgpool_fwd_vec(x):
    """_companions.avgpool_fwd_reference with strided slices instead of index lists: x [N, H, W, Cp] -> (mean over the taps inside
    the plane in float64, sum |tap| / count)."""
    x = np.asarray(x, dtype=np.float64)
    N, H, W, Cp = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, Cp))
    xp[:, 1:H + 1, 1:W + 1] = x
    one = np.zeros((2 * Ho + 1, 2 * Wo + 1))
    one[1:H + 1, 1:W + 1] = 1.0
    acc, mag, cnt = np.zeros((N, Ho, Wo, Cp)), np.zeros((N, Ho, Wo, Cp)), np.zeros((Ho, Wo))
    for a in range(3):
        for b in range(3):
            v = xp[:, a:a + 2 * Ho:2, b:b + 2 * Wo:2]
            acc += v
            mag += np.abs(v)
            cnt += one[a:a + 2 * Ho:2, b:b + 2 * Wo:2]
    cnt = cnt[None, :, :, None]
    return acc / cnt, mag / cnt


def avgpool_bwd_vec(dy, H, W):
    """_companions.avgpool_bwd_reference with strided slices: (dx float64, sum of |dy / count| over the windows that hold a pixel)."""
    dy = np.asarray(dy, dtype=np.float64)
    N, Ho, Wo, Cp = dy.shape
    one = np.zeros((2 * Ho + 1, 2 * Wo + 1))
    one[1:H + 1, 1:W + 1] = 1.0
    cnt = np.zeros((Ho, Wo))
    for a in range(3):
        for b in range(3):
            cnt += one[a:a + 2 * Ho:2, b:b + 2 * Wo:2]
    q = dy / cnt[None, :, :, None]
    dx, mag = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, Cp)), np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, Cp))
    for a in range(3):
        for b in range(3):
            dx[:, a:a + 2 * Ho:2, b:b + 2 * Wo:2] += q
            mag[:, a:a + 2 * Ho:2, b:b + 2 * Wo:2] += np.abs(q)
    return dx[:, 1:H + 1, 1:W + 1], mag[:, 1:H + 1, 1:W + 1]


def _block_sum32(v):
    """block_sum of loss.hip on float32 [blocks, 256]: the xor-shuffle tree inside each wave of 64, then the four wave sums added in
    order by thread 0."""
    v = v.reshape(v.shape[0], 4, 64).astype(np.float32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, lane ^ o]).astype(np.float32)
    t = np.zeros(v.shape[0], dtype=np.float32)
    for w in range(4):
        t = (t + v[:, w, 0]).astype(np.float32)
    return t


def loss_fwd_model32(kind, a, b, target, C, coeff, out0, grid, epp):
    """loss_fwd_kernel in float32 and in the kernel's order: thread g adds the terms of pieces g, g + G, g + 2 G, .. (G = grid *
    256) element by element, the workgroup's block_sum, the fold of the workgroup sums by 256 threads in index order and its
    block_sum, then out0 + tot * coeff / (float)(P C).  a, b: float32 [P, Cp] holding the stored values."""
    f = np.float32
    P, Cp = a.shape
    x = a.astype(f)
    t = ((x - f(target)) * (x - f(target))).astype(f) if kind == 0 else np.abs(x - b.astype(f)).astype(f)
    t[:, C:] = 0                                                      # (a masked element adds nothing; + 0.0f changes no bit of a sum >= 0)
    G = grid * 256
    pieces = P * Cp // epp
    K = cdiv(pieces, G)
    tt = np.zeros((K * G, epp), dtype=f)
    tt[:pieces] = t.reshape(pieces, epp)
    tt = tt.reshape(K, G, epp)
    acc = np.zeros(G, dtype=f)
    for k in range(K):
        for j in range(epp):
            acc = (acc + tt[k, :, j]).astype(f)
    part = _block_sum32(acc.reshape(grid, 256))
    s = np.zeros(256, dtype=f)
    for r in range(cdiv(grid, 256)):
        row = part[r * 256:(r + 1) * 256]
        s[:len(row)] = (s[:len(row)] + row).astype(f)
    tot = _block_sum32(s.reshape(1, 256))[0]
    return f(f(out0) + f(f(tot * f(coeff)) / f(P * C)))


def loss_operands(P, dt):
    """(a, b) torch [P, LOSS_CP] in the storage type, values a hash of the position; a tenth of b equals a (the L1 backward's zero)."""
    import torch
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dt]
    n = P * LOSS_CP
    a = torch.from_numpy(hashed_floats(n, seed=91).reshape(P, LOSS_CP)).to(dtype)
    b = torch.from_numpy(hashed_floats(n, seed=92).reshape(P, LOSS_CP)).to(dtype)
    same = torch.from_numpy((index_hash(n, seed=93) % np.uint32(10) == 0).reshape(P, LOSS_CP))
    return a, torch.where(same, a, b)
