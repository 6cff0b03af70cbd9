"""Per-element references and derived bounds of the kernels around the convs (csrc/norm.hip, csrc/loss.hip): InstanceNorm +
activation forward / backward and the e4m3 twin, activation backward, AvgPool, the losses, Adam, the device GradScaler.

The references are float64 and take the kernel's own inputs as given: activations in their storage type, `stats` as the fp32
(mean, M2) the caller uploads -- never recomputed from y.  The branch `yh > 0` is then the sign of the exact y - mean (y and mean
are both binary floating-point numbers, their float64 difference has the sign of the true one, and the kernel's fl(y - mean) has
it too), so no rounding can move it: nothing is excluded from a comparison and there is no "flip" allowance.

Every tolerance is per element, |got - want| <= bound[element], and is DERIVED: the fp32 roundings of the kernel's expression as
written in the .hip file are counted (u = U32 = 2^-24 each, relative to the rounded quantity); where hipcc may contract a * b + c
into one fma both roundings of the uncontracted form stay counted (the contracted form has one fewer: covered); sums get
_exact.sum_bound, which holds for any order; a 16-bit output adds half an ulp of the storage type at the stored value
(`half_ulp`: 2^(e - 8) for a bf16 value in [2^e, 2^(e+1)), 2^(e - 11) for fp16 -- between 2^-9 and 2^-8, resp. 2^-12 and 2^-11,
relative to the value; the value's own binade decides, not one relative figure).  `SECOND` = 1 + 2^-8 multiplies the bounds whose
terms contain a sum (products of two first-order terms: each at most (HW + 16) u < 2^-9 for the planes used), `SMALL` = 1 + 2^-20
those made of a handful of roundings (n u / (1 - n u), n <= 16).

Plain helper: no fixtures, no test functions.  tests/test_companions_host.py pins the references to torch-CPU float64 autograd
and shows that the bounds are usable and that they bite; tests/test_gpu_companions.py runs the kernels against them.

Layouts are the physical ones: activations [N, HW, Cp] (Cp = cpitch(C), pad channels zero), stats / bstats [N, Cp, 2]."""
import ctypes

import numpy as np
import torch

from _exact import (U32, sum_bound, YHAT_ULPS, Guarded, guarded_like, check_guards, cpitch, to_nhwc, assert_bits_equal,  # noqa: F401
                    bsum_reference, act_bwd_reference as _slope_bwd_exact, _hist)

NONE, LRELU, TANH, RELU = 0, 1, 2, 3
EPS = 1e-5
SENTINEL = 0.7
SLOPE32 = float(np.float32(0.2))
SECOND = 1.0 + 2.0 ** -8
SMALL = 1.0 + 2.0 ** -20
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def slope_of(act):
    """The kernels' neg_slope_of: the factor applied to non-positive pre-activations, as the fp32 value."""
    return {NONE: 1.0, LRELU: SLOPE32, RELU: 0.0}[act]


# ----------------------------------------------------------------------------------------------------------------------
# storage rounding, comparison
# ----------------------------------------------------------------------------------------------------------------------
_PREC = {torch.bfloat16: 8, torch.float16: 11}                 # significand bits
_MIN_ULP_EXP = {torch.bfloat16: -133, torch.float16: -24}      # exponent of the smallest subnormal


def half_ulp(v, dtype):
    """Half an ulp of `dtype` in the binade of |v| (float64 tensor); 0 for float32 outputs (the fp32 roundings are counted in the
    bound itself).  |v| in [2^(e-1), 2^e) = frexp exponent e: ulp = 2^(e - p), not below the smallest subnormal."""
    v = v.abs().double()
    if dtype == torch.float32:
        return torch.zeros_like(v)
    _, e = torch.frexp(v)
    e = (e - _PREC[dtype]).clamp(min=_MIN_ULP_EXP[dtype])
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.full_like(v, 0.5), e))


def stored_bound(want, b32, dtype):
    """Bound on the STORED value: the fp32 value lies within b32 of want, rounding to nearest moves it by at most half an ulp of
    the binade of |want| + b32 (or of a lower one)."""
    return b32 + half_ulp(want.abs() + b32, dtype)


def assert_within(got, want, bound, what, C=None):
    """|got - want| <= bound for every element (NaN fails).  got: the whole tensor the kernel left; layout [N, P, Cp] or flat.
    The message gives the count, the first offenders with their indices and histograms over n, pixel and c % 8 / 32 / 64."""
    got = got.detach().cpu().double()
    want = want.double().reshape(got.shape)
    bound = bound.double().expand(got.shape) if bound.dim() == 0 else bound.double().reshape(got.shape)
    err = (got - want).abs()
    bad = ~(err <= bound)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero().numpy()
    first = [tuple(int(v) for v in idx[i]) + (float(got[tuple(idx[i])]), float(want[tuple(idx[i])]), float(bound[tuple(idx[i])]))
             for i in range(min(8, n))]
    if got.dim() == 3:
        c = idx[:, 2]
        hist = {"n": _hist(idx[:, 0]), "pixel": _hist(idx[:, 1]), "c%8": _hist(c, 8), "c%32": _hist(c, 32), "c%64": _hist(c, 64)}
        if C is not None:
            hist["pad_channels"] = int((c >= C).sum())
    else:
        hist = {f"d{i}": _hist(idx[:, i]) for i in range(idx.shape[1])}
        hist["last%8"] = _hist(idx[:, -1], 8)
    worst = float((err / bound.clamp(min=1e-300))[bad].nan_to_num(nan=float("inf")).max())
    raise AssertionError(f"{what}: {n} of {bad.numel()} elements outside their bound (worst error / bound {worst:.3g}); first "
                         f"(index..., got, want, bound): {first}; histograms of the offenders: {hist}")


def fails(fn, *a, **kw):
    """True if the check raises AssertionError (mutant tests)."""
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm + activation: cases and data
# ----------------------------------------------------------------------------------------------------------------------
# (N, HW, C, two_pass, what it covers).  Single launch: HW <= 640 and N * ceil(cpr / 4) >= 128, cpr = Cp / 8 (16-bit), Cp / 4 (f32).
IN_CASES = [
    (64, 512, 64, 0, "ITERS 8, full"),
    (64, 513, 64, 0, "ITERS 10, one live pixel in the last two rounds"),
    (64, 640, 64, 0, "ITERS 10, full"),
    (65, 1, 40, 0, "grid 130 / 195 (no multiple of 8), last column block partly valid, every load clamped to pixel 0"),
    (129, 65, 20, 0, "Cp 24: pad channels; grid 129 / 258"),
    (128, 64, 3, 0, "one piece per pixel in 16-bit"),
    (64, 641, 64, 1, "first plane past the boundary"),
    (2, 4, 32, 1, "fewer pieces than one workgroup"),
    (1, 1, 3, 1, "smallest case"),
    (3, 1320, 24, 1, "cpr 3 / 6, several workgroups, clamped tail loads"),
    (2, 700, 200, 1, "cpr 25 / 50, no pad channels"),
    (2, 35, 67, 1, "Cp 72, cpr 9 / 18"),
    (1, 648, 1032, 1, "cpr 129 / 258: more columns than threads in f32"),
    (2, 17920, 16, 1, "a plane of more than 16384 pixels"),
]
IN_IDS = [f"n{c[0]}_hw{c[1]}_c{c[2]}" for c in IN_CASES]
# Two-pass planes whose reduce launch is CLAMPED to its region of the reduction scratch (csrc/norm.hip, instnorm_bwd_rows:
# rows_max = 2^21 / (Cp N) partial rows per sample, rounded down to a multiple of the grid unit).  A list of its own: only the
# backward tests walk it.  The tests ask p2phd_reduction_rows for the grids and assert used < wanted before they launch; the
# figures in the descriptions are what the arithmetic gives today (wanted -> used per sample, 16-bit storage / f32).
IN_CLAMP_CASES = [
    (1, 2400, 4096, 1, "the most channels the kernels hold, one sample: rows_max 512; 600 -> 512 / 1200 -> 512"),
    (8, 1100, 2048, 1, "configs[4] trunk width at its benchmarked batch: rows_max 128; 138 -> 128 / 256 -> 128"),
    (3, 5000, 1536, 1, "configs[3] trunk width, cpr 192 / 384: grid unit 3, rows_max 455 rounds down to 453; 468 -> 453 / 681 -> 453"),
]
IN_CLAMP_IDS = [f"n{c[0]}_hw{c[1]}_c{c[2]}" for c in IN_CLAMP_CASES]
# (P, C) of p2phd_act_bwd_db; the clamped ones: rows_max = 2^20 / Cp.  wanted -> used: (1100, 4096) 274 -> 256 / 548 -> 256 (the most
# channels), (8000, 1536) 750 -> 681 / 1500 -> 681 (grid unit 3: rows_max 682 rounds down)
ACT_DB_CASES = [(1, 3), (40, 40), (1320, 24), (700, 67), (5000, 200)]
ACT_DB_CLAMP_CASES = [(1100, 4096), (8000, 1536)]


def reduction_rows(lib, family, code, N, P, C):
    """p2phd_reduction_rows (host arithmetic, no device): (return code, rows_wanted, rows_used) per sample."""
    wanted, used = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.p2phd_reduction_rows(family.encode(), code, N, P, C, ctypes.byref(wanted), ctypes.byref(used))
    return rc, wanted.value, used.value


def clamped_rows(lib, family, code, N, P, C, epp):
    """(wanted, used) of a case that a test means to run on the clamped path: asserts that it is one, and that the clamp left the
    grid stride a multiple of the pieces per pixel."""
    rc, wanted, used = reduction_rows(lib, family, code, N, P, C)
    what = f"{family} N {N} P {P} C {C} dtype code {code}: wanted {wanted}, used {used}"
    assert rc == 0, (what, lib.p2phd_last_error())
    assert 1 <= used < wanted, what + ": not clamped by the reduction scratch (has the region grown?)"
    assert used * 256 % (cpitch(C) // epp) == 0, what + ": the grid stride is no multiple of the pieces per pixel"
    return wanted, used
CH_7SIGMA, CH_ONMEAN, CH_CONST = 0, 1, 2                       # C >= 3 in every case; channel 3 (if any) is the second constant one
ONMEAN = 0.25
CONST = 0.5

_DATA = {}


def physical(t, dtype):
    """[N, P, C] float -> [N, P, Cp] in dtype, pad channels +0."""
    N, P, C = t.shape
    out = torch.zeros(N, P, cpitch(C), dtype=torch.float64)
    out[..., :C] = t
    return out.to(dtype)


def in_data(case, dt):
    """Deterministic operands of an InstanceNorm case: y, g, residual [N, HW, Cp] in the storage type, stats [N, Cp, 2] fp32.
    Channel 0: |mean| = 7 sigma (sign alternating with n); channel 1: uploaded mean 0.25 exactly, every third pixel exactly on it;
    channel 2 (and 3): constant 0.5 with M2 = 0 / -1e-3 in the stats (alternating with n, opposite on channel 3): rstd =
    1 / sqrt(eps), yh = 0.  stats are those of the stored y rounded to fp32 (HW = 1: drawn, a one-pixel plane's own statistics
    would make every yh zero), then overridden on the special channels -- the kernels take them as given, so do the references."""
    key = (case[:3], dt)
    if key in _DATA:
        return _DATA[key]
    N, HW, C = case[:3]
    dtype = DT[dt]
    gen = torch.Generator().manual_seed(1000 * N + 7 * HW + C)
    y = torch.randn(N, HW, C, generator=gen) * (0.5 + torch.rand(N, 1, C, generator=gen)) + torch.randn(N, 1, C, generator=gen)
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)[:, None]
    y[:, :, CH_7SIGMA] = torch.randn(N, HW, generator=gen) + 7.0 * sign
    y[:, :, CH_ONMEAN] = ONMEAN + 0.5 * torch.randn(N, HW, generator=gen)
    y[:, ::3, CH_ONMEAN] = ONMEAN
    consts = [CH_CONST] + ([3] if C > 3 else [])
    for c in consts:
        y[:, :, c] = CONST
    y = physical(y, dtype)
    yd = y.double()
    if HW > 1:
        mean = yd.mean(1)
        m2 = ((yd - mean[:, None]) ** 2).sum(1)
    else:
        mean = yd[:, 0] + 0.5 * torch.randn(N, y.shape[2], generator=gen).double()
        m2 = torch.rand(N, y.shape[2], generator=gen).double()
    stats = torch.stack([mean, m2], -1).float()
    stats[:, CH_ONMEAN, 0] = ONMEAN
    for i, c in enumerate(consts):
        stats[:, c, 0] = CONST
        stats[:, c, 1] = torch.where((torch.arange(N) + i) % 2 == 0, 0.0, -1e-3)
    stats[:, C:] = 0
    g = physical(torch.randn(N, HW, C, generator=gen), dtype)
    res = physical(torch.randn(N, HW, C, generator=gen), dtype)
    out = dict(y=y, g=g, res=res, stats=stats.contiguous())
    if len(_DATA) > 2:
        _DATA.clear()
    _DATA[key] = out
    return out


# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm + activation: references
# ----------------------------------------------------------------------------------------------------------------------
def _mean_rstd(stats, HW, C, eps):
    """mean, rstd [N, 1, Cp] in float64 from the fp32 stats; M2 < 0 clamped to 0; rstd 0 on pad channels (ChanConsts::load)."""
    mean = stats[..., 0].double()
    rstd = 1.0 / torch.sqrt(stats[..., 1].double().clamp(min=0) / HW + float(np.float32(eps)))
    rstd[:, C:] = 0
    return mean[:, None], rstd[:, None]


# yh = fl(fl(y - mean) * rstd), rstd = rsqrtf(fmaxf(M2 * inv, 0) + eps), inv = 1.f / HW  (in_act_fwd_kernel, ChanConsts::load):
# inv 1 rounding, M2 * inv 1, + eps 1 (fmaxf sits between the product and the sum: no contraction) -> the argument within 3 u (all
# terms positive), its inverse square root within 1.5 u, rsqrtf itself 1 ulp = 2 u: rstd within 3.5 u.  y - mean: 1, the product: 1
# -> yh within 5.5 u.  act_fwd multiplies a non-positive yh by the slope: 1 more (exact for slopes 1 and 0) -> 6.5 u;
# IN_ACT_ULPS = 8 leaves the second-order terms room, as YHAT_ULPS does.  With a residual, f += r rounds once more, relative to
# the sum (contracted with the slope product: one fewer).
IN_ACT_ULPS = 8


def instnorm_fwd_reference(y, stats, residual, HW, C, eps, act):
    """act((y - mean) * rstd) + residual per element, float64 [N, HW, Cp], pad channels exactly 0, and its fp32 bound."""
    mean, rstd = _mean_rstd(stats, HW, C, eps)
    yh = (y.double() - mean) * rstd
    a = torch.where(yh > 0, yh, slope_of(act) * yh)
    b32 = IN_ACT_ULPS * U32 * a.abs()
    want = a
    if residual is not None:
        r = residual.double()
        want = a + r
        b32 = b32 + U32 * (a.abs() + r.abs() + b32)
    want[..., C:] = 0
    b32[..., C:] = 0
    return want, b32


def q8(t):
    """The e4m3 code of a float64 tensor clamped to +-448, decoded (round to nearest even on the CPU)."""
    return t.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn).float().double()


def assert_q8_neighbours(out8, want, b32, what, C):
    """out8: the uint8 twin.  The kernel quantises its fp32 value f (not the stored 16-bit one), f lies within b32 of want and q is
    monotone: the decoded byte lies between q(want - b32) and q(want + b32)."""
    got = out8.detach().cpu().contiguous().view(torch.float8_e4m3fn).float().double()
    lo, hi = q8(want - b32), q8(want + b32)
    mid = (lo + hi) / 2
    assert_within(got, mid, (hi - lo) / 2, what, C)


# dy = fl(rstd * fl(fl(gp - m1) - fl(yh * m2))), gp = fl(g * slope), m1 = fl(S1 * inv), m2 = fl(S2 * inv)  (in_act_bwd_apply_kernel,
# in_act_bwd_fused_kernel).  The bracket B = gp - m1 - yh m2, with A = |gp| + |m1| + |yh m2|:
#   gp: 1 rounding; m1: its sum S1 within sum_bound(sum |gp|, HW, 1) (1 = the rounding of each term), / HW (sum_bound's + 8 holds
#   the roundings of inv and of the product); m2 likewise with YHAT_ULPS per term (yh 5.5 u, gp 1, the product 1: 7.5 u);
#   yh m2: yh within 5.5 u, the product 1 (or contracted into the subtraction); gp - m1: 1, relative to at most |gp| + |m1|;
#   (...) - yh m2: 1, relative to at most A
#   -> |dB| <= dm1 + |yh| dm2 + u (|gp| + 2 (|gp| + |m1|) + 6.5 |yh m2| + A) <= dm1 + |yh| dm2 + IN_BWD_ULPS u A, IN_BWD_ULPS = 10.
# The product with rstd: 1 rounding and rstd's 3.5 u, relative to dy: 4.5 u -> 5.
IN_BWD_ULPS = 10
IN_BWD_OUT_ULPS = 5


def instnorm_bwd_reference(g, y, stats, HW, C, eps, act):
    """dict(dy, b32 [N, HW, Cp]; s1, s2, bs1, bs2 [N, Cp]: the two sums and their bounds) in float64."""
    mean, rstd = _mean_rstd(stats, HW, C, eps)
    yh = (y.double() - mean) * rstd
    gp = g.double() * torch.where(yh > 0, 1.0, slope_of(act))
    nchw = lambda t: t.double().permute(0, 2, 1)[..., None]               # [N, Cp, HW, 1]: the layout of _exact.bsum_reference
    s1, s2, bs1, bs2 = bsum_reference(nchw(g), nchw(y), stats[..., 0], stats[..., 1].clamp(min=0), eps, slope_of(act))
    m1, m2 = (s1 / HW)[:, None], (s2 / HW)[:, None]
    dy = rstd * (gp - m1 - yh * m2)
    A = gp.abs() + m1.abs() + (yh * m2).abs()
    b32 = (rstd * ((bs1 / HW)[:, None] + yh.abs() * (bs2 / HW)[:, None] + IN_BWD_ULPS * U32 * A) + IN_BWD_OUT_ULPS * U32 * dy.abs()) * SECOND
    dy[..., C:] = 0
    b32[..., C:] = 0
    return dict(dy=dy, b32=b32, s1=s1, s2=s2, bs1=bs1, bs2=bs2)


def colsum_check(stored, db, C, what, prefill=None):
    """db of the InstanceNorm backward / of p2phd_act_bwd_db: the kernel adds its ROUNDED outputs (for the InstanceNorm the true
    value is 0 and carries no information), so the reference is the float64 column sum of what it stored, the tolerance
    sum_bound(sum |stored|, terms); accumulate mode adds the prefill as one more term (one more rounding)."""
    s = stored.detach().cpu().double().reshape(-1, stored.shape[-1])[:, :C]
    want, mag, terms = s.sum(0), s.abs().sum(0), s.shape[0]
    if prefill is not None:
        want, mag, terms = want + prefill.double(), mag + prefill.double().abs(), terms + 1
    assert_within(db.detach().cpu()[:C], want, sum_bound(mag, terms), what)


def bstats_check(bstats, ref, C, what):
    """bstats [N, Cp, 2] of the two-pass form against the sums of instnorm_bwd_reference; pad columns exactly 0."""
    b = bstats.detach().cpu().double()
    bound = torch.stack([ref["bs1"], ref["bs2"]], -1)
    bound[:, C:] = 0
    N = b.shape[0]                                             # flat [N, 2 Cp]: index d1 = 2 c + (0: sum g', 1: sum g' yhat)
    assert_within(b.reshape(N, -1), torch.stack([ref["s1"], ref["s2"]], -1).reshape(N, -1), bound.reshape(N, -1), what)


# ----------------------------------------------------------------------------------------------------------------------
# activation backward from the saved output
# ----------------------------------------------------------------------------------------------------------------------
def act_bwd_reference(g, a, act, dtype):
    """(want, bound): NONE / RELU / LRELU are one fp32 multiply by 1, 0 or 0.2f and one rounding to storage: bit-exact, bound None
    (compare with assert_bits_equal).  TANH: s = fl(1 - fl(o o)) or fma(-o, o, 1): within u (o^2 + |s|); the product g s: 1 more,
    relative to |g s| -> u |g| (o^2 + 2 |s|)."""
    if act != TANH:
        return _slope_bwd_exact(g, a, slope_of(act), dtype), None
    o = a.double()
    s = 1.0 - o * o
    want = g.double() * s
    return want, stored_bound(want, U32 * g.double().abs() * (o * o + 2 * s.abs()) * SMALL, dtype)


# ----------------------------------------------------------------------------------------------------------------------
# AvgPool2d(3, 2, 1, count_include_pad=False)
# ----------------------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 3, 1, 1), (2, 8, 1, 7), (2, 8, 8, 1), (1, 20, 2, 5), (2, 16, 3, 3), (1, 67, 7, 5), (2, 4, 16, 10)]   # N, C, H, W
# forward: at most 9 additions (the first onto 0 is exact), inv = 1.f / cnt 1 rounding, the product 1: 11 u of sum |x| / cnt.
# backward: at most 4 terms fl(dy * inv) (inv 1, product 1, or contracted) and their additions: within the same count.
POOL_ULPS = 9 + 2


def pool_out(n):
    return (n - 1) // 2 + 1


def _windows(H, W):
    """(a, b, hs, ws): for tap (a, b) the output rows hs / columns ws whose input index 2 o - 1 + tap lies inside the plane."""
    Ho, Wo = pool_out(H), pool_out(W)
    for a in range(3):
        hs = [o for o in range(Ho) if 0 <= 2 * o - 1 + a < H]
        for b in range(3):
            ws = [o for o in range(Wo) if 0 <= 2 * o - 1 + b < W]
            if hs and ws:
                yield a, b, torch.tensor(hs), torch.tensor(ws)


def pool_counts(H, W):
    cnt = torch.zeros(pool_out(H), pool_out(W), dtype=torch.float64)
    for a, b, hs, ws in _windows(H, W):
        cnt[hs[:, None], ws[None, :]] += 1
    return cnt


def avgpool_fwd_reference(x):
    """x [N, H, W, Cp] -> (y [N, Ho, Wo, Cp] float64, fp32 bound): the mean over the taps inside the plane."""
    x = x.double()
    N, H, W, Cp = x.shape
    acc = torch.zeros(N, pool_out(H), pool_out(W), Cp, dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for a, b, hs, ws in _windows(H, W):
        v = x[:, (2 * hs - 1 + a)[:, None], (2 * ws - 1 + b)[None, :]]
        acc[:, hs[:, None], ws[None, :]] += v
        mag[:, hs[:, None], ws[None, :]] += v.abs()
    cnt = pool_counts(H, W)[None, :, :, None]
    return acc / cnt, POOL_ULPS * U32 * (mag / cnt) * SMALL


def avgpool_bwd_reference(dy, H, W):
    """The exact adjoint: dx[i, j] = sum over the windows that hold (i, j) of dy[ho, wo] / cnt[ho, wo]."""
    dy = dy.double()
    N, Ho, Wo, Cp = dy.shape
    assert (Ho, Wo) == (pool_out(H), pool_out(W))
    q = dy / pool_counts(H, W)[None, :, :, None]
    dx = torch.zeros(N, H, W, Cp, dtype=torch.float64)
    mag = torch.zeros_like(dx)
    for a, b, hs, ws in _windows(H, W):
        v = q[:, hs[:, None], ws[None, :]]
        dx[:, (2 * hs - 1 + a)[:, None], (2 * ws - 1 + b)[None, :]] += v
        mag[:, (2 * hs - 1 + a)[:, None], (2 * ws - 1 + b)[None, :]] += v.abs()
    return dx, POOL_ULPS * U32 * mag * SMALL


# ----------------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(40, 3), (700, 67), (8192, 72), (30000, 67)]      # (P, C)
OUT0 = 0.75
# per term: kind 0 fl(x - target) 1 rounding, squared: 2 u, the product 1 (or contracted into the accumulation): 3; kind 1
# fl(x - b): 1
LOSS_TERM_ULPS = {0: 3, 1: 1}


def loss_data(P, C, dt, kind):
    gen = torch.Generator().manual_seed(31 * P + C + kind)
    a = physical(torch.randn(1, P, C, generator=gen), DT[dt])[0]
    b = physical(torch.randn(1, P, C, generator=gen), DT[dt])[0]
    same = torch.rand(P, a.shape[1], generator=gen) < 0.1      # a tenth of the elements: b == a (dlt == 0 in the L1 backward)
    b = torch.where(same, a, b)
    return a, b


def loss_fwd_reference(kind, a, b, target, C, coeff, out0):
    """out0 + coeff * mean(term) over the P * C valid elements and its bound: the sum passes through per-thread accumulators, a
    shuffle tree, the per-workgroup table and the fold -- sum_bound(sum |term|, P C, term roundings), whose + 8 holds
    fl(fl(tot * coeff) / fl(P C)) --, scaled by coeff / (P C); then *out += ...: 1 rounding, relative to |out0| + |coeff| mean."""
    P = a.shape[0]
    x = a.double()[:, :C]
    t = (x - float(np.float32(target))) ** 2 if kind == 0 else (x - b.double()[:, :C]).abs()
    tot = float(t.sum())
    c = float(np.float32(coeff))
    add = c * tot / (P * C)
    bsum = float(sum_bound(tot, P * C, LOSS_TERM_ULPS[kind])) * abs(c) / (P * C)
    return out0 + add, (bsum + U32 * (abs(out0) + abs(add) + bsum)) * SMALL


def loss_bwd_reference(kind, a, b, target, C, coeff, gup, dtype):
    """Bit-exact restatement in float32 (loss_bwd_kernel): s = fl(fl(gup * coeff) / fl((float)(P C))); kind 0:
    fl(fl(2 * fl(x - target)) * s); kind 1: +s, -s, or 0 where a == b; pad channels +0; one rounding to storage."""
    P, Cp = a.shape
    f = np.float32
    s = f(f(f(gup) * f(coeff)) / f(P * C))
    x = a.float().numpy()
    if kind == 0:
        gr = (f(2.0) * (x - f(target))).astype(f) * s
    else:
        d = x - b.float().numpy()
        gr = np.where(d > 0, s, np.where(d < 0, -s, f(0.0)))
    gr = gr.astype(f)
    gr[:, C:] = 0.0
    return torch.from_numpy(gr).to(dtype)


# ----------------------------------------------------------------------------------------------------------------------
# Adam, GradScaler
# ----------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = [1, 3, 4, 5, 1003, 4096 * 1024 + 7]
# gr = fl(g * gscale): 1 rounding.
# m' = fl(fl(b1 m) + fl(fl(1 - b1) gr)): 1 - b1 is exact in fp32 for b1 in [0.5, 1] (Sterbenz; the reference forms it from the
#   fp32 b1 too); products 1 each, gr's own 1, the sum 1, relative to Am = |b1 m| + |(1 - b1) gr| at most: 3 u Am.
# v' = fl(fl(b2 v) + fl(fl(fl(1 - b2) gr) gr)): the term carries gr's rounding twice and two products: 4 u; b2 v: 1; the sum: 1:
#   5 u v' (all terms non-negative).
# update U = fl(fl(fl(lr / bc1) m') / fl(fl(sqrtf(v') / bc2s) + eps)): bc1, bc2s are fp32 roundings of the double values: 1 each;
#   lr / bc1: 1 (HIP's fp32 division and sqrtf are correctly rounded: no fast-math flag in csrc/Makefile); the product with m': 1,
#   m' itself within 3 u Am; sqrtf: half of v's 5 u = 2.5, + 1; / bc2s: 1 + 1; + eps: 1: the denominator within 6.5 u (positive
#   terms); the quotient: 1 -> |dU| <= (1 + 1 + 1 + 6.5 + 1) u |U| + 3 u Uabs <= 13.5 u Uabs, with Uabs = (lr / bc1) Am / den >= |U|
#   the same update on magnitudes.  p' = fl(p - U): 1, relative to |p| + |U| -> u |p| + ADAM_P_ULPS u Uabs, ADAM_P_ULPS = 15.
ADAM_M_ULPS, ADAM_V_ULPS, ADAM_P_ULPS = 3, 5, 15


def adam_state(n, seed):
    """Random state: p, m, g normal, v >= 0; every seventh element has v = 0 and a tiny gradient (the denominator is then of the
    order of eps: eps inside or outside the square root differ), every eleventh a zero gradient."""
    gen = torch.Generator().manual_seed(seed)
    p, m, g = (torch.randn(n, generator=gen) for _ in range(3))
    v = torch.rand(n, generator=gen) * 0.1
    i = torch.arange(n)
    tiny = i % 7 == 3
    v[tiny] = 0.0
    g[tiny] = g[tiny] * 1e-6
    g[i % 11 == 5] = 0.0
    return p, g, m * 0.1, v


def adam_reference(p, g, m, v, lr, b1, b2, eps, t, gscale):
    """One Adam step from (p, m, v) at step count t (1-based) in float64, betas / lr / eps / gscale as their fp32 values, exact
    bias corrections; returns (p', m', v') and their bounds."""
    f = lambda s: float(np.float32(s))
    lr, b1, b2, eps, gscale = f(lr), f(b1), f(b2), f(eps), f(gscale)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gr = g * gscale
    m1 = b1 * m + (1 - b1) * gr
    am = (b1 * m).abs() + ((1 - b1) * gr).abs()
    v1 = b2 * v + (1 - b2) * gr * gr
    bc1, bc2s = 1 - b1 ** t, (1 - b2 ** t) ** 0.5
    den = v1.sqrt() / bc2s + eps
    upd = lr / bc1 * m1 / den
    uabs = lr / bc1 * am / den
    bounds = (U32 * p.abs() + ADAM_P_ULPS * U32 * uabs) * SMALL, ADAM_M_ULPS * U32 * am * SMALL, ADAM_V_ULPS * U32 * v1 * SMALL
    return (p - upd, m1, v1), bounds


def scaler_update_reference(state, growth, backoff, interval):
    """scaler_update_kernel restated in fp32: state = (scale, 1 / scale, growth tracker, found_0, found_1).  Bit-exact for
    power-of-two factors (the products are exact, 1 / scale is one correctly rounded division)."""
    f = np.float32
    s = [f(x) for x in state]
    scale, tracker = s[0], s[2]
    if s[3] != 0 or s[4] != 0:
        scale, tracker = f(scale * f(backoff)), f(0)
    else:
        tracker = f(tracker + f(1))
        if tracker >= f(interval):
            scale, tracker = f(scale * f(growth)), f(0)
    return [scale, f(f(1) / scale), tracker, f(0), f(0)]


SCALER_TABLE = [  # (state before, growth, backoff, interval)
    ([1024.0, 2.0 ** -10, 5.0, 1.0, 0.0], 2.0, 0.5, 8),        # found on slot 0
    ([1024.0, 2.0 ** -10, 5.0, 0.0, 1.0], 2.0, 0.5, 8),        # found on slot 1
    ([1024.0, 2.0 ** -10, 7.0, 1.0, 1.0], 2.0, 0.5, 8),        # on both (at the interval: backoff wins)
    ([1024.0, 2.0 ** -10, 3.0, 0.0, 0.0], 2.0, 0.5, 8),        # clean, below the interval
    ([1024.0, 2.0 ** -10, 7.0, 0.0, 0.0], 2.0, 0.5, 8),        # clean, reaches the interval: growth
    ([1024.0, 2.0 ** -10, 11.0, 0.0, 0.0], 2.0, 0.5, 8),       # clean, already above it
    ([65536.0, 2.0 ** -16, 0.0, 0.0, 0.0], 2.0, 0.5, 1),       # interval 1: grows on every clean step
    ([3.0, 1.0 / 3.0, 0.0, 1.0, 0.0], 2.0, 0.5, 4),            # 1 / scale is a rounded quotient
]
