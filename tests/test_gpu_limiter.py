"""The look-ahead true-peak limiter on the GPU (csrc/limiter.hip: p2phd_limiter_envelope, p2phd_limiter_apply; generate.limit):
the envelope with integer operands against the float64 restatement of tests/_limiter_ref.py bit for bit and with float operands
inside the bound of an fp32 dot product; the sliding minimum and the sum bit for bit on operands fp32 holds, the real window inside
the bound of the fp32 sum; the clamp, the skipped tile, the product, the statistics, the launch counter and the refusals.  Every
call writes its outputs between canaries."""
import numpy as np
import pytest
import torch

import _limiter_ref as LR
import _truepeak_ref as TP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                         # words on either side of an output
GUARD_BITS = 0x7FC0BEEF                                            # a NaN pattern no kernel writes
PLANS = ((1, 0), (7, 3), (72, 0), (240, 960), (1024, 4096))       # (look-ahead A, hold H)


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _tile():
    return int(_lib().lib().p2phd_limiter_tile_len())


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"limiter", 1 if reset else 0)


def _error():
    return _lib().lib().p2phd_last_error().decode("utf-8", "replace")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _lengths(A, H, T, few=False):
    """Around the tile and the halo; the largest plan only at two lengths."""
    if few:
        return [T + 1, 2 * T + A + H + 3]
    return sorted({0, 1, A, A + H + 1, T - 1, T, T + 1, 2 * T + 1, 2 * T + A + H + 3})


def _guarded(*sizes):
    """One int32 buffer of canaries with a hole of every size -> (buffer, [float32 view at each hole], mask of the canaries)."""
    total = GUARD + sum(n + GUARD for n in sizes)
    buf = torch.full((total,), GUARD_BITS, dtype=torch.int32, device=DEV)
    views, mask, at = [], np.ones(total, dtype=bool), GUARD
    for n in sizes:
        views.append(buf[at:at + max(n, 1)].view(torch.float32))
        mask[at:at + n] = False
        at += n + GUARD
    return buf, views, mask


def _holes(buf, mask, sizes):
    """-> (the holes' int32 contents, canaries intact)."""
    bits = buf.cpu().numpy()
    out, at = [], GUARD
    for n in sizes:
        out.append(bits[at:at + n].copy())
        at += n + GUARD
    return out, bool((bits[mask] == GUARD_BITS).all())


def _rows_dev(x, pitch_extra=3, off=1):
    """Rows of x [C, L] `L + pitch_extra` floats apart, the first `off` floats past a 16-byte boundary -> (keep-alive, view, ld)."""
    C, L = x.shape
    ld = L + pitch_extra
    host = np.full(4 + off + C * ld + 4, np.float32(77.0))
    for c in range(C):
        host[4 + off + c * ld:4 + off + c * ld + L] = x[c]
    buf = torch.from_numpy(host).to(DEV)
    return buf, buf[4 + off:], ld


def _envelope(x, table_dev, ceiling, frames=None, factor=None, taps=None):
    """p2phd_limiter_envelope -> (return code, r [L] as int32 bits, peak bits, canaries intact)."""
    L_ = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    C, L = x.shape
    keep, rows, ld = _rows_dev(x)
    F, P = table_dev.shape
    buf, (r, peak), mask = _guarded(L, 1)
    rc = L_.lib().p2phd_limiter_envelope(L_.ptr(rows), L if frames is None else frames, C, ld, L_.ptr(table_dev), F if factor is None else factor,
                                         P if taps is None else taps, float(ceiling), L_.ptr(r), L_.ptr(peak), L_.stream_ptr())
    torch.cuda.synchronize()
    (rb, pb), intact = _holes(buf, mask, (L, 1))
    return rc, rb, int(pb[0]), intact


def _truepeak_top(x, table_dev):
    """The largest tpeak p2phd_truepeak reports for the rows, as bits."""
    L_ = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    C, L = x.shape
    keep, rows, ld = _rows_dev(x, 5, 3)
    F, P = table_dev.shape
    out = torch.zeros((C + 1,), dtype=torch.float32, device=DEV)
    assert L_.lib().p2phd_truepeak(L_.ptr(rows), L, C, ld, L_.ptr(table_dev), F, P, 1.0, L_.ptr(out), L_.ptr(out[C:]), L_.stream_ptr()) == 0
    return int(_bits(out[:C].cpu().numpy()).max())                # (bit patterns of non-negative floats order as the floats)


def _apply(x, r, A, H, w, want_g=True, frames=None, lookahead=None, hold=None):
    """p2phd_limiter_apply -> (return code, out [C, L] bits, g [L] bits, (min g as float32, count), canaries intact)."""
    L_ = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    C, L = x.shape
    keep, rows, ld = _rows_dev(x, 2, 3)
    r_dev = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float32)).to(DEV)
    w_dev = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(DEV)
    out_ld = L + 5
    sizes = (C * out_ld, L, 2)
    buf, (out, g, stats), mask = _guarded(*sizes)
    for c in range(C):
        mask[GUARD + c * out_ld + L:GUARD + (c + 1) * out_ld] = True        # the pitch between rows stays untouched too
    rc = L_.lib().p2phd_limiter_apply(L_.ptr(rows), L if frames is None else frames, C, ld, L_.ptr(r_dev), A if lookahead is None else lookahead,
                                      H if hold is None else hold, L_.ptr(w_dev), L_.ptr(out), out_ld, L_.ptr(g) if want_g else None,
                                      L_.ptr(stats), L_.stream_ptr())
    torch.cuda.synchronize()
    (ob, gb, sb), intact = _holes(buf, mask, sizes)
    ob = ob.reshape(C, out_ld)[:, :L]
    return rc, ob, gb, (sb[:1].view(np.float32)[0], int(sb[1]) & 0xFFFFFFFF), intact


def _int_table(rng, F, P, lo=-4, hi=4):
    t = rng.integers(lo, hi + 1, (F, P)).astype(np.float32)
    t[:, 0] = rng.choice([-3, -1, 1, 2], F)                        # both end taps count, the table is not symmetric
    t[:, -1] = rng.choice([-2, 1, 3], F)
    return t / np.float32(16.0)


# ------------------------------------------------------------------------------------------
# 1. the envelope
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", (1, 2, 4))
@pytest.mark.parametrize("P", (24, 64))
def test_envelope_of_integer_operands_is_exact(F, P):
    """Samples integers in [-8, 8], coefficients integers in [-4, 4] / 16 (tests/test_gpu_truepeak.py): every sum is exact in fp32, so
    every m has one bit pattern and r is one fp32 division of it.  Every length around the tile and the halo, 1, 2 and 5 rows; the
    folded peak is p2phd_truepeak's largest tpeak on the same clip."""
    T = _tile()
    rng = np.random.default_rng(1000 * F + P)
    table = _int_table(rng, F, P)
    table_dev = torch.from_numpy(table).to(DEV)
    xs = rng.integers(-8, 9, (5, 2 * T + 1300)).astype(np.float32)
    xs[1:, :] = np.where(rng.random(xs[1:].shape) < 0.7, 0.0, xs[1:])       # the rows differ in where they are loud
    ceiling = 6.5
    for L in _lengths(240, 960, T):
        for C in (1, 2, 5):
            x = xs[:C, :L]
            m = LR.envelope(x, table)
            m32 = m.astype(np.float32)
            assert np.array_equal(m32.astype(np.float64), m)
            want = LR.ratio(m32, ceiling)
            _count(reset=True)
            rc, r, peak, intact = _envelope(x, table_dev, ceiling)
            assert rc == 0 and intact and _count() == (1 if L else 0), (L, C, rc, intact, _error())
            assert np.array_equal(r, _bits(want)), (L, C, np.flatnonzero(r != _bits(want))[:8])
            assert peak == (int(_bits(m32).max()) if L else 0) == _truepeak_top(x, table_dev), (L, C)
            if L > T:
                assert (want < 1).any() and (want == 1).any()


def test_envelope_of_float_operands_lies_inside_the_dot_product_bound():
    """The library's own table and noise: m32 lies within dot_bound of the float64 m, so r = fl(c / m32) lies between the roundings
    of c / (m + b) and c / (m - b) (rounding is monotone; one ulp for forming those in float64 first), is exactly 1 where
    m + b <= c, and the folded peak lies within b of the largest m -- and is p2phd_truepeak's bit for bit."""
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients
    T = _tile()
    rng = np.random.default_rng(5)
    table = true_peak_coefficients(4, 24, 9.0).numpy()
    table_dev = torch.from_numpy(table).to(DEV)
    x = (0.3 * rng.standard_normal((2, 2 * T + 77))).astype(np.float32)
    c = np.float32(0.5)
    m = LR.envelope(x, table)
    b = TP.dot_bound(x, table).max()
    rc, r, peak, intact = _envelope(x, table_dev, c)
    assert rc == 0 and intact
    r = r.view(np.float32)
    one = np.float32(1.0)
    lo = np.where(m + b > c, np.float64(c) / (m + b), 1.0).astype(np.float32)
    hi = np.where(m - b > c, np.float64(c) / np.maximum(m - b, 1e-30), 1.0).astype(np.float32)
    lo, hi = np.nextafter(lo, np.float32(0)), np.minimum(np.nextafter(hi, np.float32(2)), one)
    print("r < 1 at %d of %d samples; largest m %.6f, bound %.3e" % ((r < 1).sum(), len(r), m.max(), b))
    assert ((lo <= r) & (r <= hi)).all() and (r[m + b <= c] == one).all() and (r[m - b > c] < one).all() and (r < 1).sum() > 100
    got_peak = np.array([peak], dtype=np.int32).view(np.float32)[0]
    assert abs(float(got_peak) - m.max()) <= b and peak == _truepeak_top(x, table_dev)


def test_envelope_counts_a_non_finite_sample_as_zero():
    T = _tile()
    rng = np.random.default_rng(6)
    table = _int_table(rng, 4, 24)
    table_dev = torch.from_numpy(table).to(DEV)
    x = rng.integers(-8, 9, (2, T + 50)).astype(np.float32)
    bad = x.copy()
    at = [(0, 0), (0, 5), (1, T - 2), (1, T - 1), (0, T), (1, T + 49)]
    for k, (c, i) in enumerate(at):
        bad[c, i] = (np.nan, np.inf, -np.inf)[k % 3]
        x[c, i] = 0.0
    rc0, r0, p0, ok0 = _envelope(x, table_dev, 3.0)
    rc1, r1, p1, ok1 = _envelope(bad, table_dev, 3.0)
    assert rc0 == rc1 == 0 and ok0 and ok1 and np.array_equal(r0, r1) and p0 == p1
    assert np.array_equal(r0, _bits(LR.ratio(LR.envelope(x, table).astype(np.float32), 3.0)))


# ------------------------------------------------------------------------------------------
# 2. the curve
# ------------------------------------------------------------------------------------------
def _random_r(rng, L, grid=None):
    """Mostly 1, dips alone and in runs, both ends low; `grid`: values on multiples of 1 / grid."""
    r = np.ones(L, dtype=np.float64)
    if L:
        n = max(1, L // 300)
        at = rng.choice(L, n, replace=False)
        r[at] = rng.uniform(0.05, 1.0, n)
        for s in rng.choice(L, max(1, L // 2000), replace=False):
            r[s:s + 40] = rng.uniform(0.3, 1.0, len(r[s:s + 40]))
        r[0] = 0.625
        r[L - 1] = 0.375
    if grid:
        r = np.maximum(np.round(r * grid), 1.0) / grid
    return r.astype(np.float32)


def _x(rng, C, L):
    return rng.uniform(-1.5, 1.5, (C, L)).astype(np.float32)


def _check_apply(x, r, A, H, w, want_g, what):
    """One call against the curve `want_g` (fp32): g, out = x g, the statistics, the canaries, the counter."""
    _count(reset=True)
    rc, out, g, (gmin, count), intact = _apply(x, r, A, H, w)
    L = x.shape[1]
    assert rc == 0 and intact and _count() == (1 if L else 0), (what, rc, intact, _error())
    assert np.array_equal(g, _bits(want_g)), (what, np.flatnonzero(g != _bits(want_g))[:8])
    assert np.array_equal(out, _bits(x * want_g[None, :])), what
    assert _bits(gmin) == _bits(want_g.min() if L else np.float32(1.0)) and count == int((want_g < 1).sum()), (what, gmin, count)
    return g


@pytest.mark.parametrize("A,H", PLANS)
def test_sliding_minimum_is_exact_for_arbitrary_r(A, H):
    """The window a unit impulse: s[i] = d[i - k0] and g = min(r[i], 1.0f - (1.0f - h[i - k0])), the same two roundings in the
    restatement -- at the first tap (the minimum around the sample itself) and at the last (the minimum A samples back)."""
    T = _tile()
    rng = np.random.default_rng(10 * A + H)
    for n, L in enumerate(_lengths(A, H, T, few=A == 1024)):
        C = (1, 2, 5)[n % 3]
        r, x = _random_r(rng, L), _x(rng, C, L)
        for k0 in (0, A):
            w = np.zeros(A + 1, dtype=np.float32)
            w[k0] = 1.0
            _check_apply(x, r, A, H, w, LR.curve32(r, w, A, H), (A, H, L, C, k0))


@pytest.mark.parametrize("A,H", PLANS)
def test_sum_is_exact_on_a_dyadic_grid(A, H):
    """r on the grid of 2^-8 and a window of integers / 4096 that sum to 4096: every product is a multiple of 2^-20 and every
    partial sum at most 1 -- 20 bits, exact in fp32 in any order, so there is one right bit pattern per g."""
    T = _tile()
    rng = np.random.default_rng(20 * A + H)
    cut = np.sort(rng.integers(0, 4097, A))
    w = (np.diff(np.concatenate([[0], cut, [4096]])) / 4096.0).astype(np.float32)
    assert len(w) == A + 1 and w.astype(np.float64).sum() == 1.0
    for n, L in enumerate(_lengths(A, H, T, few=A == 1024)):
        C = (2, 5, 1)[n % 3]
        r, x = _random_r(rng, L, grid=256), _x(rng, C, L)
        want = LR.curve32(r, w, A, H)
        g64, _ = LR.curve(r, w, A, H)
        assert np.array_equal(want.astype(np.float64), g64)        # exact: the order does not matter
        _check_apply(x, r, A, H, w, want, (A, H, L, C))


@pytest.mark.parametrize("A,H", PLANS)
def test_real_window_lies_inside_the_bound_of_the_fp32_sum_and_never_above_r(A, H):
    """|g - g64| <= (A + 1) 2^-24 sum_k |w[k] d[i - k]| -- the worst case of A + 1 roundings of a sum of that size -- plus the
    half ulp of the last subtraction, 1.0f - s in [0, 1]: 2^-25.  g <= r everywhere, g = 1 exactly out of reach of any r < 1,
    out = x g bit for bit, the statistics those of g."""
    from pix2pixhdaudiosr_amd.generate import limiter_window
    T = _tile()
    rng = np.random.default_rng(30 * A + H)
    w = limiter_window(A).numpy()
    L = 2 * T + A + H + 3
    r, x = _random_r(rng, L), _x(rng, 2, L)
    r[100:100 + 2 * A + H + 400] = 1.0                             # a stretch whose middle no r < 1 reaches
    x[0, 7], x[1, 9], x[0, L - 1] = np.inf, -np.inf, np.inf        # pass through the multiply as they are
    rc, out, g, (gmin, count), intact = _apply(x, r, A, H, w)
    assert rc == 0 and intact
    g = g.view(np.float32)
    g64, a = LR.curve(r, w, A, H)
    err, bound = np.abs(g.astype(np.float64) - g64), (A + 1) * 2.0 ** -24 * a + 2.0 ** -25
    print("A %d H %d: largest error %.3e, its bound %.3e, largest error / bound %.3f" % (A, H, err.max(), bound[err.argmax()], (err / bound).max()))
    assert (err <= bound).all()
    assert (g <= r).all() and (g > 0).all()
    reach = LR.reach(r, A, H)
    assert (~reach).any() and (_bits(g[~reach]) == _bits(np.float32(1.0))).all()
    with np.errstate(invalid='ignore'):
        assert np.array_equal(out, _bits(x * g[None, :]))
    assert _bits(gmin) == _bits(g.min()) and count == int((g < 1).sum()) and 0 < count < L


def test_all_ones_r_returns_the_clip():
    T = _tile()
    rng = np.random.default_rng(7)
    from pix2pixhdaudiosr_amd.generate import limiter_window
    for L in (1, T - 1, 2 * T + 5):
        x = _x(rng, 2, L)
        x[0, 0] = np.inf
        rc, out, g, (gmin, count), intact = _apply(x, np.ones(L, dtype=np.float32), 240, 960, limiter_window(240).numpy())
        assert rc == 0 and intact and np.array_equal(out, _bits(x)) and (g == _bits(np.float32(1.0))).all()
        assert _bits(gmin) == _bits(np.float32(1.0)) and count == 0
    # without g_out: the same out
    rc, out2, g2, _, intact = _apply(x, np.ones(L, dtype=np.float32), 240, 960, limiter_window(240).numpy(), want_g=False)
    assert rc == 0 and intact and np.array_equal(out2, out) and (g2 == GUARD_BITS).all()


def test_a_skipped_tile_and_a_computed_tile_give_the_same_bits():
    """Five tiles, A = 72, H = 100, a dyadic window.  One r < 1 sits at the first sample of tile 2: tile 1 is computed only because
    its look-ahead halo holds it, tile 2 holds it, tile 3 only in its look-back halo; tiles 0 and 4 stage nothing but ones and are
    skipped.  A second call adds one r < 1 in the middle of tile 4 and one in tile 0: both are computed now, and wherever the new
    samples do not reach, g and out keep the bits of the skipped run.  Both runs equal the restatement everywhere."""
    T = _tile()
    A, H = 72, 100
    rng = np.random.default_rng(8)
    w = np.full(A + 1, 56.0)                                       # 73 * 56 + 8 = 4096: every tap counts
    w[A // 2] += 8.0
    w = (w / 4096.0).astype(np.float32)
    L = 5 * T
    x = _x(rng, 2, L)
    r = np.ones(L, dtype=np.float32)
    r[2 * T] = 0.25
    g1 = _check_apply(x, r, A, H, w, LR.curve32(r, w, A, H), "one dip").view(np.float32)
    assert (w > 0).all() and w.astype(np.float64).sum() == 1.0
    assert (g1[:2 * T - A] == 1).all() and (g1[2 * T - A:2 * T + H + A + 1] < 1).all() and (g1[2 * T + H + A + 1:] == 1).all()
    assert (g1[T:2 * T] < 1).any() and (g1[3 * T:] == 1).all()    # tile 1 through its halo alone; the reach ends inside tile 2
    r2 = r.copy()
    r2[4 * T + T // 2], r2[5] = 0.5, 0.75
    g2 = _check_apply(x, r2, A, H, w, LR.curve32(r2, w, A, H), "three dips").view(np.float32)
    same = ~LR.reach(np.where(r2 != r, np.float32(0.5), np.float32(1.0)), A, H)           # out of reach of the new dips
    assert same[T:4 * T].all() and same[4 * T:].any() and same[:T].any()
    assert np.array_equal(_bits(g2[same]), _bits(g1[same])) and (g2[~same] < 1).any()
    # a dip that only the look-back halo of the last, short tile sees
    L3 = 2 * T + 9
    r3 = np.ones(L3, dtype=np.float32)
    r3[2 * T - A - H] = 0.5
    _check_apply(x[:, :L3], r3, A, H, w, LR.curve32(r3, w, A, H), "look-back halo")


@pytest.mark.parametrize("grid", (1, 2))
def test_a_workgroup_that_walks_several_tiles_gives_the_same_bits(grid):
    """The option "limiter_grid" makes a workgroup take tiles b, b + gx, ..: both kernels on five tiles, against the restatement
    (integer and dyadic operands) -- the bits of one workgroup per tile."""
    L_ = _lib()
    T = _tile()
    rng = np.random.default_rng(40 + grid)
    table = _int_table(rng, 4, 24)
    table_dev = torch.from_numpy(table).to(DEV)
    L = 4 * T + 9
    xi = rng.integers(-8, 9, (2, L)).astype(np.float32)
    m32 = LR.envelope(xi, table).astype(np.float32)
    A, H = 7, 3
    w = (np.array([1, 2, 3, 4, 3, 2, 1, 0]) / 16.0).astype(np.float32)
    r, x = _random_r(rng, L, grid=256), _x(rng, 2, L)
    assert L_.lib().p2phd_set_option(b"limiter_grid", grid) == 0
    try:
        rc, rb, peak, intact = _envelope(xi, table_dev, 6.5)
        assert rc == 0 and intact and np.array_equal(rb, _bits(LR.ratio(m32, 6.5))) and peak == int(_bits(m32).max())
        _check_apply(x, r, A, H, w, LR.curve32(r, w, A, H), "walked")
    finally:
        assert L_.lib().p2phd_set_option(b"limiter_grid", 0) == 0
    assert L_.lib().p2phd_set_option(b"limiter_grid", -1) != 0 and L_.lib().p2phd_set_option(b"limiter_grid", 16385) != 0


# ------------------------------------------------------------------------------------------
# 3. the tensor functions, the counter, the refusals
# ------------------------------------------------------------------------------------------
def test_limit_is_the_two_launches_in_a_row():
    from pix2pixhdaudiosr_amd import generate as G
    rng = np.random.default_rng(9)
    T = _tile()
    x = torch.from_numpy((0.4 * rng.standard_normal((2, 2 * T + 301))).astype(np.float32)).to(DEV)
    ceiling = 0.5
    _count(reset=True)
    out, g, stats, peak = G.limit(x, 48000, ceiling, 1.5, 0.0)
    assert _count() == 2                                           # two launches per clip
    r, peak2 = G.limiter_envelope(x, 48000, ceiling)
    out2, g2, stats2 = G.limiter_apply(x, r, {'lookahead': 72, 'hold': 0})
    assert _count() == 4 and torch.equal(out, out2) and torch.equal(g, g2) and torch.equal(stats, stats2) and torch.equal(peak, peak2)
    tpeak, _ = G.true_peaks(x, 48000)
    assert float(peak[0]) == float(tpeak.max())
    gn, rn = g.cpu().numpy(), r.cpu().numpy()
    assert (gn <= rn).all() and (rn < 1).any() and torch.equal(out, x * g[None, :])
    assert stats[:4].view(torch.float32).item() == gn.min() and stats[4:].view(torch.int32).item() == int((gn < 1).sum())
    # the limited clip's own true peak: at the ceiling, a hair over at most -- a measurement, printed, not bounded here
    after, _ = G.true_peaks(out, 48000)
    print("true peak in %.6f, out %.6f, ceiling %.6f: overshoot %+.5f dB" % (float(peak[0]), float(after.max()), ceiling,
                                                                            20.0 * np.log10(float(after.max()) / ceiling)))
    assert float(after.max()) < float(peak[0])
    # an empty clip: nothing is launched that counts, the statistics are 1 and 0
    _count(reset=True)
    out0, g0, stats0, peak0 = G.limit(x[:, :0], 48000, ceiling)
    torch.cuda.synchronize()
    assert _count() == 0 and out0.shape == (2, 0) and float(peak0[0]) == 0.0
    assert stats0[:4].view(torch.float32).item() == 1.0 and stats0[4:].view(torch.int32).item() == 0


def test_bad_arguments_return_the_error_text_and_launch_nothing():
    rng = np.random.default_rng(11)
    table_dev = torch.from_numpy(_int_table(rng, 4, 24)).to(DEV)
    x = rng.integers(-8, 9, (2, 100)).astype(np.float32)
    _count(reset=True)
    for kw, word in ((dict(factor=3), "factor"), (dict(taps=23), "taps_per_phase"), (dict(taps=66), "taps_per_phase"), (dict(frames=104), "ld"),
                     (dict(frames=-1), "frames")):
        rc, r, peak, intact = _envelope(x, table_dev, 1.0, **kw)
        assert rc != 0 and intact and (r == GUARD_BITS).all() and peak == GUARD_BITS and word in _error(), (kw, _error())
    for ceiling in (0.0, -1.0, float('inf'), float('nan')):
        rc, r, peak, intact = _envelope(x, table_dev, ceiling)
        assert rc != 0 and intact and (r == GUARD_BITS).all() and "ceiling" in _error()
    w = np.full(8, 0.125, dtype=np.float32)
    r1 = np.ones(100, dtype=np.float32)
    for kw, word in ((dict(lookahead=0), "lookahead"), (dict(lookahead=1025), "lookahead"), (dict(hold=-1), "hold"), (dict(hold=4097), "hold"),
                     (dict(frames=103), "ld"), (dict(frames=-1), "frames")):
        rc, out, g, stats, intact = _apply(x, r1, 7, 3, w, **kw)
        assert rc != 0 and intact and (out == GUARD_BITS).all() and (g == GUARD_BITS).all() and word in _error(), (kw, _error())
    L_ = _lib()
    buf = torch.zeros(256, dtype=torch.float32, device=DEV)
    odd = buf.view(torch.uint8)[2:].data_ptr()
    assert L_.lib().p2phd_limiter_envelope(odd, 10, 1, 10, L_.ptr(table_dev), 4, 24, 1.0, L_.ptr(buf[64:]), L_.ptr(buf[128:]), L_.stream_ptr()) != 0
    assert "aligned" in _error()
    assert L_.lib().p2phd_limiter_apply(L_.ptr(buf), 10, 1, 10, L_.ptr(buf[32:]), 7, 3, L_.ptr(buf[64:]), L_.ptr(buf), 10, None, L_.ptr(buf[128:]),
                                        L_.stream_ptr()) != 0
    assert "overlaps" in _error()
    assert L_.lib().p2phd_limiter_apply(L_.ptr(buf), 10, 1, 10, L_.ptr(buf[32:]), 7, 3, L_.ptr(buf[64:]), L_.ptr(buf[96:]), 10, None, None,
                                        L_.stream_ptr()) != 0
    assert "null" in _error()
    torch.cuda.synchronize()
    assert _count() == 0
