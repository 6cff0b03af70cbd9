"""The true-peak measurement on the GPU (csrc/truepeak.hip: p2phd_truepeak; generate.true_peaks): integer operands against the
float64 restatement of tests/_truepeak_ref.py bit for bit, float operands inside the worst-case bound of an fp32 dot product,
non-finite samples, the gain rule, refusals, and what the guard does to a tone whose samples miss its crests.  Every call writes
`tpeak` and `gain` between canaries; the rows sit at the pitches and 16-byte offsets of tests/test_gpu_xover.py."""
import numpy as np
import pytest
import torch

import _truepeak_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                         # words on either side of an output
GUARD_BITS = 0x7FC0BEEF                                            # a NaN pattern no kernel writes
OFFSETS = (0, 1, 3, 0, 3)                                          # floats past a 16-byte boundary
PITCHES = (5, 2, 3, 1, 64, 9)                                      # floats between the end of a row and the next one


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _tile():
    return int(_lib().lib().p2phd_truepeak_tile_len())


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"truepeak", 1 if reset else 0)


def _placed(a, pitch, off):
    """Rows of `a` [C, L] at `pitch` floats apart, the first one `off` floats past a 16-byte boundary -> (buffer, view of row 0)."""
    C, L = a.shape
    host = np.full(4 + off + C * pitch + 4, np.float32(77.0))
    for c in range(C):
        host[4 + off + c * pitch:4 + off + c * pitch + L] = a[c]
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[4 + off:]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _call(x, table, ceiling=1.0, case=0, table_dev=None, factor=None, taps=None, frames=None):
    """p2phd_truepeak on rows placed as case `case` asks -> (return code, tpeak [C] f32, gain f32, canaries intact)."""
    L_ = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    C, L = x.shape
    ld = L + PITCHES[case % len(PITCHES)]
    keep, rows = _placed(x, ld, OFFSETS[case % len(OFFSETS)])
    if table_dev is None:
        table_dev = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).to(DEV)
    F, P = table_dev.shape
    # canaries | tpeak [C] | canaries | gain | canaries
    buf = torch.full((GUARD + C + GUARD + 1 + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    tpeak, gain = buf[GUARD:], buf[GUARD + C + GUARD:]
    rc = L_.lib().p2phd_truepeak(L_.ptr(rows), L if frames is None else frames, C, ld, L_.ptr(table_dev), F if factor is None else factor,
                                 P if taps is None else taps, float(ceiling), L_.ptr(tpeak), L_.ptr(gain), L_.stream_ptr())
    torch.cuda.synchronize()
    bits = buf.view(torch.int32).cpu().numpy()
    mask = np.ones(bits.shape, dtype=bool)
    mask[GUARD:GUARD + C] = False
    mask[GUARD + C + GUARD] = False
    intact = bool((bits[mask] == GUARD_BITS).all())
    return rc, bits[GUARD:GUARD + C].copy().view(np.float32), bits[GUARD + C + GUARD:GUARD + C + GUARD + 1].copy().view(np.float32)[0], intact


def _want(x, table, ceiling=1.0):
    """The restatement on the fp32 operands -> (tpeak [C] as fp32, gain fp32); asserts that every peak is an fp32 number."""
    tp = R.true_peak(x, table)
    t32 = tp.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), tp)
    return t32, R.gain(t32, ceiling)


# ------------------------------------------------------------------------------------------
# 1. exact: every product and partial sum is representable, so there is one right bit pattern per peak
# ------------------------------------------------------------------------------------------
def _int_table(rng, F, P, lo=-4, hi=4):
    t = rng.integers(lo, hi + 1, (F, P)).astype(np.float32)
    t[:, 0] = rng.choice([-3, -1, 1, 2], F)                        # both end taps count, the table is not symmetric
    t[:, -1] = rng.choice([-2, 1, 3], F)
    return t / np.float32(16.0)


def _mirrored(table):
    """c'[p][k] = c[F - p][P - 1 - k] (phase 0, which is not read, stays)."""
    out = table.copy()
    for p in range(1, table.shape[0]):
        out[p] = table[table.shape[0] - p][::-1]
    return out


def _lengths(P, T):
    return sorted({L for L in (1, 2, P - 1, P, P + 1, T - 1, T, T + 1, 2 * T + 5, 10007) if L >= 1})


@pytest.mark.parametrize("F", (1, 2, 4))
@pytest.mark.parametrize("P", (4, 24, 64))
def test_integer_operands_are_exact(F, P):
    """Samples integers in [-8, 8], coefficients integers in [-4, 4] / 16: products in 1/16, sums below 64 * 8 * 4 / 16 = 128 --
    12 bits at most, exact in fp32 whatever the order.  Every length around the taps and the tile, one and three rows, and the
    time-reversed clip with the mirrored table, which holds the same set of sums."""
    T = _tile()
    rng = np.random.default_rng(1000 * F + P)
    table = _int_table(rng, F, P)
    table_dev, mirror_dev = torch.from_numpy(table).to(DEV), torch.from_numpy(_mirrored(table)).to(DEV)
    xs = rng.integers(-8, 9, (3, 10007)).astype(np.float32)
    case = 0
    for L in _lengths(P, T):
        for C in (1, 3):
            x = xs[:C, :L]
            want, want_gain = _want(x, table, 0.75)
            _count(reset=True)
            rc, got, gain, intact = _call(x, table, 0.75, case, table_dev)
            assert rc == 0 and intact and _count() == 1, (L, C, rc, intact)
            assert np.array_equal(_bits(got), _bits(want)) and _bits(gain) == _bits(want_gain), (L, C, got, want, gain, want_gain)
            rc, rev, gain, intact = _call(x[:, ::-1], None, 0.75, case + 1, mirror_dev)
            assert rc == 0 and intact and np.array_equal(_bits(rev), _bits(want)) and _bits(gain) == _bits(want_gain), (L, C, rev, want)
            case += 1


@pytest.mark.parametrize("grid", (1, 2, 3))
def test_a_workgroup_that_walks_several_tiles_gives_the_same_bits(grid):
    """A clip with more tiles than the partial table has rows makes a workgroup take tiles b, b + gx, ...: the option
    "truepeak_grid" runs that path at five tiles, with integer operands against the restatement and with float operands against
    the run of one workgroup per tile."""
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients
    L_ = _lib()
    T = _tile()
    rng = np.random.default_rng(40 + grid)
    table = _int_table(rng, 4, 24)
    x = rng.integers(-8, 9, (3, 4 * T + 9)).astype(np.float32)
    x[1, :3 * T] = np.clip(x[1, :3 * T], -2, 2)                    # row 1 has its peak in the last tiles, row 2 in the first
    x[2, T:] = np.clip(x[2, T:], -2, 2)
    real = true_peak_coefficients(4, 24, 9.0).numpy()
    xf = (0.3 * rng.standard_normal((2, 4 * T + 9))).astype(np.float32)
    rc, plain, gain_plain, intact = _call(xf, real, 0.25, case=1)
    assert rc == 0 and intact
    want, want_gain = _want(x, table, 0.75)
    assert L_.lib().p2phd_set_option(b"truepeak_grid", grid) == 0
    try:
        _count(reset=True)
        rc, got, gain, intact = _call(x, table, 0.75, case=2)
        assert rc == 0 and intact and _count() == 1
        assert np.array_equal(_bits(got), _bits(want)) and _bits(gain) == _bits(want_gain), (got, want)
        rc, walked, gain_walked, intact = _call(xf, real, 0.25, case=3)
        assert rc == 0 and intact and np.array_equal(_bits(walked), _bits(plain)) and _bits(gain_walked) == _bits(gain_plain)
    finally:
        assert L_.lib().p2phd_set_option(b"truepeak_grid", 0) == 0
    assert L_.lib().p2phd_set_option(b"truepeak_grid", -1) != 0 and L_.lib().p2phd_set_option(b"truepeak_grid", 65537) != 0


def _planted(F, P, T, where, rng):
    """A clip of length 2 T + 5 and a table whose largest magnitude arises at one instant and phase alone -> (x [1, L], table,
    (instant i, phase p)).  Phase p* holds +-4/16 in every tap, the other phases at most 1/16; the samples under the window of the
    planted instant are 8 sign(c[p*][k]), the rest of the clip is 0: the planted sum is 2 per sample under the window, any other
    phase reaches an eighth of that, and another instant of phase p* lines the samples up with other taps."""
    L, h = 2 * T + 5, P // 2 - 1
    p_star = F - 1 if where == 'phase' else 1
    table = _int_table(rng, F, P, -1, 1)
    table[:, 0], table[:, -1] = np.sign(table[:, 0]) / np.float32(16.0), np.sign(table[:, -1]) / np.float32(16.0)
    table[p_star] = rng.choice([-0.25, 0.25], P).astype(np.float32)
    i = {'first': -1, 'last': L - 1, 'boundary': T - 1, 'boundary_left': T - 2, 'phase': T + 301}[where]
    x = np.zeros((1, L), dtype=np.float32)
    for k in range(P):
        n = i + k - h
        if 0 <= n < L:
            x[0, n] = 8.0 * np.sign(table[p_star, k])
    return x, table, (i, p_star)


@pytest.mark.parametrize("F", (2, 4))
@pytest.mark.parametrize("P", (4, 24, 64))
@pytest.mark.parametrize("where", ('first', 'last', 'boundary', 'boundary_left', 'phase'))
def test_the_largest_magnitude_in_one_place_alone(F, P, where):
    """The maximum planted at instant i = -1 (only the last P / 2 taps meet samples), at the last instant i = L - 1 (only the first
    P / 2), at the first and the last instant of a tile (the window straddles the tile boundary: halo on either side) and in phase
    F - 1.  The restatement confirms that no other (instant, phase) reaches it.  With P = 4 no fractional phase can exceed the
    largest sample under its window (the taps' magnitudes sum to at most 4 * 4 / 16 = 1), so there the place cannot be unique --
    the peak is then the sample's 8 and the call is checked for its bits all the same."""
    T = _tile()
    x, table, (i, p) = _planted(F, P, T, where, np.random.default_rng(7 * F + P))
    y = np.abs(R.oversampled(x[0], table))
    if P > 4:
        at = np.argwhere(y == y.max())
        assert at.tolist() == [[i + 1, p]], (where, at[:4].tolist(), y.max())
        assert y.max() == 2.0 * (P // 2 if where in ('first', 'last') else P) and y.max() > np.abs(x).max()
    want, want_gain = _want(x, table, 0.5)
    rc, got, gain, intact = _call(x, table, 0.5, case=F + P)
    assert rc == 0 and intact and _bits(got)[0] == _bits(want)[0] and _bits(gain) == _bits(want_gain), (got, want)


def test_one_phase_is_the_sample_peak():
    """F = 1: nothing is interpolated; the largest sample at the last instant and on either side of a tile boundary."""
    T = _tile()
    rng = np.random.default_rng(5)
    table = _int_table(rng, 1, 24)
    for n in (0, T - 2, T - 1, T, 2 * T + 4):
        x = rng.integers(-7, 8, (2, 2 * T + 5)).astype(np.float32)
        x[1, n] = -8.0
        rc, got, gain, intact = _call(x, table, 1.0, case=n)
        assert rc == 0 and intact and got.tolist() == [np.abs(x[0]).max(), 8.0] and gain == np.float32(1.0) / np.float32(8.0)


# ------------------------------------------------------------------------------------------
# 2. float operands
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (48000, 96000))
def test_float_operands_within_the_dot_product_bound(rate):
    """|tpeak - ref| <= P 2^-24 max_p sum_k |c x|: the worst case of an fp32 dot product of P terms, taken over every sum of the row
    (a maximum moves by no more than its operands do).  And tpeak >= the peak of pcm_peaks, exactly: phase 0 is the samples."""
    from pix2pixhdaudiosr_amd.generate import pcm_peaks, true_peak_coefficients, true_peaks, truepeak_plan
    plan = truepeak_plan(rate)
    table = true_peak_coefficients(plan['factor'], plan['taps_per_phase'], plan['beta']).numpy()
    T = _tile()
    rng = np.random.default_rng(rate)
    x = (0.3 * rng.standard_normal((3, 2 * T + 301))).astype(np.float32)
    x[2] *= np.float32(0.01)
    want, bound = R.true_peak(x, table), R.dot_bound(x, table)
    rc, got, gain, intact = _call(x, table, 0.25, case=2)
    assert rc == 0 and intact
    err = np.abs(got.astype(np.float64) - want)
    print("rate %d: tpeak %s, error / bound %s, gain %r" % (rate, got, err / bound, gain))
    assert (bound > 0).all() and (err <= bound).all()
    assert _bits(gain) == _bits(R.gain(got, 0.25))
    xd = torch.from_numpy(x).to(DEV)
    peak = pcm_peaks(xd, 'float32')[0].cpu().numpy()
    assert (got >= peak).all() and (peak == np.abs(x).max(axis=1)).all()
    assert (got > peak).any()                                      # (Gaussian rows: some crest lies between the samples)
    # the binding: the same kernel on a contiguous tensor, and on a view with another pitch
    tp, g = true_peaks(xd, rate, 0.25)
    assert tp.dtype == torch.float32 and tuple(tp.shape) == (3,) and tuple(g.shape) == (1,)
    assert np.array_equal(_bits(tp.cpu().numpy()), _bits(got)) and _bits(g.cpu().numpy())[0] == _bits(gain)
    wide = torch.zeros((3, x.shape[1] + 13), device=DEV)
    wide[:, 5:5 + x.shape[1]].copy_(xd)
    tp2, g2 = true_peaks(wide[:, 5:5 + x.shape[1]], rate, 0.25)
    assert torch.equal(tp2.view(torch.int32), tp.view(torch.int32)) and torch.equal(g2.view(torch.int32), g.view(torch.int32))


def test_non_finite_samples_count_as_zero():
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients
    table = true_peak_coefficients(4, 24, 9.0).numpy()
    T = _tile()
    rng = np.random.default_rng(11)
    x = (0.3 * rng.standard_normal((2, T + 77))).astype(np.float32)
    bad = x.copy()
    zeroed = x.copy()
    for n, v in ((0, np.nan), (5, np.inf), (T - 2, -np.inf), (T - 1, np.nan), (T, np.inf), (T + 76, -np.inf)):
        bad[:, n] = v
        zeroed[:, n] = 0.0
    rc, got, gain, intact = _call(bad, table, 0.5, case=1)
    rc0, want, gain0, intact0 = _call(zeroed, table, 0.5, case=3)
    assert rc == 0 and rc0 == 0 and intact and intact0
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want)) and _bits(gain) == _bits(gain0)
    # a row without a finite sample reads 0
    rc, got, gain, intact = _call(np.full((1, 300), np.nan, dtype=np.float32), table, 0.5)
    assert rc == 0 and intact and _bits(got)[0] == 0 and gain == 1.0


# ------------------------------------------------------------------------------------------
# 3. the gain, empty clips, repeatability, the launch count
# ------------------------------------------------------------------------------------------
def test_gain_rule_empty_clip_and_repeatability():
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients
    table = true_peak_coefficients(4, 24, 9.0).numpy()
    rng = np.random.default_rng(3)
    x = (0.2 * rng.standard_normal((2, 5000))).astype(np.float32)
    x[1] *= np.float32(0.5)                                        # one gain for all channels: the louder one decides
    _count(reset=True)
    rc, tp, gain, intact = _call(x, table, 1e-3)
    assert rc == 0 and intact and _count() == 1 and tp[0] > tp[1]
    assert _bits(gain) == _bits(np.float32(1e-3) / tp[0])          # one fp32 division
    for ceiling in (0.1, 0.5, float(tp[0]), 3.0):
        rc, again, gain, intact = _call(x, table, ceiling, case=4)
        assert rc == 0 and intact and np.array_equal(_bits(again), _bits(tp))      # a run repeats, wherever the rows lie
        assert _bits(gain) == _bits(R.gain(tp, ceiling))
        assert (gain == 1.0) == (np.float32(ceiling) >= tp[0])
    assert _count() == 5
    # frames = 0: zeros and gain 1, written, not counted
    _count(reset=True)
    rc, tp0, gain0, intact = _call(x, table, 0.5, frames=0)
    assert rc == 0 and intact and _bits(tp0).tolist() == [0, 0] and gain0 == 1.0 and _count() == 0
    L_ = _lib()
    out = torch.full((4,), 7.0, device=DEV)
    td = torch.from_numpy(table).to(DEV)
    assert L_.lib().p2phd_truepeak(None, 0, 1, 0, L_.ptr(td), 4, 24, 0.5, L_.ptr(out), L_.ptr(out[2:]), L_.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0.0, 7.0, 1.0, 7.0] and _count() == 0


def test_the_guard_holds_the_true_peak_of_a_tone():
    """A tone at a quarter of the rate with 45 degrees of phase, amplitude 0.9: its samples read 3.01 dB under its crests.  Scaled
    by the true-peak gain the decoded float32 payload has its true peak, measured by the restatement, at the ceiling -- within
    the dot-product bound; scaled by the sample-peak gain it stays about 3 dB over."""
    from pix2pixhdaudiosr_amd.generate import pcm_encode, pcm_peaks, true_peak_coefficients, true_peaks
    table = true_peak_coefficients(4, 24, 9.0).numpy()
    x = R.ramped_tone(0.25, np.pi / 4, amplitude=0.9).astype(np.float32)[None]
    xd = torch.from_numpy(x).to(DEV)
    _count(reset=True)
    peak, _, _, gain_s = pcm_peaks(xd, 'float32', ceiling=0.5)
    tp, gain_t = true_peaks(xd, 48000, ceiling=0.5)
    assert _count() == 1
    assert float(tp[0]) == pytest.approx(0.9, abs=1e-3) and float(peak[0]) == pytest.approx(0.9 * np.sqrt(0.5), abs=1e-4)
    results = {}
    for name, g in (('true', gain_t), ('sample', gain_s)):
        y = pcm_encode(xd, 'float32', gain=g).cpu().numpy().view(np.float32)
        results[name] = (R.true_peak(y, table), R.dot_bound(y[None], table)[0], np.abs(y).max())
    got, bound, _ = results['true']
    print("true-peak gain %r: true peak %.9f (bound %.3e); sample-peak gain %r: true peak %.6f, sample peak %.6f"
          % (float(gain_t[0]), got, bound, float(gain_s[0]), results['sample'][0], results['sample'][2]))
    assert abs(got - 0.5) <= bound
    over_db = 20.0 * np.log10(results['sample'][0] / 0.5)
    assert abs(over_db - 3.0103) <= 0.01 and abs(results['sample'][2] - 0.5) <= 1e-6


# ------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------
def test_refusals():
    L_ = _lib()
    lib = L_.lib()
    C, L, ld = 2, 300, 310
    table = torch.full((4, 24), 0.1, device=DEV)
    buf = torch.full((4 * 1024,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    rows, tpeak, gain = buf[1024:], buf[2048:], buf[3072:]
    st = L_.stream_ptr()
    einval = lib.p2phd_segments_stitch(None, 0, 0, 0, 1.0, None, 0, st)          # P2PHD_EINVAL of a neighbour
    assert einval != 0
    _count(reset=True)
    p = L_.ptr

    def refused(word, *args):
        rc = lib.p2phd_truepeak(*args)
        text = lib.p2phd_last_error().decode()
        assert rc == einval and "truepeak" in text and word in text, (word, rc, text)

    for factor in (0, 3, 8, -1):
        refused("factor", p(rows), L, C, ld, p(table), factor, 24, 0.5, p(tpeak), p(gain), st)
    for taps in (0, 2, 23, 66, 65, -4):
        refused("taps_per_phase", p(rows), L, C, ld, p(table), 4, taps, 0.5, p(tpeak), p(gain), st)
    for ceiling in (0.0, -1.0, float('nan'), float('inf')):
        refused("ceiling", p(rows), L, C, ld, p(table), 4, 24, ceiling, p(tpeak), p(gain), st)
    two = lambda t: L_.C.c_void_p(t.data_ptr() + 2)                                 # noqa: E731
    for args in ((two(rows), L, C, ld, p(table), 4, 24, 0.5, p(tpeak), p(gain), st), (p(rows), L, C, ld, two(table), 4, 24, 0.5, p(tpeak), p(gain), st),
                 (p(rows), L, C, ld, p(table), 4, 24, 0.5, two(tpeak), p(gain), st), (p(rows), L, C, ld, p(table), 4, 24, 0.5, p(tpeak), two(gain), st)):
        refused("aligned", *args)
    for args in ((None, L, C, ld, p(table), 4, 24, 0.5, p(tpeak), p(gain), st), (p(rows), L, C, ld, None, 4, 24, 0.5, p(tpeak), p(gain), st),
                 (p(rows), L, C, ld, p(table), 4, 24, 0.5, None, p(gain), st), (p(rows), L, C, ld, p(table), 4, 24, 0.5, p(tpeak), None, st)):
        refused("null", *args)
    refused("ld", p(rows), L, C, L - 1, p(table), 4, 24, 0.5, p(tpeak), p(gain), st)
    refused("channels", p(rows), L, 0, ld, p(table), 4, 24, 0.5, p(tpeak), p(gain), st)
    refused("frames", p(rows), -1, C, ld, p(table), 4, 24, 0.5, p(tpeak), p(gain), st)
    torch.cuda.synchronize()
    assert _count() == 0                                           # nothing launched
    assert bool((buf.view(torch.int32) == GUARD_BITS).all())       # nothing written
    # the binding's own checks
    from pix2pixhdaudiosr_amd.generate import true_peaks
    a = torch.zeros((2, 100), device=DEV)
    for bad in (0.0, -0.5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match="ceiling"):
            true_peaks(a, 48000, bad)
    with pytest.raises(ValueError, match="truepeak_plan"):
        true_peaks(a, 0)
    with pytest.raises(L_.P2PHDError, match=r"float32 tensor on the GPU"):
        true_peaks(a.cpu(), 48000)
    with pytest.raises(L_.P2PHDError, match=r"rows that are contiguous"):
        true_peaks(a[:, ::2], 48000)
