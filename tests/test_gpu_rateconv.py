"""The rate converter of the output stage on the GPU (csrc/rateconv.hip: p2phd_rateconv_fwd; generate.rate_convert): integer
operands against the int64 restatement of tests/_rateconv_ref.py bit for bit -- every (o, n) shape of the tiling, every length
around the taps and the tile -- float operands inside the worst-case bound of an fp32 dot product, non-finite samples, runs and
streams, the launch counter and every refusal.  Every call writes its rows between canaries; the input rows sit at the pitches
and 16-byte offsets of tests/test_gpu_truepeak.py."""
import numpy as np
import pytest
import torch

import _rateconv_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD_BITS = 0x7FC0BEEF                                            # a NaN pattern no kernel writes
OFFSETS = (0, 1, 3, 0, 3)                                          # floats past a 16-byte boundary
PITCHES = (5, 2, 3, 1, 64, 9)                                      # floats between the end of a row and the next one
# the issue's shapes; then one whose phases do not fit one chunk (n > 1024) and one whose o / n also shrinks the chunk
PAIRS = ((1, 2), (2, 1), (3, 2), (2, 3), (160, 147), (147, 160))
WIDE_PAIRS = ((1000, 1201), (5000, 1201))
TAPS = (4, 10, 92, 256)


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _tile(o, n, P):
    T = int(_lib().lib().p2phd_rateconv_tile_len(o, n, P))
    assert T > 0
    return T


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"rateconv", 1 if reset else 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _placed(a, pitch, off):
    """Rows of `a` [C, L] at `pitch` floats apart, the first one `off` floats past a 16-byte boundary -> (buffer, view of row 0)."""
    C, L = a.shape
    host = np.full(4 + off + C * pitch + 4, np.float32(77.0))
    for c in range(C):
        host[4 + off + c * pitch:4 + off + c * pitch + L] = a[c]
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[4 + off:]


def _call(x, table_dev, o, n, case=0, over=None):
    """p2phd_rateconv_fwd on rows placed as case `case` asks -> (return code, out [C, L_out] f32, canaries intact).  `over`: arguments
    to hand over in place of the right ones (the refusals)."""
    L_ = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    C, L = x.shape
    P = table_dev.numel() // n
    ld = L + PITCHES[case % len(PITCHES)]
    off = OFFSETS[case % len(OFFSETS)]
    keep, rows = _placed(x, ld, off)
    Lo = R.out_len(L, o, n)
    out_ld = Lo + PITCHES[(case + 1) % len(PITCHES)]
    # canaries | row 0 | canaries up to the pitch | row 1 | ... ; the first row `off` floats past a 16-byte boundary as well
    buf = torch.full((8 + off + C * out_ld + 8,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    out = buf[8 + off:]
    a = dict(planar=L_.ptr(rows), frames=L, channels=C, ld=ld, table=L_.ptr(table_dev), o=o, n=n, P=P, out=L_.ptr(out), out_frames=Lo, out_ld=out_ld)
    a.update(over or {})
    rc = L_.lib().p2phd_rateconv_fwd(a['planar'], a['frames'], a['channels'], a['ld'], a['table'], a['o'], a['n'], a['P'], a['out'], a['out_frames'],
                                     a['out_ld'], L_.stream_ptr())
    torch.cuda.synchronize()
    bits = buf.view(torch.int32).cpu().numpy()
    mask = np.ones(bits.shape, dtype=bool)
    got = np.zeros((C, Lo), dtype=np.float32)
    for c in range(C):
        lo = 8 + off + c * out_ld
        mask[lo:lo + Lo] = False
        got[c] = bits[lo:lo + Lo].view(np.float32)
    if rc != 0:
        mask[:] = True                                             # a refused call writes nothing at all
    return rc, got, bool((bits[mask] == GUARD_BITS).all())


def _int_table(rng, n, P):
    t = rng.integers(-4, 5, (n, P)).astype(np.int64)
    t[:, 0] = rng.choice([-3, -1, 1, 2], n)                        # both end taps count
    t[:, -1] = rng.choice([-2, 1, 3], n)
    return t


def _lengths(o, n, P):
    T = _tile(o, n, P)
    return sorted({0, 1, P // 2, P, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1})


def _exact(o, n, P, seed):
    rng = np.random.default_rng(seed)
    table = _int_table(rng, n, P)
    table_dev = torch.from_numpy(table.astype(np.float32)).to(DEV)
    lengths = _lengths(o, n, P)
    xs = rng.integers(-64, 65, (3, max(lengths))).astype(np.int64)
    case = 0
    for L in lengths:
        want = np.stack([R.convert(xs[c, :L], table, o, n) for c in range(3)])
        assert want.dtype == np.int64 and want.shape == (3, R.out_len(L, o, n)) and np.abs(want).max(initial=0) < 2 ** 24
        for C in (1, 3):
            _count(reset=True)
            rc, got, intact = _call(xs[:C, :L], table_dev, o, n, case)
            assert rc == 0 and intact and _count() == (1 if L else 0), (o, n, P, L, C, rc, intact, _count())
            assert np.array_equal(_bits(got), _bits(want[:C].astype(np.float32))), (o, n, P, L, C)
            case += 1


# ------------------------------------------------------------------------------------------
# 1. exact: every product and partial sum is an integer below 2^24, so there is one right bit pattern per output
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", TAPS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dto%d" % p)
def test_integer_operands_are_exact(pair, P):
    """Tables of integers in [-4, 4], samples in [-64, 64]: sums below 256 * 4 * 64 = 2^16, exact in fp32 whatever the order.  L = 0,
    1, P / 2, P and one below, at and above the first two tile boundaries; one and three rows at pitches above L, offset from 16-byte
    alignment, canaries around every output row.  P = 256 at 160 -> 147 and 147 -> 160 walks the taps in runs (the table does not
    fit beside the samples)."""
    _exact(pair[0], pair[1], P, 1000 * pair[0] + 10 * pair[1] + P)


@pytest.mark.parametrize("P", (4, 10))
@pytest.mark.parametrize("pair", WIDE_PAIRS, ids=lambda p: "%dto%d" % p)
def test_phases_in_several_chunks_are_exact(pair, P):
    """n = 1201 phases do not fit one workgroup's chunk (1024 at most; fewer where o / n spreads them over more samples than a
    segment holds): the grid then carries the chunk beside the run of blocks."""
    _exact(pair[0], pair[1], P, 7 * pair[0] + P)


def test_nonfinite_samples_are_samples():
    """An infinite or NaN sample is not special-cased: every output whose window holds one is what IEEE arithmetic makes of it (0 *
    inf is NaN), every other output is exact."""
    o, n, P = 160, 147, 10
    rng = np.random.default_rng(5)
    table = _int_table(rng, n, P)
    x = rng.integers(-64, 65, (1, 5000)).astype(np.float64)
    x[0, [7, 1234, 4999]] = [np.inf, np.nan, -np.inf]
    with np.errstate(invalid='ignore'):
        want = R.convert(x[0], table, o, n).astype(np.float32)
    rc, got, intact = _call(x, torch.from_numpy(table.astype(np.float32)).to(DEV), o, n, 2)
    assert rc == 0 and intact
    finite = np.isfinite(want)
    assert 0 < (~finite).sum() < 3 * (P + 2) and np.array_equal(np.isnan(got[0]), np.isnan(want))
    assert np.array_equal(_bits(got[0][finite]), _bits(want[finite])) and np.array_equal(got[0][np.isinf(want)], want[np.isinf(want)])


# ------------------------------------------------------------------------------------------
# 2. float operands: the real table on noise
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real():
    from pix2pixhdaudiosr_amd import generate as g
    plan = g.rateconv_plan(48000, 44100)
    table = g.rateconv_coefficients(plan)
    return plan, table.numpy(), table.to(DEV)


def test_noise_stays_inside_the_dot_product_bound(real):
    """The 48000 -> 44100 table (92 taps x 147 phases) on noise at -12 dBFS: every output within P 2^-24 sum |c x| of the float64
    sum over the same fp32 operands -- the worst case of an fp32 fma chain of P terms (_truepeak_ref.dot_bound's model: one
    rounding per tap, none of the partial sums above the absolute sum)."""
    plan, table, table_dev = real
    o, n = plan['o'], plan['n']
    rng = np.random.default_rng(11)
    x = (0.25 * rng.standard_normal((3, 2 * _tile(o, n, 92) + 77))).astype(np.float32)
    rc, got, intact = _call(x, table_dev, o, n, 3)
    assert rc == 0 and intact
    worst = 0.0
    for c in range(3):
        want, bound = R.convert(x[c], table, o, n), R.dot_bound(x[c], table, o, n)
        err = np.abs(got[c].astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-30)).max()))
        assert np.all(err <= bound), (c, float(err.max()), float(bound[np.argmax(err)]))
    print("largest error / bound: %.3f" % worst)


def test_two_runs_and_two_streams_give_the_same_bits(real):
    from pix2pixhdaudiosr_amd import generate as g
    plan, _, table_dev = real
    rng = np.random.default_rng(12)
    x = torch.from_numpy((0.25 * rng.standard_normal((2, 50001))).astype(np.float32)).to(DEV)
    first = g.rate_convert(x, 48000, 44100)
    again = g.rate_convert(x, 48000, 44100, plan=plan, table=table_dev)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(g.rate_convert(x, 48000, 44100))
    torch.cuda.synchronize()
    assert first.shape == (2, g.rateconv_out_len(50001, 48000, 44100))
    for t in [again] + outs:
        assert torch.equal(t.view(torch.int32), first.view(torch.int32))
    # a row of a call is the call on that row
    assert torch.equal(g.rate_convert(x[1:], 48000, 44100).view(torch.int32), first[1:].view(torch.int32))


def test_rate_convert_arguments(real):
    from pix2pixhdaudiosr_amd import generate as g
    plan, _, table_dev = real
    x = torch.zeros((2, 1000), device=DEV)
    _count(reset=True)
    assert g.rate_convert(x, 48000, 48000) is x and _count() == 0          # equal rates: the input itself
    assert g.rate_convert(x[:, :0], 48000, 44100).shape == (2, 0) and _count() == 0
    out = torch.full((2, 930), 5.0, device=DEV)[:, :919]                   # a view with a pitch of its own
    assert g.rate_convert(x, 48000, 44100, out=out) is out and _count() == 1 and float(out.abs().max()) == 0.0
    with pytest.raises(ValueError, match="the plan is one of"):
        g.rate_convert(x, 48000, 32000, plan=plan)
    with pytest.raises(ValueError, match="the table must hold"):
        g.rate_convert(x, 48000, 44100, plan=plan, table=table_dev[:-1])
    with pytest.raises(ValueError, match="out must have the shape"):
        g.rate_convert(x, 48000, 44100, out=torch.zeros((2, 918), device=DEV))
    with pytest.raises(_lib().P2PHDError):
        g.rate_convert(x.cpu(), 48000, 44100)
    with pytest.raises(ValueError, match="504 taps"):
        g.rate_convert(x, 48000, 8000)


# ------------------------------------------------------------------------------------------
# 3. refusals: nothing is launched, nothing is written
# ------------------------------------------------------------------------------------------
def test_refusals():
    L_ = _lib()
    o, n, P = 3, 2, 10
    rng = np.random.default_rng(3)
    table_dev = torch.from_numpy(_int_table(rng, n, P).astype(np.float32)).to(DEV)
    x = rng.integers(-64, 65, (2, 100)).astype(np.float32)
    other = torch.zeros(1000, device=DEV)
    bad = (dict(P=9), dict(P=2), dict(P=258), dict(o=0), dict(n=0), dict(o=2, n=2), dict(o=6, n=4), dict(o=1, n=1), dict(n=1 << 18),
           dict(out_frames=66), dict(out_frames=68), dict(out_ld=66), dict(ld=99), dict(frames=-1), dict(channels=0), dict(channels=65536),
           dict(planar=None), dict(table=None), dict(out=None), dict(planar=L_.C.c_void_p(other.data_ptr() + 2)),
           dict(table=L_.C.c_void_p(other.data_ptr() + 1)), dict(out=L_.C.c_void_p(other.data_ptr() + 3)))
    _count(reset=True)
    for over in bad:
        rc, _, intact = _call(x, table_dev, o, n, 1, over)
        assert rc != 0 and intact and b"rateconv_fwd" in L_.lib().p2phd_last_error(), over
    # an output that overlaps the input
    buf = torch.zeros(400, device=DEV)
    rc = L_.lib().p2phd_rateconv_fwd(L_.ptr(buf), 100, 2, 100, L_.ptr(table_dev), o, n, P, L_.ptr(buf[150:]), 67, 67, L_.stream_ptr())
    assert rc != 0 and b"overlaps" in L_.lib().p2phd_last_error()
    assert _count() == 0
    rc, got, intact = _call(x, table_dev, o, n, 1)
    assert rc == 0 and intact and _count() == 1 and got.shape == (2, 67)
