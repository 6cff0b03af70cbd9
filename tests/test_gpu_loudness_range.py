"""The short-term and the range kernel of csrc/loudness.hip on the GPU against the restatement of tests/_loudness_range_ref.py:
block powers bit for bit on integer hop energies, the selected order statistics bit for bit, the levels to the device's log10,
hand-made powers aimed at each radix pass and each gate, the same bits on every run and stream, the argument errors and the
launch counter."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _loudness_range_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = -7.25
RATE = 8000
# n = 0, 1, 2, 3, 256, 257, 258, 512, 513, 1024 blocks: around the workgroup's width and a histogram's worth of bins
HOPS = (29, 30, 31, 32, 285, 286, 287, 541, 542, 1053)
WEIGHTS = {1: None, 2: (1.0, 0.5), 6: (1.0, 1.0, 1.0, 0.0, 1.41, 1.41)}
LEVEL_TOL = 1e-9                                                   # a cap: the device's log10 is a few ulp of values below 100, 1e-14


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib


def _count(reset=False):
    return _L().lib().p2phd_launch_count(b"loudness", 1 if reset else 0)


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def _same(got, want, tol=LEVEL_TOL):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return abs(got - want) <= tol


def _short_direct(z, rate, weights, gain):
    """p2phd_loudness_short_term into a p with canaries around it -> p (numpy)."""
    L_ = _L()
    C, J = z.shape
    NS = max(J - 29, 0)
    zt = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    buf = torch.full((NS + 16,), CANARY, dtype=torch.float64, device=DEV)
    p = buf[8:8 + NS]
    wbuf = None if weights is None else (ctypes.c_float * C)(*weights)
    g = None if gain is None else torch.tensor([gain, 123.0], dtype=torch.float32, device=DEV)
    L_.check(L_.lib().p2phd_loudness_short_term(L_.ptr(zt), J, C, rate, wbuf, L_.ptr(g), ctypes.c_void_p(p.data_ptr()), L_.stream_ptr()),
             "loudness_short_term")
    host = buf.cpu().numpy()
    assert (host[:8] == CANARY).all() and (host[8 + NS:] == CANARY).all()
    return host[8:8 + NS].copy()


def _range(p, **kw):
    from pix2pixhdaudiosr_amd.generate import loudness_range
    pt = torch.from_numpy(np.array(p, dtype=np.float64)).to(DEV)
    res8 = loudness_range(pt, **kw)
    assert res8.dtype == torch.float64 and res8.shape == (8,)
    assert (pt.cpu().numpy().view(np.uint64) == _bits(p)).all()   # p is read, never written
    return res8.cpu().numpy()


def _check_range(p, what=""):
    """The kernel on p against the restatement: the count and both selected powers bit for bit, the levels within LEVEL_TOL."""
    want = RR.loudness_range(p)
    res8 = _range(p)
    print("%s NS %d: LRA %r (ref %r)  low %r  high %r  threshold %r  n %r (ref %d)  max %r  q %r %r"
          % (what, len(p), res8[0], want['lra'], res8[1], res8[2], res8[3], res8[4], want['n'], res8[5], res8[6], res8[7]))
    assert res8[4] == want['n']
    for k, name in ((6, 'q_lo'), (7, 'q_hi')):
        assert (math.isnan(res8[k]) and math.isnan(want[name])) or _bits(res8[k]) == _bits(want[name]), name
    for k, name in ((0, 'lra'), (1, 'low'), (2, 'high'), (3, 'threshold'), (5, 'short_term_max')):
        assert _same(float(res8[k]), want[name]), (name, res8[k], want[name])
    return res8, want


@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("J", HOPS)
def test_integer_hops_bit_for_bit(J, C):
    """z of integers below 2^20: every 30-term sum is exact, every later step one IEEE operation, so p must be the restatement's
    bits, with and without a gain read from device memory; on those p the selected powers and the count must be too."""
    from pix2pixhdaudiosr_amd.generate import loudness_short_term
    z = RR.integer_hops(C, J)
    for gain in (None, 0.37):
        want = RR.block_powers(z, RATE, WEIGHTS[C], gain)
        _count(reset=True)
        p = _short_direct(z, RATE, WEIGHTS[C], gain)
        assert _count() == (1 if J >= 30 else 0)                   # no block: nothing launched
        assert p.shape == want.shape == (max(J - 29, 0),)
        assert (_bits(p) == _bits(want)).all()
        # the tensor function: the same bits, its own allocation
        g = None if gain is None else torch.tensor([gain], dtype=torch.float32, device=DEV)
        p2 = loudness_short_term(torch.from_numpy(z).to(DEV), RATE, WEIGHTS[C], gain_dev=g)
        assert p2.dtype == torch.float64 and tuple(p2.shape) == p.shape and (_bits(p2.cpu().numpy()) == _bits(p)).all()
        _count(reset=True)
        res8, ref = _check_range(p, "J %d C %d gain %r" % (J, C, gain))
        assert _count() == 1                                       # the range kernel launches for every NS
        assert res8[4] == max(J - 29, 0)                           # every block of this draw is behind both gates
        if J >= 30:
            print("margin %.3g" % ref['margin'])
            assert ref['margin'] > 1e-6                            # ... and far from either threshold: no tie decides
    if J == 30:
        assert res8[0] == 0.0 and res8[6] == res8[7]               # one block: both ranks select it


def test_launch_counter():
    from pix2pixhdaudiosr_amd.generate import loudness_range, loudness_short_term
    for J, want in ((29, 1), (30, 2), (700, 2)):
        z = torch.from_numpy(RR.integer_hops(2, J)).to(DEV)
        _count(reset=True)
        res8 = loudness_range(loudness_short_term(z, RATE))
        assert _count() == want
        if J == 29:
            assert res8.cpu().tolist() == [0.0, float('-inf'), float('-inf'), float('-inf'), 0.0, float('-inf'), 0.0, 0.0]


def test_all_equal_and_ties():
    res8, _ = _check_range(np.full(500, 1e-3), "all equal")
    assert res8[0] == 0.0 and res8[4] == 500 and res8[6] == 1e-3 and res8[7] == 1e-3
    # both ranks inside one run of equal values
    res8, _ = _check_range(np.concatenate([np.full(90, 1e-3), np.full(870, 2e-3), np.full(40, 4e-3)]), "ranks in one run")
    assert res8[0] == 0.0 and res8[6] == 2e-3 and res8[7] == 2e-3
    # each rank inside a run of its own, the runs interleaved in memory
    p = np.concatenate([np.full(300, 1e-3), np.full(400, 2e-3), np.full(300, 4e-3)])
    np.random.default_rng(1).shuffle(p)
    res8, _ = _check_range(p, "ranks in two runs")
    assert res8[6] == 1e-3 and res8[7] == 4e-3 and abs(res8[0] - 10.0 * math.log10(4.0)) <= 1e-9


def test_the_last_pass_decides():
    """Powers that differ in the lowest mantissa bits alone: seven passes see one bin."""
    base = _bits(1e-3) & ~np.uint64(0xFF)
    two = np.concatenate([np.full(100, base), np.full(200, base | np.uint64(1))]).astype(np.uint64).view(np.float64)
    res8, _ = _check_range(two, "lowest bit")
    assert _bits(res8[6]) == base and _bits(res8[7]) == base | np.uint64(1) and res8[0] >= 0.0
    many = (base + np.random.default_rng(2).integers(0, 256, size=3000).astype(np.uint64)).view(np.float64)
    res8, _ = _check_range(many, "lowest byte")
    assert _bits(res8[6]) >> np.uint64(8) == _bits(res8[7]) >> np.uint64(8) and res8[6] < res8[7]


def test_the_first_pass_decides():
    """Powers on both sides of 2^-15, where the top byte of the pattern changes (the exponent field goes from 0x3EF to 0x3F0): the
    ranks part in the first pass.  And powers that differ only in the exponent's top bits, 2^16 apart: the few large ones are
    counted, the ranks lie among the small ones."""
    rng = np.random.default_rng(3)
    p = np.concatenate([2.0 ** -15 * rng.uniform(0.5, 1.0, 400), 2.0 ** -15 * rng.uniform(1.0, 2.0, 600)])
    rng.shuffle(p)
    assert set((_bits(p) >> np.uint64(56)).tolist()) == {0x3E, 0x3F}
    res8, _ = _check_range(p, "across the top byte")
    assert _bits(res8[6]) >> np.uint64(56) == 0x3E and _bits(res8[7]) >> np.uint64(56) == 0x3F
    small = _bits(1.5 * 2.0 ** -17)
    large = small + (np.uint64(16) << np.uint64(52))               # the same mantissa and low exponent bits
    p = np.concatenate([np.full(5000, small), np.full(3, large)]).astype(np.uint64).view(np.float64)
    assert p[-1] == p[0] * 2.0 ** 16
    res8, _ = _check_range(p, "exponent top bits")
    assert res8[4] == 5003 and _bits(res8[6]) == small and _bits(res8[7]) == small and res8[0] == 0.0
    assert _same(float(res8[5]), -0.691 + 10.0 * math.log10(p[-1]))


def test_the_gates():
    ninf = float('-inf')
    # every block under the absolute gate (or on it: equality is out)
    p = np.concatenate([np.full(300, 1e-8), [RR.P_ABS]])
    res8, _ = _check_range(p, "under the absolute gate")
    assert res8[:5].tolist() == [0.0, ninf, ninf, ninf, 0.0] and res8[6] == 0.0 and res8[7] == 0.0
    assert _same(float(res8[5]), -70.0, 1e-9)
    # just over it: in
    res8, _ = _check_range(np.array([RR.P_ABS, np.nextafter(RR.P_ABS, 1.0)]), "over the absolute gate")
    assert res8[4] == 1 and res8[6] == np.nextafter(RR.P_ABS, 1.0)
    # half of the blocks under the relative gate: 30 dB down, over the absolute gate
    p = np.concatenate([np.full(400, 1e-2), np.full(400, 1e-5)])
    np.random.default_rng(4).shuffle(p)
    res8, _ = _check_range(p, "half under the relative gate")
    assert res8[4] == 400 and res8[0] == 0.0 and res8[6] == 1e-2
    # 15 dB down stays in
    res8, _ = _check_range(np.concatenate([np.full(400, 1e-2), np.full(400, 10.0 ** -3.5)]), "over the relative gate")
    assert res8[4] == 800 and abs(res8[0] - 15.0) <= 1e-9


def test_nan_and_inf():
    p = 1e-3 * np.random.default_rng(6).uniform(0.5, 2.0, 700)
    p[333] = float('nan')
    res8, _ = _check_range(p, "one NaN")
    assert all(math.isnan(res8[k]) for k in (0, 1, 2, 6, 7))       # a broken clip shows
    assert res8[4] == 699 and _same(float(res8[5]), -0.691 + 10.0 * math.log10(np.nanmax(p)))     # the maximum is still the fmax
    # +inf is a value like any other: the loudest block, and a mean that nothing is over
    p[333] = float('inf')
    res8, _ = _check_range(p, "one +inf")
    assert res8[5] == float('inf') and res8[4] == 0 and res8[0] == 0.0 and res8[3] == float('inf')


_LONG = {}


def _long():
    """36 000 powers (an hour of blocks) spread over 90 dB around the gates, computed once."""
    if not _LONG:
        rng = np.random.default_rng(7)
        p = 10.0 ** rng.uniform(-9.0, 0.0, 36000)
        p.setflags(write=False)
        _LONG['p'] = p
    return _LONG['p']


def test_an_hour_of_blocks_against_a_sort():
    p = _long()
    res8, want = _check_range(p, "an hour")
    n, over = want['n'], int((p > RR.P_ABS).sum())
    assert 0.3 * len(p) < n < 0.4 * len(p) and 0.7 * len(p) < over < 0.85 * len(p)               # both gates bite
    # the gates keep what is over the higher threshold, the n largest powers: numpy's sort of all of them, counted from the top
    k_lo, k_hi = RR.ranks(n)
    q = np.sort(p)[len(p) - n:]
    assert _bits(res8[6]) == _bits(q[k_lo]) and _bits(res8[7]) == _bits(q[k_hi])


def test_same_bits_twice_and_on_another_stream():
    from pix2pixhdaudiosr_amd.generate import loudness_range, loudness_short_term
    pt = torch.from_numpy(np.array(_long())).to(DEV)
    z = torch.from_numpy(RR.integer_hops(2, 1053)).to(DEV)
    a, b = loudness_range(pt).cpu().numpy(), loudness_range(pt).cpu().numpy()
    pa = loudness_short_term(z, RATE).cpu().numpy()
    out = torch.full((10,), CANARY, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = loudness_range(pt, out=out[1:9])
        pc = loudness_short_term(z, RATE)
    side.synchronize()
    assert c.data_ptr() == out[1:9].data_ptr()
    host = out.cpu().numpy()
    assert host[0] == CANARY and host[9] == CANARY
    assert a.tobytes() == b.tobytes() == host[1:9].tobytes() and pa.tobytes() == pc.cpu().numpy().tobytes()


def test_argument_errors():
    from pix2pixhdaudiosr_amd.generate import loudness_range, loudness_short_term
    L_ = _L()
    lib = L_.lib()
    z = torch.zeros((2, 40), dtype=torch.float64, device=DEV)
    p = torch.zeros((12,), dtype=torch.float64, device=DEV)
    res8 = torch.zeros((9,), dtype=torch.float64, device=DEV)
    g = torch.ones((2,), dtype=torch.float32, device=DEV)
    s = L_.stream_ptr()
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)           # noqa: E731
    _count(reset=True)
    bad_short = [(None, 40, 2, RATE, None, L_.ptr(p)), (L_.ptr(z), 40, 2, RATE, None, None),               # null
                 (off(z, 4), 40, 2, RATE, None, L_.ptr(p)), (L_.ptr(z), 40, 2, RATE, None, off(p, 4)),     # misaligned
                 (L_.ptr(z), 40, 2, RATE, off(g, 2), L_.ptr(p)),
                 (L_.ptr(z), 40, 0, RATE, None, L_.ptr(p)), (L_.ptr(z), 40, 65, RATE, None, L_.ptr(p)),    # channels
                 (L_.ptr(z), -1, 2, RATE, None, L_.ptr(p)),
                 (L_.ptr(z), 40, 2, 44101, None, L_.ptr(p)), (L_.ptr(z), 40, 2, 7990, None, L_.ptr(p))]    # rate
    for zp, J, C, rate, gp, pp in bad_short:
        with pytest.raises(L_.P2PHDError, match="loudness_short_term"):
            L_.check(lib.p2phd_loudness_short_term(zp, J, C, rate, None, gp, pp, s), "short_term")
    for w in ((1.0, float('nan')), (-1.0, 1.0), (float('inf'), 1.0)):
        with pytest.raises(L_.P2PHDError, match="loudness_short_term: weight"):
            loudness_short_term(z, RATE, weights=w)
    for pp, NS, rp in ((None, 11, L_.ptr(res8)), (L_.ptr(p), 11, None), (None, 0, None),                   # null
                       (off(p, 4), 11, L_.ptr(res8)), (L_.ptr(p), 11, off(res8, 4)),                       # misaligned
                       (L_.ptr(p), -1, L_.ptr(res8))):
        with pytest.raises(L_.P2PHDError, match="loudness_range"):
            L_.check(lib.p2phd_loudness_range(pp, NS, rp, s), "range")
    # the tensor functions
    with pytest.raises(ValueError, match="multiple of 10"):
        loudness_short_term(z, 44101)
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_short_term(z.cpu(), RATE)
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_short_term(z, RATE, gain_dev=torch.ones(1))
    with pytest.raises(L_.P2PHDError):
        loudness_short_term(z.float(), RATE)                       # hop energies are float64
    with pytest.raises(L_.P2PHDError):
        loudness_short_term(z, RATE, gain_dev=g.double())          # a gate's gain is float32
    with pytest.raises(ValueError, match="weights for 2 channels"):
        loudness_short_term(z, RATE, weights=(1.0,))
    with pytest.raises(ValueError, match=r"\[C, J\]"):
        loudness_short_term(torch.zeros((65, 40), dtype=torch.float64, device=DEV), RATE)
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_range(p.cpu())
    with pytest.raises(L_.P2PHDError):
        loudness_range(p.float())
    with pytest.raises(ValueError, match=r"\[NS\]"):
        loudness_range(z)
    with pytest.raises(ValueError, match="8 float64"):
        loudness_range(p, out=res8)
    assert _count() == 0                                           # nothing was launched
