"""The two album kernels of csrc/loudness.hip on the GPU: loudness_blocks bit for bit on integer hop energies and inside its slice
of a larger buffer; loudness_gate_blocks bit for bit against loudness_gate on one file's blocks, against the restatement of
tests/_loudness_album_ref.py on albums; the same bits on every run and stream, the packed form, the argument errors and the launch
counter."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _loudness_album_ref as AR
import _loudness_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATE = 48000
CANARY = -7.25
WEIGHTS = {1: (1.0,), 2: (1.0, 1.0), 6: (1.0, 1.0, 1.0, 1.41, 1.41, 1.0)}
RANDOM_SEED = 10                                                  # of twelve tried on the restatement, the one farthest from both thresholds


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib


def _count(reset=False):
    return _L().lib().p2phd_launch_count(b"loudness", 1 if reset else 0)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_level(got, want):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return abs(got - want) <= 1e-6


@pytest.mark.parametrize("C", [1, 2, 6])
@pytest.mark.parametrize("J", [0, 1, 3, 4, 5, 67, 259, 260])
def test_blocks_bit_for_bit_inside_their_slice(J, C):
    """Integer hop energies below 2^20: the four-term sum is exact and every later step one IEEE operation, so the power has one bit
    pattern -- R.gating's 'p' is the kernel's expression in the kernel's order."""
    from pix2pixhdaudiosr_amd.generate import loudness_blocks
    z = np.random.default_rng(100 * J + C).integers(1, 1 << 20, size=(C, J)).astype(np.float64)
    want = R.gating(z, RATE, WEIGHTS[C])['p']
    NB = max(J - 3, 0)
    assert want.shape == (NB,)
    buf = torch.full((NB + 16,), CANARY, dtype=torch.float64, device=DEV)
    _count(reset=True)
    p = loudness_blocks(_dev(z), RATE, WEIGHTS[C], out=buf[8:8 + NB])
    assert _count() == (1 if J >= 4 else 0)                        # fewer than four hops: no block, no launch
    assert p.data_ptr() == buf[8:8 + NB].data_ptr() and p.shape == (NB,)
    host = buf.cpu().numpy()
    assert (host[:8] == CANARY).all() and (host[8 + NB:] == CANARY).all()
    assert (_bits(host[8:8 + NB]) == _bits(want)).all()
    # without `out`: a tensor of its own with the same bits
    q = loudness_blocks(_dev(z), RATE, WEIGHTS[C])
    assert q.shape == (NB,) and q.dtype == torch.float64 and (_bits(q.cpu().numpy()) == _bits(want)).all()


def _file(NB, seed, channels=2):
    """Hop energies of a file of NB blocks: levels between -60 and -15 LUFS, so both gates have something to do."""
    levels = np.random.default_rng(seed).uniform(-60.0, -15.0, size=(channels, NB + 3))
    return R.hops_at_level(levels, RATE // 10)


@pytest.mark.parametrize("NB", [1, 255, 256, 257, 1000])
def test_gate_blocks_on_one_file_is_the_gate_bit_for_bit(NB):
    from pix2pixhdaudiosr_amd.generate import loudness_blocks, loudness_gate, loudness_gate_blocks
    z = _file(NB, NB)
    bad = z.copy()
    bad[1, min(5, NB + 2)] = float('nan')
    weights = (1.0, 1.41)
    target_dev = torch.tensor([-30.0, 123.0], dtype=torch.float64, device=DEV)
    for zz in (z, bad):
        zt = _dev(zz)
        p = loudness_blocks(zt, RATE, weights)
        assert p.shape == (NB,)
        for kw in ({}, {'target': -23.0}, {'target': -23.0, 'max_gain_db': 3.0}, {'target_dev': target_dev, 'target': -1.0}):
            want4, want_gain = loudness_gate(zt, RATE, weights, **kw)
            res4, gain = loudness_gate_blocks(p, **kw)
            assert res4.dtype == torch.float64 and res4.shape == (4,) and gain.dtype == torch.float32 and gain.shape == (1,)
            a, b = res4.cpu().numpy(), want4.cpu().numpy()
            print("NB %d %s: %r  gain %r" % (NB, sorted(kw), a, float(gain.cpu()[0])))
            assert (_bits(a) == _bits(b)).all()
            assert gain.cpu().numpy().view(np.uint32)[0] == want_gain.cpu().numpy().view(np.uint32)[0]
            if zz is bad:
                assert math.isnan(a[0]) and float(gain.cpu()[0]) == 1.0     # a NaN block passes both gates
            elif 'target' not in kw and 'target_dev' not in kw:
                assert float(gain.cpu()[0]) == 1.0
    # the restatement agrees with both
    g = R.gating(z, RATE, weights)
    res4 = loudness_gate_blocks(loudness_blocks(_dev(z), RATE, weights))[0].cpu().numpy()
    assert _same_level(res4[0], g['I']) and _same_level(res4[1], g['max']) and _same_level(res4[2], g['gamma']) and res4[3] == g['kept']


def test_gate_blocks_without_a_block():
    from pix2pixhdaudiosr_amd.generate import loudness_gate_blocks
    ninf = float('-inf')
    _count(reset=True)
    res4, gain = loudness_gate_blocks(torch.empty((0,), dtype=torch.float64, device=DEV), target=-23.0)
    assert _count() == 1                                           # it always launches: its outputs are valid after every call
    assert tuple(res4.cpu().numpy()) == (ninf, ninf, ninf, 0.0) and float(gain.cpu()[0]) == 1.0


def _check_album(p, target=-23.0, max_gain_db=40.0):
    from pix2pixhdaudiosr_amd.generate import loudness_gate_blocks
    g = AR.album_gating(p)
    # the precondition, on the restatement: no block within 1e-3 LU of a threshold, so `kept` does not hang on a rounding
    margin = min(np.abs(g['l'] + 70.0).min(), np.abs(g['l'] - g['gamma']).min())
    assert margin > 1e-3, margin
    res4, gain = loudness_gate_blocks(_dev(p), target=target, max_gain_db=max_gain_db)
    res4, gain = res4.cpu().numpy(), np.float32(gain.cpu()[0])
    print("album of %d blocks: I %r (ref %r)  max %r  gamma %r (ref %r)  kept %r (ref %d)  gain %r  margin %.2e"
          % (p.size, res4[0], g['I'], res4[1], res4[2], g['gamma'], res4[3], g['kept'], gain, margin))
    assert _same_level(res4[0], g['I']) and _same_level(res4[1], g['max']) and _same_level(res4[2], g['gamma'])
    assert res4[3] == g['kept']
    want = np.float32(R.gain(float(res4[0]), target, max_gain_db))
    assert abs(gain - want) <= np.spacing(want), (gain, want)
    return res4, g


def test_gate_blocks_on_the_hand_made_album():
    """The album of tests/test_loudness_album_host.py: every file's blocks through loudness_blocks into its slice of one buffer."""
    from pix2pixhdaudiosr_amd.generate import loudness_blocks
    zs = AR.hand_made_album()
    weights = [(1.0,) * z.shape[0] for z in zs]
    want = AR.album_blocks(zs, RATE, weights)
    buf = torch.full((want.size + 2,), CANARY, dtype=torch.float64, device=DEV)
    at = 1
    _count(reset=True)
    for z, w, n in zip(zs, weights, AR.ALBUM_BLOCKS):
        loudness_blocks(_dev(z), RATE, w, out=buf[at:at + n])
        at += n
    assert _count() == 4 and at == want.size + 1                   # the file under 400 ms launches nothing
    host = buf.cpu().numpy()
    assert host[0] == CANARY and host[-1] == CANARY
    np.testing.assert_allclose(host[1:-1], want, rtol=1e-15, atol=0.0)
    res4, _ = _check_album(host[1:-1].copy())
    assert abs(res4[0] - (-20.2108)) <= 1e-4 and abs(res4[2] - (-32.2080)) <= 1e-4 and res4[3] == 46


def _random_album():
    levels = np.random.default_rng(RANDOM_SEED).uniform(-90.0, -10.0, 36000)
    return 10.0 ** ((levels + 0.691) / 10.0)


def test_gate_blocks_on_a_large_random_album():
    res4, g = _check_album(_random_album(), target=-14.0, max_gain_db=2.0)
    assert 9000 < g['kept'] < 10000 and res4[0] > -18.0


def test_same_bits_twice_on_another_stream_and_packed():
    from pix2pixhdaudiosr_amd.generate import loudness_blocks, loudness_gate_blocks
    pt = _dev(_random_album())
    z = _dev(np.random.default_rng(3).integers(1, 1 << 20, size=(2, 1053)).astype(np.float64))
    a4, ag = loudness_gate_blocks(pt, target=-23.0)
    b4, bg = loudness_gate_blocks(pt, target=-23.0)
    pa = loudness_blocks(z, RATE)
    # the packed form: res4, gain and four spare bytes in the middle of a canary buffer
    out = torch.full((56,), 0x5A, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c4, cg = loudness_gate_blocks(pt, target=-23.0, out=out[8:48])
        pc = loudness_blocks(z, RATE)
    side.synchronize()
    assert c4.data_ptr() == out.data_ptr() + 8 and cg.data_ptr() == out.data_ptr() + 40
    host = out.cpu().numpy()
    assert (host[:8] == 0x5A).all() and (host[44:] == 0x5A).all()
    for r4, rg in ((b4, bg), (c4, cg)):
        assert (_bits(r4.cpu().numpy()) == _bits(a4.cpu().numpy())).all()
        assert rg.cpu().numpy().view(np.uint32)[0] == ag.cpu().numpy().view(np.uint32)[0]
    assert (_bits(pa.cpu().numpy()) == _bits(pc.cpu().numpy())).all()
    assert (_bits(pt.cpu().numpy()) == _bits(_random_album())).all()           # p is only read


def test_argument_errors_and_launch_counts():
    from pix2pixhdaudiosr_amd.generate import loudness_blocks, loudness_gate_blocks
    L_ = _L()
    z = torch.zeros((2, 10), dtype=torch.float64, device=DEV)
    p = torch.zeros((8,), dtype=torch.float64, device=DEV)
    out = torch.zeros((5,), dtype=torch.float64, device=DEV)
    s = L_.stream_ptr()
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)           # noqa: E731
    _count(reset=True)
    for rate in (44101, 7990, 0):
        with pytest.raises(ValueError, match="multiple of 10"):
            loudness_blocks(z, rate)
        with pytest.raises(L_.P2PHDError, match="multiple of 10"):
            L_.check(L_.lib().p2phd_loudness_blocks(L_.ptr(z), 10, 2, rate, None, L_.ptr(p), s), "loudness_blocks")
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_blocks(z.cpu(), RATE)
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_blocks(z, RATE, out=p[:7].cpu())
    with pytest.raises(L_.P2PHDError):
        loudness_blocks(z.float(), RATE)                           # hop energies are float64
    with pytest.raises(ValueError, match=r"\[C, J\]"):
        loudness_blocks(torch.zeros((65, 4), dtype=torch.float64, device=DEV), RATE)
    for weights in ((1.0,), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="weights for 2 channels"):
            loudness_blocks(z, RATE, weights=weights)
    with pytest.raises(L_.P2PHDError, match="weight 1"):
        loudness_blocks(z, RATE, weights=(1.0, float('nan')))
    for bad in (p, p[:6], torch.zeros((14,), dtype=torch.float64, device=DEV)[::2], torch.zeros((7, 1), dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError, match="out must be a contiguous float64 tensor of 7 elements"):
            loudness_blocks(z, RATE, out=bad)
    bad_blocks = [(None, 10, 2, RATE, None, L_.ptr(p)), (L_.ptr(z), 10, 2, RATE, None, None),          # null
                  (off(z, 4), 10, 2, RATE, None, L_.ptr(p)), (L_.ptr(z), 10, 2, RATE, None, off(p, 4)),  # not aligned
                  (L_.ptr(z), -1, 2, RATE, None, L_.ptr(p)), (L_.ptr(z), 10, 0, RATE, None, L_.ptr(p)), (L_.ptr(z), 10, 65, RATE, None, L_.ptr(p))]
    for args in bad_blocks:
        with pytest.raises(L_.P2PHDError):
            L_.check(L_.lib().p2phd_loudness_blocks(*(args + (s,))), "loudness_blocks")
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_gate_blocks(p.cpu())
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_gate_blocks(p, target_dev=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(L_.P2PHDError):
        loudness_gate_blocks(p.float())
    with pytest.raises(ValueError, match=r"\[NB\]"):
        loudness_gate_blocks(z)
    with pytest.raises(ValueError, match="target_dev is empty"):
        loudness_gate_blocks(p, target_dev=torch.zeros(0, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="40 bytes"):
        loudness_gate_blocks(p, out=torch.zeros((36,), dtype=torch.uint8, device=DEV))
    with pytest.raises(L_.P2PHDError, match="max_gain_db"):
        loudness_gate_blocks(p, max_gain_db=-1.0)
    with pytest.raises(L_.P2PHDError, match="max_gain_db"):
        loudness_gate_blocks(p, max_gain_db=float('inf'))
    nan = float('nan')
    bad_gate = [(None, 8, nan, None, 40.0, L_.ptr(out), L_.ptr(out[4:])), (L_.ptr(p), 8, nan, None, 40.0, None, L_.ptr(out[4:])),
                (L_.ptr(p), 8, nan, None, 40.0, L_.ptr(out), None), (L_.ptr(p), -1, nan, None, 40.0, L_.ptr(out), L_.ptr(out[4:])),
                (off(p, 4), 7, nan, None, 40.0, L_.ptr(out), L_.ptr(out[4:])), (L_.ptr(p), 8, nan, off(p, 4), 40.0, L_.ptr(out), L_.ptr(out[4:])),
                (L_.ptr(p), 8, nan, None, 40.0, off(out, 4), L_.ptr(out[4:])), (L_.ptr(p), 8, nan, None, 40.0, L_.ptr(out), off(out, 34))]
    for args in bad_gate:
        with pytest.raises(L_.P2PHDError):
            L_.check(L_.lib().p2phd_loudness_gate_blocks(*(args + (s,))), "loudness_gate_blocks")
    assert _count() == 0                                           # nothing was launched
    loudness_blocks(z, RATE)
    assert _count() == 1
    loudness_gate_blocks(p)
    assert _count() == 2
    loudness_blocks(z[:, :3].contiguous(), RATE)
    assert _count() == 2
