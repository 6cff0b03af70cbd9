"""csrc/loudness.hip on the GPU: the hop energies against the sequential float64 restatement (tests/_loudness_ref.py), the same
bits on every run and for every number of rows, the gate kernel on hand-made vectors and on the hop kernel's output, and the
argument errors."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _loudness_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATES = (8000, 16000, 44100, 48000)
CANARY = -7.25
LEVELS = list(R.GATING_LEVELS)


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib


def _count(reset=False):
    return _L().lib().p2phd_launch_count(b"loudness", 1 if reset else 0)


def _frames(hop):
    return (0, 1, hop - 1, hop, 4 * hop, 4 * hop + 1, 7 * hop + 123)


_CLIPS = {}


def _clip(rate):
    """(x [3, 7 hop + 123] float32, z_ref [3, 7]): seeded noise with a DC offset, a stretch 60 dB down behind a loud part and a
    loud burst, and the sequential restatement's hop energies -- computed once per rate, never changed."""
    if rate not in _CLIPS:
        hop = rate // 10
        rng = np.random.default_rng(rate)
        x = 0.1 * rng.standard_normal((3, 7 * hop + 123)) + np.array([[0.05], [-0.02], [0.0]])
        x[:, 2 * hop + 17:4 * hop - 5] *= 1e-3                     # 60 dB down
        x[:, 5 * hop + 11:5 * hop + 11 + hop // 8] *= 8.0          # a burst
        x[2] *= 0.3
        x = x.astype(np.float32)
        assert np.isfinite(x).all()
        z = R.hop_energies(x, rate)
        x.setflags(write=False)
        z.setflags(write=False)
        _CLIPS[rate] = (x, z)
    return _CLIPS[rate]


def _rows_off_boundary(x, frames, C):
    """x[:C, :frames] as rows of a buffer whose first row starts 4 bytes behind a 16-byte boundary, with a pitch of frames + 5
    floats (so the rows start at every alignment) and NaN between the rows."""
    ld = frames + 5
    buf = torch.full((C * ld + 8,), float('nan'), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + C * ld].view(C, ld)
    view[:, :frames] = torch.from_numpy(np.ascontiguousarray(x[:C, :frames])).to(DEV)
    return buf, view, ld


def _hops_direct(view, frames, C, ld, rate, rows_ptr=None):
    """p2phd_loudness_hops into a z with canaries around it -> z [C, J] (numpy), the raw buffer."""
    L_ = _L()
    J = frames // (rate // 10)
    zbuf = torch.full((C * J + 16,), CANARY, dtype=torch.float64, device=DEV)
    z = zbuf[8:8 + C * J]
    ptr = ctypes.c_void_p(view.data_ptr() if rows_ptr is None else rows_ptr)
    L_.check(L_.lib().p2phd_loudness_hops(ptr, frames, C, ld, rate, ctypes.c_void_p(z.data_ptr()), L_.stream_ptr()), "loudness_hops")
    host = zbuf.cpu().numpy()
    assert (host[:8] == CANARY).all() and (host[8 + C * J:] == CANARY).all()
    return host[8:8 + C * J].reshape(C, J).copy()


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("rate", RATES)
def test_hop_energies_match_the_sequential_restatement(rate, C):
    """|z - z_ref| <= 1e-8 z_ref + 1e-12 max z_ref: float64 rounding through a double pole at 0.995 is about 2^-53 / (1 - r)^2 =
    5e-12, the 200 ms warm-up leaves less than that, the printed figure needs 1e-3, and an fp32 recursion (1.5e-2) cannot pass."""
    x, z_ref = _clip(rate)
    hop = rate // 10
    for frames in _frames(hop):
        J = frames // hop
        buf, view, ld = _rows_off_boundary(x, frames, C)
        _count(reset=True)
        z = _hops_direct(view, frames, C, ld, rate)
        assert _count() == (1 if J else 0)                       # J = 0 launches nothing
        want = z_ref[:C, :J]
        assert z.shape == want.shape
        if J:
            err = np.abs(z - want)
            print("rate %d C %d frames %d: max rel err %.3e" % (rate, C, frames, (err / want).max()))
            assert (err <= 1e-8 * want + 1e-12 * want.max()).all()
        # the tensor function: the same bits, its own allocation
        from pix2pixhdaudiosr_amd.generate import loudness_hops
        z2 = loudness_hops(view[:, :frames], rate)
        assert z2.dtype == torch.float64 and tuple(z2.shape) == (C, J) and (z2.cpu().numpy() == z).all()


def test_more_hops_than_one_workgroup_and_a_partly_filled_one():
    """150 hops at 8 kHz: three workgroups of 64 hops per row, the last with 22; against the restatement."""
    rate, hop = 8000, 800
    rng = np.random.default_rng(5)
    x = (0.05 * rng.standard_normal((2, 150 * hop + 37))).astype(np.float32)
    x[:, 70 * hop:90 * hop] *= 1e-3
    want = R.hop_energies(x, rate)
    buf, view, ld = _rows_off_boundary(x, x.shape[1], 2)
    z = _hops_direct(view, x.shape[1], 2, ld, rate)
    assert z.shape == (2, 150) and (np.abs(z - want) <= 1e-8 * want + 1e-12 * want.max()).all()


def test_same_bits_on_two_runs_and_for_any_number_of_rows():
    for rate in (8000, 44100):
        x, _ = _clip(rate)
        frames = x.shape[1]
        buf, view, ld = _rows_off_boundary(x, frames, 3)
        a = _hops_direct(view, frames, 3, ld, rate)
        b = _hops_direct(view, frames, 3, ld, rate)
        assert a.tobytes() == b.tobytes()
        for c in range(3):                                         # the one-row call on row c, in place (its own alignment)
            one = _hops_direct(view, frames, 1, ld, rate, rows_ptr=view.data_ptr() + 4 * c * ld)
            assert one[0].tobytes() == a[c].tobytes(), (rate, c)
        two = _hops_direct(view, frames, 2, ld, rate, rows_ptr=view.data_ptr() + 4 * ld)
        assert two.tobytes() == a[1:].tobytes()


def _gate(z, rate, **kw):
    from pix2pixhdaudiosr_amd.generate import loudness_gate
    zt = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(z))).to(DEV)
    res4, gain = loudness_gate(zt, rate, **kw)
    assert res4.dtype == torch.float64 and res4.shape == (4,) and gain.dtype == torch.float32 and gain.shape == (1,)
    return res4.cpu().numpy(), float(gain.cpu()[0])


def _same_level(got, want):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return abs(got - want) <= 1e-6


def _check_gate(z, rate, weights=None, target=None, max_gain_db=40.0, target_dev=None):
    g = R.gating(z, rate, weights)
    kw = dict(weights=weights, max_gain_db=max_gain_db)
    T = target
    if target_dev is not None:
        kw['target_dev'] = torch.tensor([target_dev, 123.0], dtype=torch.float64, device=DEV)
        T = target_dev
        kw['target'] = -1.0                                        # ignored: the device value wins
    elif target is not None:
        kw['target'] = target
    res4, gain = _gate(z, rate, **kw)
    print("gate: I %r (ref %r)  max %r  gamma %r (ref %r)  kept %r  gain %r" % (res4[0], g['I'], res4[1], res4[2], g['gamma'], res4[3], gain))
    assert _same_level(res4[0], g['I']) and _same_level(res4[1], g['max']) and _same_level(res4[2], g['gamma'])
    assert res4[3] == g['kept']
    # the float64 formula on the level the kernel found, rounded once: within one float32 ulp
    want = np.float32(R.gain(float(res4[0]), T, max_gain_db))
    assert abs(np.float32(gain) - want) <= np.spacing(want), (gain, want)
    return res4, gain


def test_gate_on_the_hand_made_vectors():
    z1 = R.hops_at_level(LEVELS, 4800)[None]
    res4, gain = _check_gate(z1, 48000, target=-23.0)
    assert abs(res4[0] - (-21.5197)) <= 1e-4 and abs(res4[2] - (-33.4741)) <= 1e-4 and res4[3] == 10
    assert gain == pytest.approx(10.0 ** ((-23.0 - res4[0]) / 20.0), rel=1e-6)
    z2 = np.stack([z1[0], R.hops_at_level([-26.0] * len(LEVELS), 4800)])
    res4, _ = _check_gate(z2, 48000, weights=(1.0, 1.41), target_dev=-30.0)
    assert abs(res4[0] - (-21.3514)) <= 1e-4
    # no target: gain 1; another rate: another hop length in the mean square
    res4, gain = _check_gate(z1 * (800.0 / 4800.0), 8000)
    assert gain == 1.0 and abs(res4[0] - (-21.5197)) <= 1e-4
    # the clamp, both ways
    _, gain = _check_gate(z1, 48000, target=-60.0, max_gain_db=6.0)
    assert gain == float(np.float32(10.0 ** (-6.0 / 20.0)))
    _, gain = _check_gate(z1, 48000, target_dev=0.0, max_gain_db=3.0)
    assert gain == float(np.float32(10.0 ** (3.0 / 20.0)))
    _, gain = _check_gate(z1, 48000, target=-60.0, max_gain_db=0.0)
    assert gain == 1.0
    # a target that is not finite on the device: no gain
    _, gain = _check_gate(z1, 48000, target_dev=float('-inf'))
    assert gain == 1.0


def test_gate_edge_cases():
    ninf = float('-inf')
    for J in (0, 1, 3):                                            # fewer than four hops: no block
        _count(reset=True)
        res4, gain = _check_gate(np.full((2, J), 5.0), 48000, target=-23.0)
        assert _count() == 1                                       # the gate always launches: its outputs are valid after every call
        assert tuple(res4) == (ninf, ninf, ninf, 0.0) and gain == 1.0
    res4, gain = _check_gate(np.full((1, 4), 4800.0 * 10.0 ** ((-23.0 + 0.691) / 10.0)), 48000, target=-20.0)
    assert abs(res4[0] - (-23.0)) <= 1e-9 and res4[3] == 1.0       # J = 4: one block
    res4, gain = _check_gate(np.zeros((3, 40)), 48000, target=-23.0)
    assert tuple(res4) == (ninf, ninf, ninf, 0.0) and gain == 1.0  # silence
    res4, gain = _check_gate(R.hops_at_level([-75.0] * 9, 4800)[None], 48000, target=-23.0)
    assert res4[0] == ninf and abs(res4[1] - (-75.0)) <= 1e-6 and res4[2] == ninf and res4[3] == 0.0 and gain == 1.0
    z = R.hops_at_level([-30.0] * 600, 4800)[None].copy()          # more blocks than the workgroup has threads
    z[0, 300:400] *= 0.5
    _check_gate(z, 48000, target=-23.0)
    z[0, 17] = float('nan')
    res4, gain = _check_gate(z, 48000, target=-23.0)
    assert math.isnan(res4[0]) and gain == 1.0


def test_hops_then_gate_on_a_clip_and_a_nan_sample():
    from pix2pixhdaudiosr_amd.generate import loudness
    rate = 16000
    x, z_ref = _clip(rate)
    for C, weights in ((1, None), (3, (1.0, 0.5, 1.41))):
        xt = torch.from_numpy(np.ascontiguousarray(x[:C])).to(DEV)
        g = R.gating(z_ref[:C], rate, weights)
        _count(reset=True)
        res4, gain = loudness(xt, rate, weights, target=-23.0)
        assert _count() == 2
        res4 = res4.cpu().numpy()
        assert _same_level(res4[0], g['I']) and _same_level(res4[1], g['max']) and _same_level(res4[2], g['gamma']) and res4[3] == g['kept']
        assert abs(np.float32(gain.cpu()[0]) - np.float32(R.gain(float(res4[0]), -23.0, 40.0))) <= np.spacing(np.float32(R.gain(float(res4[0]), -23.0, 40.0)))
    bad = torch.from_numpy(x[:1].copy()).to(DEV)
    bad[0, 3 * (rate // 10) + 5] = float('nan')
    res4, gain = loudness(bad, rate, target=-23.0)
    assert not math.isfinite(float(res4.cpu()[0])) and float(gain.cpu()[0]) == 1.0


def test_argument_errors():
    from pix2pixhdaudiosr_amd.generate import loudness_gate, loudness_hops
    L_ = _L()
    x = torch.zeros((2, 9000), dtype=torch.float32, device=DEV)
    z = torch.zeros((2, 10), dtype=torch.float64, device=DEV)
    _count(reset=True)
    for rate in (44101, 7990, 0):
        with pytest.raises(ValueError, match="multiple of 10"):
            loudness_hops(x, rate)
        with pytest.raises(ValueError, match="multiple of 10"):
            loudness_gate(z, rate)
        with pytest.raises(L_.P2PHDError, match="multiple of 10"):
            L_.check(L_.lib().p2phd_loudness_hops(L_.ptr(x), 9000, 2, 9000, rate, L_.ptr(z), L_.stream_ptr()), "loudness_hops")
        out = torch.zeros((5,), dtype=torch.float64, device=DEV)
        with pytest.raises(L_.P2PHDError, match="multiple of 10"):
            L_.check(L_.lib().p2phd_loudness_gate(L_.ptr(z), 10, 2, rate, None, -23.0, None, 40.0, L_.ptr(out), L_.ptr(out[4:]), L_.stream_ptr()), "gate")
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_hops(x.cpu(), 48000)
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_gate(z.cpu(), 48000)
    with pytest.raises(L_.P2PHDError, match="on the GPU"):
        loudness_gate(z, 48000, target_dev=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(L_.P2PHDError):
        loudness_gate(z.float(), 48000)                            # hop energies are float64
    for weights in ((1.0,), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError, match="weights for 2 channels"):
            loudness_gate(z, 48000, weights=weights)
    with pytest.raises(L_.P2PHDError, match="weight 1"):
        loudness_gate(z, 48000, weights=(1.0, float('nan')))
    with pytest.raises(L_.P2PHDError, match="max_gain_db"):
        loudness_gate(z, 48000, max_gain_db=-1.0)
    with pytest.raises(L_.P2PHDError, match="ld 8999"):           # the shared layout check of the PCM entries
        L_.check(L_.lib().p2phd_loudness_hops(L_.ptr(x), 9000, 2, 8999, 48000, L_.ptr(z), L_.stream_ptr()), "loudness_hops")
    with pytest.raises(ValueError, match=r"\[C, J\]"):
        loudness_gate(torch.zeros((65, 4), dtype=torch.float64, device=DEV), 48000)
    assert _count() == 0                                           # nothing was launched
