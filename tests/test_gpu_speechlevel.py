"""The active speech level on the GPU (csrc/speechlevel.hip: p2phd_speechlevel_envelope, p2phd_speechlevel_counts,
p2phd_speechlevel_decide; generate.speech_level*): m (between 0xA5 guard bytes), sq and a bit for bit against the chunked
restatement of tests/_speechlevel_ref.py fed the entry's own constants; res within 1e-9 dB / 1e-12 activity and the gain within
2 float32 ulp (the two sides' log10 and pow are different libraries).  Lengths around the chunk, the hangover window and the
workgroup tile at 8 kHz, one case at 48 kHz and the largest halo at 192 kHz; rows with a pitch, a row pointer off 16-byte
alignment; zeros, a NaN and an infinity; the grid option, a side stream, a poisoned workspace; targets, the clamp, the counter and
every refusal."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _speechlevel_ref as R

pytestmark = pytest.mark.gpu


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib


def _G():
    from pix2pixhdaudiosr_amd import generate
    return generate


def _tile():
    return int(_L().lib().p2phd_speechlevel_tile_len())


def _count(reset=False):
    return _L().lib().p2phd_launch_count(b"speechlevel", 1 if reset else 0)


_CONSTS = {}


def _consts(rate):
    if rate not in _CONSTS:
        c, I = _G().speech_level_consts(rate)
        _CONSTS[rate] = (tuple(c[:4].tolist()), I)
    return _CONSTS[rate]


def _noise(C, n, rate, seed):
    return np.stack([R.modulated_noise(n, rate, seed + c, depth_hz=1.3 + 0.7 * c, level=0.1 * (c + 1)) for c in range(C)])


_REF = {}


def _ref(key, clip, rate):
    """The restatement of a clip, computed once per key and shared."""
    if key not in _REF:
        k, I = _consts(rate)
        _REF[key] = R.chunked(clip, k, I)
    return _REF[key]


def _run(clip, rate, pitch=0, offset=0, workspace=None, **decide):
    """clip [C, n] numpy -> (m with its guards [C, n + 5], sq, a, res, gain) as numpy, through the three entries.  `pitch`: extra
    floats between rows; `offset`: floats the first row starts behind a fresh allocation."""
    G = _G()
    C, n = clip.shape
    ld = n + pitch
    buf = torch.full((offset + C * ld + 8,), 7.0, dtype=torch.float32, device="cuda")
    x = buf[offset:offset + C * ld].view(C, ld)[:, :n]
    x.copy_(torch.from_numpy(clip))
    m = torch.full((C, n + 5), 0xA5, dtype=torch.uint8, device="cuda")
    mv, sq = G.speech_level_envelope(x, rate, m=m, **({} if workspace is None else {'workspace': workspace}))
    a = G.speech_level_counts(mv, rate)
    res, gain = G.speech_level_decide(sq, a, n, **decide)
    return m.cpu().numpy(), sq.cpu().numpy(), a.cpu().numpy(), res.cpu().numpy(), gain.cpu().numpy()


def _same(x, y):
    """Bit for bit, a NaN equal to a NaN."""
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and bool(((x == y) | ((x != x) & (y != y))).all())


def _close(got, want, tol):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return abs(got - want) <= tol


def _check(out, ref, n, target=None, max_gain_db=40.0):
    m, sq, a, res, gain = out
    rows, fig, ch = ref
    C = len(rows)
    assert m.shape == (C, n + 5) and (m[:, n:] == 0xA5).all()
    for c, r in enumerate(rows):
        assert (m[c, :n] == r['m']).all(), (c, int(np.argmax(m[c, :n] != r['m'])))
        assert _same(sq[c], r['sq']), (c, sq[c], r['sq'])
        assert a[c, :15].tolist() == r['a'] and a[c, 15] == 0
        assert _close(res[c, 0], r['active'], 1e-9) and _close(res[c, 1], r['long_term'], 1e-9) and _close(res[c, 2], r['activity'], 1e-12)
        assert res[c, 3] == r['bracket']
    assert _close(res[C, 0], fig['active'], 1e-9) and _close(res[C, 1], fig['long_term'], 1e-9) and _close(res[C, 2], fig['activity'], 1e-12)
    assert res[C, 3] == ch
    want = R.gain_of(target, fig['active'], max_gain_db)
    assert abs(int(gain.view(np.int32)[0]) - int(np.array([want]).view(np.int32)[0])) <= 2, (gain, want)


def _lengths():
    T = _tile()
    return [1, 255, 256, 257, 1600, 1601, 1602, T - 1, T, T + 1, T + 1601, 3 * T + 77]


@pytest.mark.parametrize("k", range(12))
def test_lengths_at_8_khz(k):
    """I = 1600, the smallest legal window.  One channel from an aligned allocation (the 16-byte path) with guards behind m."""
    n = _lengths()[k]
    # (the short clips are modulated faster and louder, so that they hold activity and a pause as the long ones do)
    clip = _noise(1, n, 8000, 100 + k) if n > 1602 else R.modulated_noise(n, 8000, 100 + k, depth_hz=20.0, level=0.3)[None]
    _count(reset=True)
    out = _run(clip, 8000, target=-26.0)
    assert _count() == 3
    _check(out, _ref(("len", n), clip, 8000), n, target=-26.0)


def test_three_rows_with_a_pitch_off_alignment_and_option_grid():
    """Three rows, ld = frames + 5, the first row 4 bytes off a 16-byte boundary (the 4-byte path), 3 T + 77 frames: several tiles.
    Then the same clip with speechlevel_grid = 1 (one workgroup walks every tile), twice, and on a side stream: the same bits."""
    T = _tile()
    n = 3 * T + 77
    clip = _noise(3, n, 8000, 7)
    ref = _ref(("rows3", n), clip, 8000)
    first = _run(clip, 8000, pitch=5, offset=1)
    _check(first, ref, n)
    L_ = _L()
    assert L_.lib().p2phd_set_option(b"speechlevel_grid", 1) == 0
    try:
        one = _run(clip, 8000, pitch=5, offset=1)
        # frames + 5 and ld multiples of 4: every row of x on 16 bytes and of m on 4 -- the 16-byte path over three rows, one workgroup
        aligned = _run(clip[:, :n - 2], 8000, pitch=1, offset=0)
    finally:
        assert L_.lib().p2phd_set_option(b"speechlevel_grid", 0) == 0
    assert L_.lib().p2phd_set_option(b"speechlevel_grid", -1) != 0 and L_.lib().p2phd_set_option(b"speechlevel_grid", 16385) != 0
    again = _run(clip, 8000, pitch=5, offset=1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _run(clip, 8000, pitch=5, offset=1)
    side.synchronize()
    for o in (one, again, other):
        assert all(_same(x, y) for x, y in zip(o, first))
    assert (n - 2 + 5) % 4 == 0 and (n - 2 + 1) % 4 == 0
    _check(aligned, _ref(("rows3", n - 2), clip[:, :n - 2], 8000), n - 2)


def test_48_khz_and_the_largest_halo_at_192_khz():
    n = 2 * 9601 + 3
    clip = _noise(1, n, 48000, 21)
    _check(_run(clip, 48000), _ref(("48k", n), clip, 48000), n)
    n = _tile() + 38401
    clip = _noise(1, n, 192000, 22)
    clip[0, :500] = 0.5                                            # activity at the very start: the halo of the second tile holds it
    _check(_run(clip, 192000, offset=1), _ref(("192k", n), clip, 192000), n)


def test_gated_tone_zeros_nan_and_inf():
    rate, n = 8000, 32000
    tone = R.gated_tone(n, rate)[None]
    out = _run(tone, rate, target=-26.0)
    _check(out, _ref("tone", tone, rate), n, target=-26.0)
    assert abs(out[3][0, 0] - (-16.114)) <= 0.01 and abs(out[3][0, 2] - 0.6386) <= 0.001
    zeros = np.zeros((2, 2000), np.float32)
    out = _run(zeros, rate, target=-26.0)
    _check(out, _ref("zeros", zeros, rate), 2000, target=-26.0)
    assert out[4][0] == 1.0 and (out[3][:, 0] == float('-inf')).all() and (out[2] == 0).all()
    # a NaN and an infinity in row 1 of 3: rows 0 and 2 keep their bits
    clip = _noise(3, 20000, rate, 31)
    clean = _run(clip, rate)
    for bad in (np.nan, np.inf):
        broken = clip.copy()
        broken[1, 7777] = bad
        out = _run(broken, rate, target=-26.0)
        _check(out, _ref(("bad", str(bad)), broken, rate), 20000, target=-26.0)
        for c in (0, 2):
            assert (out[0][c] == clean[0][c]).all() and out[1][c] == clean[1][c] and (out[2][c] == clean[2][c]).all()
        assert not math.isfinite(out[1][1]) and not math.isfinite(out[3][1, 0])
    # every channel broken: a non-finite file figure, the gain 1
    out = _run(broken[1:2], rate, target=-26.0)
    assert not math.isfinite(out[3][1, 0]) and out[4][0] == 1.0


def test_poisoned_workspace_of_exactly_the_queried_size():
    n = _tile() + 1601
    clip = _noise(2, n, 8000, 41)
    need = _L().lib().p2phd_speechlevel_workspace_bytes(n, 2)
    assert need == 2 * -(-n // 256) * 24
    outs = []
    for poison in (0xFF, 0x7F):                                    # NaN patterns and huge finite numbers
        work = torch.full((need,), poison, dtype=torch.uint8, device="cuda")
        outs.append(_run(clip, 8000, workspace=work))
    _check(outs[0], _ref(("poison", n), clip, 8000), n)
    assert all(_same(x, y) for x, y in zip(outs[0], outs[1]))
    with pytest.raises(ValueError, match="workspace holds"):
        _run(clip, 8000, workspace=torch.empty((need - 1,), dtype=torch.uint8, device="cuda"))


def test_workspace_holds_the_carries_bit_for_bit():
    """m shows a rounding of q only where q sits within an ulp of a threshold.  The workspace shows every bit: after the call it holds
    (P_k, Q_k, s_k) per chunk, and a product fused into a sum anywhere in steps 1 and 2 of the contract moves their last bits."""
    G = _G()
    for rate, n, C in ((8000, 3 * _tile() + 77, 2), (48000, 2 * 9601 + 3, 1), (192000, 70000, 1)):
        clip = _noise(C, n, rate, 71)
        k, _ = _consts(rate)
        nch = -(-n // 256)
        work = torch.full((_L().lib().p2phd_speechlevel_workspace_bytes(n, C),), 0xFF, dtype=torch.uint8, device="cuda")
        G.speech_level_envelope(torch.from_numpy(clip).cuda(), rate, workspace=work)
        got = work.cpu().numpy().view(np.float64).reshape(C, 3, nch)
        for c in range(C):
            _, _, (P, Q, s) = R.envelope_chunked(clip[c], k, carries=True)
            full = n // 256                                       # (the last, shorter chunk's own (zp, zq) are never used)
            assert (got[c, 0] == P).all() and (got[c, 1] == Q).all() and (got[c, 2] == s).all(), (rate, c)
            assert P[full - 1] > 0 and Q[full - 1] > 0


def test_targets_target_dev_and_the_clamp():
    G = _G()
    rate, n = 8000, 12000
    clip = _noise(2, n, rate, 51)
    rows, fig, ch = _ref("targets", clip, rate)
    x = torch.from_numpy(clip).cuda()
    for target, cap in ((-26.0, None), (fig['active'] + 3.0, None), (fig['active'] + 60.0, None), (fig['active'] - 60.0, None),
                        (fig['active'] + 3.0, 1.0), (fig['active'] - 3.0, 1.0), (fig['active'] + 3.0, 0.0), (None, None), (float('nan'), None)):
        res, gain = G.speech_level(x, rate, target=target, **({} if cap is None else {'max_gain_db': cap}))
        want = R.gain_of(target, fig['active'], 40.0 if cap is None else cap)
        got = gain.cpu().numpy()
        assert abs(int(got.view(np.int32)[0]) - int(np.array([want]).view(np.int32)[0])) <= 2, (target, cap, got, want)
    # a target in device memory: another clip's file figure, and it wins over `target`
    other = torch.from_numpy(0.5 * clip[:1]).cuda()
    res_o, _ = G.speech_level(other, rate)
    res, gain = G.speech_level(x, rate, target=-5.0, target_dev=res_o[1])
    want = R.gain_of(float(res_o[1, 0]), float(res[2, 0]))
    assert abs(int(gain.cpu().numpy().view(np.int32)[0]) - int(np.array([want]).view(np.int32)[0])) <= 2
    assert abs(float(res_o[1, 0]) - (_ref("targets-half", 0.5 * clip[:1], rate)[1]['active'])) <= 1e-9
    # the packed form: res and gain in the caller's bytes
    out = torch.zeros((G.ops.speech_level_packed_bytes(2),), dtype=torch.uint8, device="cuda")
    res2, gain2 = G.speech_level(x, rate, target=-26.0, out=out)
    assert res2.data_ptr() == out.data_ptr() and gain2.data_ptr() == out.data_ptr() + 96
    assert _same(res2.cpu().numpy(), res.cpu().numpy())


def test_counter_and_empty_clip():
    G = _G()
    x = torch.zeros((2, 0), dtype=torch.float32, device="cuda")
    _count(reset=True)
    m, sq = G.speech_level_envelope(x, 8000)
    a = G.speech_level_counts(m, 8000)
    res, gain = G.speech_level_decide(sq, a, 0, target=-26.0)
    assert _count() == 0
    assert (a.cpu().numpy() == 0).all() and float(gain[0]) == 1.0
    assert res.cpu().numpy().tolist() == [[float('-inf'), float('-inf'), 0.0, -1.0]] * 2 + [[float('-inf'), float('-inf'), 0.0, 0.0]]
    y = torch.from_numpy(_noise(1, 300, 8000, 61)).cuda()
    G.speech_level(y, 8000)
    assert _count() == 3


def test_refusals():
    G, L_ = _G(), _L()
    lib = L_.lib()
    x = torch.zeros((2, 1000), dtype=torch.float32, device="cuda")
    m = torch.zeros((2, 1000), dtype=torch.uint8, device="cuda")
    sq = torch.zeros((2,), dtype=torch.float64, device="cuda")
    a = torch.zeros((2, 16), dtype=torch.int64, device="cuda")
    work = torch.zeros((lib.p2phd_speechlevel_workspace_bytes(1000, 2),), dtype=torch.uint8, device="cuda")
    res = torch.zeros((12,), dtype=torch.float64, device="cuda")
    gain = torch.zeros((1,), dtype=torch.float32, device="cuda")
    st = L_.stream_ptr()
    p = L_.ptr

    def env(xp=p(x), frames=1000, C=2, ld=1000, rate=8000, mp=p(m), ld_m=1000, sqp=p(sq), wp=p(work)):
        return lib.p2phd_speechlevel_envelope(xp, frames, C, ld, rate, mp, ld_m, sqp, wp, st)

    def cnt(mp=p(m), frames=1000, C=2, ld_m=1000, rate=8000, ap=p(a)):
        return lib.p2phd_speechlevel_counts(mp, frames, C, ld_m, rate, ap, st)

    def dec(sqp=p(sq), ap=p(a), frames=1000, C=2, target=-26.0, tdev=None, cap=40.0, rp=p(res), gp=p(gain)):
        return lib.p2phd_speechlevel_decide(sqp, ap, frames, C, target, tdev, cap, rp, gp, st)

    _count(reset=True)
    assert env() == 0 and cnt() == 0 and dec() == 0 and _count() == 3
    for call, word in ((lambda: env(frames=-1), b"frames"), (lambda: env(C=0), b"channels"), (lambda: env(C=65), b"channels"),
                       (lambda: env(ld=999), b"ld 999"), (lambda: env(ld_m=999), b"ld_m 999"), (lambda: env(rate=7999), b"rate must be in"),
                       (lambda: env(rate=192001), b"rate must be in"), (lambda: env(xp=None), b"null"), (lambda: env(mp=None), b"null"),
                       (lambda: env(sqp=None), b"null"), (lambda: env(wp=None), b"null"),
                       (lambda: env(xp=ctypes.c_void_p(x.data_ptr() + 2)), b"aligned"), (lambda: env(sqp=ctypes.c_void_p(sq.data_ptr() + 4)), b"aligned"),
                       (lambda: env(wp=ctypes.c_void_p(work.data_ptr() + 4)), b"aligned"),
                       (lambda: cnt(frames=-1), b"frames"), (lambda: cnt(C=0), b"channels"), (lambda: cnt(ld_m=999), b"ld_m 999"),
                       (lambda: cnt(rate=100), b"rate must be in"), (lambda: cnt(ap=None), b"null"), (lambda: cnt(mp=None), b"null"),
                       (lambda: cnt(ap=ctypes.c_void_p(a.data_ptr() + 4)), b"aligned"),
                       (lambda: dec(frames=-1), b"frames"), (lambda: dec(C=65), b"channels"), (lambda: dec(cap=-1.0), b"max_gain_db"),
                       (lambda: dec(cap=float('inf')), b"max_gain_db"), (lambda: dec(cap=float('nan')), b"max_gain_db"),
                       (lambda: dec(rp=None), b"null"), (lambda: dec(gp=None), b"null"), (lambda: dec(sqp=None), b"null"),
                       (lambda: dec(tdev=ctypes.c_void_p(res.data_ptr() + 4)), b"aligned"),
                       (lambda: dec(gp=ctypes.c_void_p(gain.data_ptr() + 2)), b"aligned")):
        assert call() != 0 and word in lib.p2phd_last_error(), (word, lib.p2phd_last_error())
    assert _count() == 3                                          # a refused call launches nothing
    torch.cuda.synchronize()
    # the tensor functions
    with pytest.raises(L_.P2PHDError):
        G.speech_level_envelope(x.cpu(), 8000)
    with pytest.raises(ValueError, match="whole rate in"):
        G.speech_level_envelope(x, 4000)
    with pytest.raises(ValueError, match="at most 64 rows"):
        G.speech_level_envelope(torch.zeros((65, 4), device="cuda"), 8000)
    with pytest.raises(ValueError, match="m must be a uint8 tensor"):
        G.speech_level_envelope(x, 8000, m=torch.zeros((2, 999), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="expected m"):
        G.speech_level_counts(m[0], 8000)
    with pytest.raises(ValueError, match="expected sq"):
        G.speech_level_decide(sq, a[:1], 1000)
    with pytest.raises(ValueError, match="out must hold"):
        G.speech_level_decide(sq, a, 1000, out=torch.zeros((10,), dtype=torch.uint8, device="cuda"))
