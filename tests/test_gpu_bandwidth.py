"""csrc/bandwidth.hip on the GPU: the long-term average spectrum against float64 torch.stft(center=False) within a derived bound,
its bits (a row of a call is the call on that row, a run repeats) and its degenerate cases; the band-edge decision bit for bit
against its numpy restatement (tests/_bandwidth_ref.py) on hand-made float64 spectra; every refusal and the launch counter."""
import math
import os

import numpy as np
import pytest
import torch

import _bandwidth_ref as BR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"bandwidth", 1 if reset else 0)


def _chunk():
    return _lib().lib().p2phd_ltas_chunk_frames()


def _signal(n, start=0):
    """n samples of speech: the golden excerpt, repeated where the clip is longer, with a little noise so that no two repeats agree."""
    x = np.load(os.path.join(GOLDEN, "feeder.npz"))["test_wav_excerpt_i16"].astype(np.float32) / 32768.0
    reps = (start + n + len(x) - 1) // len(x)
    y = torch.from_numpy(np.tile(x, reps)[start:start + n].copy())
    return y + 1e-3 * torch.randn(n, generator=torch.Generator().manual_seed(n + start))


def _offset_rows(x, ld):
    """x [R, L] -> the same values as rows of pitch ld > L that start one float off a 16-byte boundary, NaN between the rows."""
    R_, L = x.shape
    buf = torch.full((R_ * ld + 5,), float('nan'), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    rows = buf[1:1 + R_ * ld].view(R_, ld)[:, :L]
    rows.copy_(x)
    assert rows.data_ptr() % 16 == 4
    return rows


# ------------------------------------------------------------------------------------------
# the long-term average spectrum
# ------------------------------------------------------------------------------------------
# The bound.  tests/test_gpu_specimg.py derives, for the amplitude a = |X| 4 / n_fft of one bin of one frame, |a_gpu - a_ref| <= t with
# t = 16 u log2(n) (4 / n) sqrt(n) max_f ||w x_f||_2 (u = 2^-24; Higham's FFT bound, doubled for the window product and for the two
# frames that share one complex transform, the norm taken as the largest over the row's frames) -- its first term, without the
# log10f one, which this kernel does not have.  The kernel then forms P = a^2 in fp32: a square, a sum of two squares and an exact
# scaling, at most 4 u P relative (3 roundings and the contraction either way).  So per frame |P_gpu - P_ref| <= 2 a_ref t + t^2 +
# 4 u P_ref, and the float64 sum over F frames adds F 2^-53 relative, which disappears in the 4 u.
U = 2.0 ** -24
GEOMETRIES = [(64, 16), (256, 128), (512, 256), (2048, 1024)]


def _ltas_bound(rows64, n_fft, hop):
    P = BR.frame_powers_ref(rows64, n_fft, hop)                                       # [R, F, K]
    norms = BR.frame_norms_ref(rows64, n_fft, hop).max(axis=1)                        # [R]
    t = (16.0 * U * math.log2(n_fft) * (4.0 / n_fft) * math.sqrt(n_fft) * norms)[:, None, None]
    return P.sum(axis=1), (2.0 * np.sqrt(P) * t + t * t + 4.0 * U * P).sum(axis=1)


def _check_ltas(rows_dev, rows_host, n_fft, hop):
    from pix2pixhdaudiosr_amd.generate import ltas
    got = ltas(rows_dev, n_fft, hop)
    R_, L = rows_host.shape
    assert tuple(got.shape) == (R_, n_fft // 2 + 1) and got.dtype == torch.float64
    again = ltas(rows_dev, n_fft, hop)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                # the same bits on every run
    g = got.cpu().numpy()
    assert np.isfinite(g).all() and (g >= 0.0).all()
    ref, tol = _ltas_bound(rows_host.double().numpy(), n_fft, hop)
    err = np.abs(g - ref)
    worst = float((err / tol).max())
    print(f"ltas n_fft {n_fft} hop {hop} R {R_} L {L} F {BR.frames_ref(L, n_fft, hop)}: max |S_gpu - S_ref| / bound = {worst:.4f}")
    assert worst <= 1.0, (n_fft, hop, R_, L, worst, np.unravel_index((err / tol).argmax(), err.shape))
    return got, ref, tol


@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_ltas_is_within_the_bound_of_float64(n_fft, hop):
    from pix2pixhdaudiosr_amd.generate import ltas
    lib, chunk = _lib().lib(), _chunk()
    assert chunk >= 2 and chunk % 2 == 0
    # (19 chunks and a frame: the folding workgroup takes its partials in batches, two full ones and a rest)
    for F in (1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 19 * chunk + 1):
        L = n_fft + (F - 1) * hop + (hop - 1) // 2                 # not a whole number of hops where the hop allows it
        assert lib.p2phd_ltas_frames(L, n_fft, hop) == F == BR.frames_ref(L, n_fft, hop)
        x = torch.stack([(0.9, -0.6, 0.3)[r] * _signal(L, 700 * r) for r in range(3)])
        rows = _offset_rows(x, L + 9)
        _count(reset=True)
        got, _, _ = _check_ltas(rows, x, n_fft, hop)
        assert _count() == 2                                       # one launch a call
        # row r of the 3-row call is the 1-row call, bit for bit -- from a buffer of its own, so neither pitch nor alignment matter
        for r in (0, 2):
            one = ltas(x[r:r + 1].to(DEV), n_fft, hop)
            assert torch.equal(one.view(torch.int64)[0], got.view(torch.int64)[r]), (F, r)


def test_ltas_two_tones_sixty_db_apart():
    """The weaker tone's bin meets the bound, and the bound there is a small fraction of the tone: it is not vacuous."""
    n_fft, hop = 512, 256
    F = _chunk() + 3
    L = n_fft + (F - 1) * hop
    t = torch.arange(L, dtype=torch.float64)
    k1, k2 = 50, 150
    x = (0.5 * torch.sin(2 * torch.pi * k1 * t / n_fft) + 0.5e-3 * torch.sin(2 * torch.pi * k2 * t / n_fft + 0.4)).float()[None]
    got, ref, tol = _check_ltas(_offset_rows(x, L + 7), x, n_fft, hop)
    assert ref[0, k1] == pytest.approx(F * 0.25, rel=1e-3) and ref[0, k2] == pytest.approx(F * 0.25e-6, rel=1e-2)
    assert ref[0].argmax() == k1 and tol[0, k2] < 0.05 * ref[0, k2]
    assert abs(float(got[0, k2]) / ref[0, k2] - 1.0) < 0.05


def test_ltas_short_clip_is_zeros_and_no_launch():
    from pix2pixhdaudiosr_amd.generate import ltas
    L = _lib()
    _count(reset=True)
    for n_fft, n in ((64, 63), (2048, 2047), (256, 0)):
        x = torch.randn((2, n), device=DEV)
        psd = ltas(x, n_fft, n_fft // 2)
        assert tuple(psd.shape) == (2, n_fft // 2 + 1) and (psd.view(torch.int64) == 0).all()
    # written, not left: a buffer of NaN comes back as zeros
    out = torch.full((3, 33), float('nan'), dtype=torch.float64, device=DEV)
    x = torch.randn((3, 50), device=DEV)
    assert L.lib().p2phd_ltas(L.ptr(x), 50, 3, 50, 64, 16, None, L.ptr(out), None, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (out.view(torch.int64) == 0).all() and _count() == 0
    assert L.lib().p2phd_ltas_workspace_bytes(3, 50, 64, 16) == 0
    assert L.lib().p2phd_ltas_workspace_bytes(3, 64 + 16 * 40, 64, 16) == 3 * -(-41 // _chunk()) * 33 * 8      # 41 frames


def test_ltas_refusals():
    from pix2pixhdaudiosr_amd.generate import ltas
    L = _lib()
    lib = L.lib()
    x = torch.zeros((2, 4096), device=DEV)
    out = torch.zeros((2, 2049), dtype=torch.float64, device=DEV)
    tables = torch.zeros((3 * 2048,), device=DEV)
    work = torch.zeros((1 << 20,), dtype=torch.uint8, device=DEV)
    _count(reset=True)

    def call(xp=None, ld=4096, R_=2, n=4096, n_fft=64, hop=16, tp=None, op=None, wp=None):
        return lib.p2phd_ltas(L.ptr(x) if xp is None else xp, ld, R_, n, n_fft, hop, L.ptr(tables) if tp is None else tp,
                              L.ptr(out) if op is None else op, L.ptr(work) if wp is None else wp, L.stream_ptr())
    for kw, word in ((dict(n_fft=1000), b"n_fft"), (dict(n_fft=32), b"n_fft"), (dict(n_fft=4096), b"n_fft"), (dict(n_fft=0), b"n_fft"),
                     (dict(hop=0), b"hop"), (dict(hop=65), b"hop"), (dict(hop=-1), b"hop"), (dict(R_=65536), b"R"), (dict(R_=-1), b"R"),
                     (dict(n=-1), b"L"), (dict(ld=4095), b"row pitch"), (dict(xp=L.ptr(x).value + 2), b"aligned"),
                     (dict(op=L.ptr(out).value + 4), b"8 bytes"), (dict(wp=L.ptr(work).value + 4), b"aligned"),
                     (dict(tp=L.ptr(tables).value + 4), b"aligned"), (dict(op=0), b"psd"), (dict(wp=0), b"null"), (dict(tp=0), b"null"),
                     (dict(xp=0), b"null")):
        assert call(**kw) == -1 and word in lib.p2phd_last_error(), (kw, lib.p2phd_last_error())
    assert lib.p2phd_ltas_frames(4096, 1000, 16) == -1 and b"n_fft" in lib.p2phd_last_error()
    assert lib.p2phd_ltas_frames(4096, 64, 0) == -1 and lib.p2phd_ltas_workspace_bytes(2, 4096, 64, 65) == 0
    assert call(R_=0) == 0                                         # no rows: nothing to do
    with pytest.raises(L.P2PHDError, match="n_fft"):
        ltas(x, 1000, 16)
    with pytest.raises(L.P2PHDError, match="hop"):
        ltas(x, 64, 65)
    with pytest.raises(L.P2PHDError, match="float32"):
        ltas(x.double(), 64, 16)
    torch.cuda.synchronize()
    assert _count() == 0 and float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------
# the decision
# ------------------------------------------------------------------------------------------
def _same_res(got, want):
    """Bit for bit, except that the sign and payload of a NaN are nobody's promise."""
    g, w = got.cpu().numpy(), np.asarray(want)
    assert g.shape == w.shape
    same = (g.view(np.int64) == w.view(np.int64)) | (np.isnan(g) & np.isnan(w))
    assert same.all(), (g.tolist(), w.tolist())


def _spectra(K, Q, G, seed):
    """G groups of Q rows that look like spectra: a band of strong bins, a floor 70 to 90 dB under it, random positive values."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(1e-9, 1e-7, (G * Q, K))
    for g in range(G):
        edge = rng.integers(1, K)
        s[g * Q:(g + 1) * Q, :edge] = rng.uniform(0.1, 2.0, (Q, edge))
        s[g * Q:(g + 1) * Q, edge:min(K, edge + 6)] *= rng.uniform(1.0, 1e5, (Q, min(K, edge + 6) - edge))     # a slope across thr
    return s


@pytest.mark.parametrize("K", [33, 129, 1025])
@pytest.mark.parametrize("M", [1, 7, 8])
def test_decision_is_the_restatement_bit_for_bit(K, M):
    from pix2pixhdaudiosr_amd.generate import bandwidth_detect
    _count(reset=True)
    calls = 0
    for Q in (1, 2, 3):
        s = _spectra(K, Q, 5, 100 * K + 10 * M + Q)
        for db in (60.0, 33.0):
            _same_res(bandwidth_detect(torch.from_numpy(s).to(DEV), Q, M, db), BR.decide_ref(s, Q, M, BR.rel_of(db)))
            calls += 1
    torch.cuda.synchronize()
    assert _count() == calls                                       # one launch a call, whatever G is


def test_decision_edge_cases_bit_for_bit():
    from pix2pixhdaudiosr_amd.generate import bandwidth_detect
    K, M, rel = 33, 8, 1e-6
    cases = []
    t = np.zeros(K)
    t[:8], t[16] = 1.0, 8.0 * 1e-6                                 # band 2 stands at thr exactly (8 * 1e-6 / 8, both exact): it does not pass
    assert 1.0 * rel == 1e-6 and (8.0 * 1e-6) / 8.0 == 1e-6
    cases.append(t.copy())
    t[16] = 1.2e-5                                                 # now its mean is above thr and bin 16 alone is
    cases.append(t.copy())
    last = np.full(K, 1e-9)
    last[:8], last[32] = 1.0, 0.5                                  # the top band is the last band, a partial one of one bin
    cases.append(last)
    cases.append(np.zeros(K))                                      # silence
    cases.append(np.full(K, np.nan))                               # all NaN
    nan = np.full(K, 1e-9)
    nan[:10], nan[20], nan[3] = 1.0, np.nan, np.nan                # a NaN bin makes its band NaN: it neither wins nor passes
    cases.append(nan)
    inf = np.full(K, 1e-9)
    inf[:10], inf[12] = 1.0, np.inf                                # an infinite level: ref and thr infinite, nothing passes
    cases.append(inf)
    neg = np.full(K, 1e-9)
    neg[:10], neg[11] = 1.0, -3.0
    cases.append(neg)
    s = np.stack(cases)
    want = BR.decide_ref(s, 1, M, rel)
    assert want[0][:2].tolist() == [7.0, 0.0] and want[1][:2].tolist() == [16.0, 2.0] and want[2][:2].tolist() == [32.0, 4.0]
    assert want[3].tolist() == [-1.0, -1.0, 0.0, 0.0] and want[4].tolist() == [-1.0, -1.0, 0.0, 0.0] and want[6][:2].tolist() == [-1.0, -1.0]
    assert want[5][:2].tolist() == [9.0, 1.0]
    got = bandwidth_detect(torch.from_numpy(s).to(DEV), 1, M, 60.0)
    _same_res(got, want)
    # 1025 random positive values; a second run; the out= buffer
    r = np.random.default_rng(7).uniform(0.0, 1.0, (4, 1025)) ** 8
    for M_ in (1, 7, 8, 1025):
        got = bandwidth_detect(torch.from_numpy(r).to(DEV), 2, M_, 20.0)
        _same_res(got, BR.decide_ref(r, 2, M_, BR.rel_of(20.0)))
        out = torch.full((8,), float('nan'), dtype=torch.float64, device=DEV)
        assert bandwidth_detect(torch.from_numpy(r).to(DEV), 2, M_, 20.0, out=out).data_ptr() == out.data_ptr()
        assert torch.equal(out.view(2, 4).view(torch.int64), got.view(torch.int64))


def test_decision_refusals_and_the_counter():
    from pix2pixhdaudiosr_amd.generate import bandwidth_detect
    L = _lib()
    lib = L.lib()
    psd = torch.ones((4, 4097), dtype=torch.float64, device=DEV)
    res = torch.zeros((4, 4), dtype=torch.float64, device=DEV)
    _count(reset=True)

    def call(pp=None, G=2, Q=2, K=33, M=8, rel=1e-6, rp=None):
        return lib.p2phd_bandwidth(L.ptr(psd) if pp is None else pp, G, Q, K, M, rel, L.ptr(res) if rp is None else rp, L.stream_ptr())
    for kw, word in ((dict(K=0), b"K"), (dict(K=4098), b"K"), (dict(M=0), b"band_bins"), (dict(M=34), b"band_bins"), (dict(Q=0), b"Q"),
                     (dict(G=-1), b"G"), (dict(G=1 << 31, Q=1), b"G"), (dict(rel=0.0), b"rel"), (dict(rel=1.5), b"rel"), (dict(rel=float('nan')), b"rel"),
                     (dict(rel=-1e-6), b"rel"), (dict(pp=0), b"null"), (dict(rp=0), b"null"), (dict(pp=L.ptr(psd).value + 4), b"aligned"),
                     (dict(rp=L.ptr(res).value + 4), b"aligned")):
        assert call(**kw) == -1 and word in lib.p2phd_last_error(), (kw, lib.p2phd_last_error())
    assert call(G=0) == 0
    torch.cuda.synchronize()
    assert _count() == 0 and float(res.abs().max()) == 0.0
    assert call(K=4097, M=4097, G=1, Q=4) == 0 and call(rel=1.0) == 0
    assert _count() == 2
    with pytest.raises(ValueError, match=r"\[G \* Q, K\]"):
        bandwidth_detect(psd, 3, 8, 60.0)
    with pytest.raises(L.P2PHDError, match="float64"):
        bandwidth_detect(psd.float(), 1, 8, 60.0)
    with pytest.raises(ValueError, match="out must hold"):
        bandwidth_detect(psd, 2, 8, 60.0, out=torch.zeros(4, dtype=torch.float64, device=DEV))


def test_bandwidth_is_the_two_kernels_in_a_row():
    """ops.bandwidth on brick-wall noise: two launches, all channels one group, the restatement's k_top -- on inputs whose nearest
    band level or bin stands at least 0.1 dB from thr, three orders of magnitude more than the fp32 error at -60 dB."""
    from pix2pixhdaudiosr_amd.generate import bandwidth, bandwidth_detect, ltas
    rate = 48000
    for plan, fc, C in ((None, 3400, 1), (dict(n_fft=512, hop=256, band_bins=8, threshold_db=60.0), 8000, 2)):
        p = dict(BR.DEFAULTS, **(plan or {}))
        x = np.stack([BR.brickwall_noise(rate, rate, fc, 5 + c) for c in range(C)]).astype(np.float32)
        hz, want = BR.bandwidth_ref(x, rate, p)
        margin = BR.margin_db(BR.ltas_ref(x, p['n_fft'], p['hop']), C, p['band_bins'], BR.rel_of(p['threshold_db']))
        print(f"bandwidth fc {fc} C {C}: k_top {int(want[0])} ({hz:.1f} Hz), nearest level {margin:.2f} dB from thr")
        assert margin >= 0.1 and 0 <= want[0] - fc * p['n_fft'] / rate <= 8
        dev = torch.from_numpy(x).to(DEV)
        _count(reset=True)
        res = bandwidth(dev, rate, plan)
        assert _count() == 2 and tuple(res.shape) == (4,) and res.dtype == torch.float64
        assert res[:2].tolist() == want[:2].tolist()
        assert float(res[2]) == pytest.approx(want[2], rel=1e-5) and float(res[3]) == float(res[2]) * 1e-6
        assert torch.equal(res, bandwidth_detect(ltas(dev, p['n_fft'], p['hop']), C, p['band_bins'], p['threshold_db'])[0])
    assert bandwidth(torch.zeros((2, 5000), device=DEV), rate).tolist() == [-1.0, -1.0, 0.0, 0.0]      # silence
    assert bandwidth(torch.randn((1, 2047), device=DEV), rate).tolist() == [-1.0, -1.0, 0.0, 0.0]      # shorter than a frame
    with pytest.raises(ValueError, match="rate"):
        bandwidth(torch.zeros((1, 5000), device=DEV), 0)
