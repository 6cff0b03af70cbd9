"""Per-row evaluation metrics (p2phd_audio_metrics_rows, csrc/metrics.hip) through the C ABI against the float64 restatement
(tests/_metrics_ref.py).

Tolerances: rtol 1e-4 on every figure and atol 2e-6 on the matched signal, this project's bounds for these quantities
(tests/test_gpu_evaltail.py); a figure that the restatement gives as NaN, -10 or 35 must be exactly that.  One kind of row is
outside the relative bound by construction: sr = 1.7 hr - 0.3, whose moment-matched sr' is hr up to fp32 rounding.  Every
figure that measures sr' - hr there is a rounding residue in fp32 and another one in fp64, so those get the bounds that
test_metrics_identical_signals_and_errors uses for sr == hr (mse < 1e-12, snr_sr > 60 dB, every LSD < 1e-3) and the segmental
SNR of that row must sit at the upper clamp (>= 34.9)."""
import ctypes

import numpy as np
import pytest
import torch

import _metrics_ref as R
from oracle import mdct4 as OM4

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W8, H8 = R.seg_geometry(8000)
CANARY = 12345.678
PAD = 64                                                                      # floats of canary on either side


def _call(hr, lr, sr, n_fft, hop, win, center, cut_bin, W, H):
    """The C entry on float32 numpy rows [B, T]; rows_out and matched_out sit between canaries, the workspace has exactly
    the reported size and a canary behind it.  -> (rows [B, 8] float32, matched [B, T] float32) as numpy."""
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.util import util as U
    L = _lib.lib()
    B, T = hr.shape
    n2, hop2, win2 = 2 * n_fft, 2 * hop, 2 * win
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (hr, lr, sr)]
    window2 = U.kbdwin(win2).to(DEV).contiguous()
    nbytes = L.p2phd_metrics_rows_workspace_bytes(B, T, n2, hop2, win2, int(center), cut_bin, W, H)
    assert nbytes > 0 and nbytes % 8 == 0, L.p2phd_last_error()
    ws = torch.full((nbytes // 4 + PAD,), CANARY, dtype=torch.float32, device=DEV)
    rows = torch.full((PAD + B * 8 + PAD,), CANARY, dtype=torch.float32, device=DEV)
    matched = torch.full((PAD + B * T + PAD,), CANARY, dtype=torch.float32, device=DEV)
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + 4 * off)
    _lib.check(L.p2phd_audio_metrics_rows(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), B, T, n2, hop2, win2, _lib.ptr(window2),
                                          _lib.ptr(U._stft_tables(n2, torch.device(DEV))), int(center), cut_bin, W, H,
                                          at(matched, PAD), at(rows, PAD), _lib.ptr(ws), _lib.stream_ptr()), "audio_metrics_rows")
    rows, matched, tail = rows.cpu().numpy(), matched.cpu().numpy(), ws[nbytes // 4:].cpu().numpy()
    for name, a, n in (("rows_out", rows, B * 8), ("matched_out", matched, B * T)):
        assert np.all(a[:PAD] == np.float32(CANARY)) and np.all(a[PAD + n:] == np.float32(CANARY)), name
    assert np.all(tail == np.float32(CANARY)), "workspace"
    return rows[PAD:PAD + B * 8].reshape(B, 8).copy(), matched[PAD:PAD + B * T].reshape(B, T).copy()


def _check(got, matched, hr, lr, sr, n_fft, hop, win, center, cut_bin, W, H):
    want, want_matched = R.rows(hr, lr, sr, n_fft, hop, win, OM4.kbdwin(2 * win), center, cut_bin, W, H)
    print("\ngot\n", got, "\nwant\n", want)
    np.testing.assert_allclose(matched, want_matched, rtol=0, atol=2e-6)
    F = R.seg_frame_count(hr.shape[1], W, H)
    for b in range(hr.shape[0]):
        residue = bool(np.array_equal(sr[b], np.float32(1.7) * hr[b] - np.float32(0.3)))
        for j, name in enumerate(R.NAMES):
            g, w = float(got[b, j]), float(want[b, j])
            if j >= 6 and F < 1:
                assert np.isnan(w) and np.isnan(g), (b, name, g)
            elif residue and name == "mse":
                assert 0 <= g < 1e-12, (b, name, g)
            elif residue and name == "snr_sr":
                assert g > 60, (b, name, g)
            elif residue and name.startswith("lsd"):
                assert 0 <= g < 1e-3, (b, name, g)
            elif residue and name == "ssnr_sr":
                assert 34.9 <= g <= 35.0, (b, name, g)
            elif w in (-10.0, 35.0) or np.isinf(w):
                assert g == w, (b, name, g, w)
            else:
                np.testing.assert_allclose(g, w, rtol=1e-4, err_msg="row %d %s" % (b, name))
    return want


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft", [32, 64])
@pytest.mark.parametrize("T", [W8 + H8 - 1, W8 + H8, 997, 4096])
def test_rows_match_restatement(T, n_fft, center):
    """8 kHz geometry (W 240, H 60); T = W + H - 1 holds no segment (NaN), W + H exactly one; B = 1 and 3; cut_bin at both ends
    of its range and where 2 kHz -> 8 kHz puts it.  Row b of the 3-row call is the 1-row call on that row, bit for bit."""
    hop, win = n_fft // 2, n_fft
    hr, lr, sr = R.signals(3, T, W8, H8, seed=T + n_fft)
    rate_cut = (2 * n_fft * 2000) // (2 * 8000)
    for cut_bin in (1, rate_cut, n_fft):
        got, matched = _call(hr, lr, sr, n_fft, hop, win, center, cut_bin, W8, H8)
        want = _check(got, matched, hr, lr, sr, n_fft, hop, win, center, cut_bin, W8, H8)
        assert want[1, 7] == 35.0 or T < W8 + H8                              # lr == hr: the upper clamp, exactly
        for b in range(3):
            one, one_matched = _call(hr[b:b + 1], lr[b:b + 1], sr[b:b + 1], n_fft, hop, win, center, cut_bin, W8, H8)
            assert one.tobytes() == got[b:b + 1].tobytes(), (cut_bin, b, one, got[b])
            assert one_matched.tobytes() == matched[b:b + 1].tobytes(), (cut_bin, b)


def test_rows_48k_geometry():
    """W = 1440 (not a multiple of the wavefront), H = 360, T = 5000: 9 segments over 3 workgroups; the silent stretch of row 0
    holds whole segments, which sit at the lower clamp."""
    W, H = R.seg_geometry(48000)
    T, n_fft = 5000, 64
    hr, lr, sr = R.signals(3, T, W, H, seed=48)
    assert (R.ssnr_frames(hr[0], lr[0], W, H) == -10.0).any()
    cut_bin = (2 * n_fft * 8000) // (2 * 48000)
    got, matched = _call(hr, lr, sr, n_fft, n_fft // 2, n_fft, True, cut_bin, W, H)
    _check(got, matched, hr, lr, sr, n_fft, n_fft // 2, n_fft, True, cut_bin, W, H)
    again, _ = _call(hr, lr, sr, n_fft, n_fft // 2, n_fft, True, cut_bin, W, H)
    assert again.tobytes() == got.tobytes()                                   # no atomics: the same bits from run to run


def test_python_entry_and_existing_path():
    """util.audio_metrics_rows is the C entry with the geometry the rates give; the row mean of its first four columns is what
    util.audio_metrics reports; compute_matrics keeps its 7-tuple with the zeros; compute_matrics_ext names the columns."""
    from types import SimpleNamespace
    from pix2pixhdaudiosr_amd.util import util as U
    n_fft, T = 32, 997
    hr, lr, sr = R.signals(3, T, W8, H8, seed=3)
    t = [torch.from_numpy(a).to(DEV) for a in (hr, lr, sr)]
    rows, matched = U.audio_metrics_rows(*t, n_fft, n_fft // 2, n_fft, True, 8000, 2000)
    assert rows.is_cuda and tuple(rows.shape) == (3, 8) and rows.dtype == torch.float32 and tuple(matched.shape) == (3, T)
    want, want_matched = _call(hr, lr, sr, n_fft, n_fft // 2, n_fft, True, 8, W8, H8)
    assert rows.cpu().numpy().tobytes() == want.tobytes() and matched.cpu().numpy().tobytes() == want_matched.tobytes()
    res4, matched4 = U.audio_metrics(*t, n_fft, n_fft // 2, n_fft, True)
    assert torch.equal(matched4, matched)
    np.testing.assert_allclose(want[:, :4].astype(np.float64).mean(0), res4.cpu().numpy(), rtol=1e-4)
    opt = SimpleNamespace(n_fft=n_fft, hop_length=n_fft // 2, win_length=n_fft, center=True, hr_sampling_rate=8000,
                          lr_sampling_rate=2000)
    old = U.compute_matrics(*t, opt)
    assert len(old) == 7 and old[3:6] == (0, 0, 0)
    assert old[:3] + old[6:] == tuple(res4.tolist())
    ext = U.compute_matrics_ext(*t, opt)
    assert len(ext) == 3 and all(tuple(e) == U.METRIC_ROW_NAMES for e in ext)
    assert [[e[k] for k in U.METRIC_ROW_NAMES] for e in ext] == want.astype(np.float64).tolist()
    # a 1-D clip is one row; equal rates put the Nyquist bin alone into the high band
    one = U.compute_matrics_ext(t[0][0], t[1][0], t[2][0], SimpleNamespace(**{**vars(opt), "lr_sampling_rate": 8000}))
    assert len(one) == 1 and one[0]["mse"] == ext[0]["mse"] and one[0]["ssnr_lr"] == ext[0]["ssnr_lr"]
    assert one[0]["lsd_hf"] == float(_call(hr[:1], lr[:1], sr[:1], n_fft, n_fft // 2, n_fft, True, n_fft, W8, H8)[0][0, 5])


def test_launches_do_not_depend_on_rows_and_errors():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.util import util as U
    L = _lib.lib()
    counts = []
    for B in (1, 3):
        hr, lr, sr = (torch.from_numpy(a).to(DEV) for a in R.signals(B, 997, W8, H8, seed=B))
        L.p2phd_launch_count(b"metrics_rows", 1)
        U.audio_metrics_rows(hr, lr, sr, 32, 16, 32, True, 8000, 2000)
        counts.append(L.p2phd_launch_count(b"metrics_rows", 1))
    assert counts[0] == counts[1] > 0
    x = torch.zeros(2, 997, device=DEV)
    with pytest.raises(_lib.P2PHDError, match="cut_bin"):
        U.audio_metrics_rows(x, x, x, 32, 16, 32, True, 8000, 100)            # the low rate's Nyquist frequency below bin 1
    with pytest.raises(_lib.P2PHDError, match="cut_bin"):
        U.audio_metrics_rows(x, x, x, 32, 16, 32, True, 8000, 16000)          # ... above the high rate's
    with pytest.raises(ValueError, match="shapes differ"):
        U.audio_metrics_rows(x, x[:1], x, 32, 16, 32, True, 8000, 2000)
