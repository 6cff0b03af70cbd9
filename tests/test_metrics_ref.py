"""The float64 restatement of the per-row metrics (tests/_metrics_ref.py) against the oracle and against its own
definitions, and the host-only half of the C ABI (p2phd_metrics_rows_workspace_bytes).  No GPU."""
import numpy as np

import _metrics_ref as R
from oracle import evaltail as E
from oracle import mdct4 as OM4

W, H = R.seg_geometry(8000)


def test_geometry():
    assert (W, H) == (240, 60) and R.seg_geometry(48000) == (1440, 360)
    w = R.seg_window(W)
    assert w.shape == (W,) and np.all(w > 0) and np.allclose(w, w[::-1], rtol=0, atol=1e-15)       # Hann without its zeros


def test_first_four_columns_are_the_oracles():
    n_fft, hop, win = 32, 16, 32
    window2 = OM4.kbdwin(2 * win)
    for center in (True, False):
        hr, lr, sr = R.signals(1, 997, W, H, seed=6)                          # a 1-row input
        got, matched = R.rows(hr, lr, sr, n_fft, hop, win, window2, center, 8, W, H)
        mse, snr_sr, snr_lr, lsd, sr_m = E.compute_metrics(hr, lr, sr, n_fft, hop, win, window2, center)
        assert got.shape == (1, 8)
        np.testing.assert_allclose(got[0, :4], [mse, snr_sr, snr_lr, lsd], rtol=1e-12)
        np.testing.assert_array_equal(matched, sr_m)


def test_band_energies_add_up_per_frame():
    n_fft, hop, win = 32, 16, 32
    hr, _, sr = R.signals(3, 997, W, H, seed=7)
    srm = E.match_moments(sr.astype(np.float64), hr.astype(np.float64))
    n_all = n_fft + 1
    for cut in (1, 8, n_fft):
        d_all, d_lo, d_hi = R.lsd_frames(hr, srm, n_fft, hop, win, OM4.kbdwin(2 * win), True, cut)
        assert d_all.shape == d_lo.shape == d_hi.shape == (3, 1 + 997 // (2 * hop))
        np.testing.assert_allclose(cut * d_lo ** 2 + (n_all - cut) * d_hi ** 2, n_all * d_all ** 2, rtol=1e-12)


def test_segmental_snr_clamps():
    hr, lr, sr = R.signals(3, 997, W, H, seed=8)
    assert np.array_equal(lr[1], hr[1])
    assert R.ssnr(hr[1], lr[1], W, H) == 35.0                                 # En = 0: every frame at the upper clamp
    # row 0 is silent over W + H + 1 samples from T // 4 on: at least one frame lies inside, Es = 0 there
    v = R.ssnr_frames(hr[0], lr[0], W, H)
    start = 997 // 4
    inside = [f for f in range(len(v)) if f * H >= start and f * H + W <= start + W + H + 1]
    assert inside and all(v[f] == -10.0 for f in inside)
    assert np.all(v >= -10.0) and np.all(v <= 35.0) and (v > -10.0).any()
    assert R.ssnr(hr[0], lr[0], W, H) == v.mean()


def test_frame_count():
    g = np.random.default_rng(9)
    for T, want in ((W + H - 1, 0), (W + H, 1), (W + 2 * H + 1, 2)):
        assert R.seg_frame_count(T, W, H) == want == (T - W) // H
        x = g.standard_normal(T)
        v = R.ssnr_frames(x, x + 0.1 * g.standard_normal(T), W, H)
        assert v.shape == (want,)
        assert np.isnan(R.ssnr(x, x + 0.1, W, H)) == (want == 0)
    assert R.seg_frame_count(W - 5, W, H) == 0


def test_workspace_entry_host_only():
    """p2phd_metrics_rows_workspace_bytes is host arithmetic: the argument checks of the per-row entry without a GPU."""
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "p2phd_metrics_rows_workspace_bytes") and hasattr(L, "p2phd_audio_metrics_rows")
    B, T, n2, hop2, win2 = 3, 997, 64, 32, 64
    ok = L.p2phd_metrics_rows_workspace_bytes(B, T, n2, hop2, win2, 1, 8, W, H)
    assert ok > 0 and ok % 8 == 0
    assert L.p2phd_metrics_rows_workspace_bytes(B, T, n2, hop2, win2, 1, 1, W, H) > 0
    assert L.p2phd_metrics_rows_workspace_bytes(B, T, n2, hop2, win2, 0, n2 // 2, W, H) > 0
    for bad, word in (((0, W, H), b"cut_bin"), ((n2 // 2 + 1, W, H), b"cut_bin"), ((8, W, 0), b"hop"), ((8, 0, H), b"window")):
        assert L.p2phd_metrics_rows_workspace_bytes(B, T, n2, hop2, win2, 1, *bad) == 0, bad
        assert word in L.p2phd_last_error(), (bad, L.p2phd_last_error())
    # the checks of the existing entry hold here too
    assert L.p2phd_metrics_rows_workspace_bytes(B, T, 100, hop2, win2, 1, 8, W, H) == 0 and b"power of two" in L.p2phd_last_error()
    # a row shorter than one segment is not refused: its two segmental-SNR slots are NaN, the rest is valid
    assert L.p2phd_metrics_rows_workspace_bytes(B, W - 1, n2, hop2, win2, 1, 8, W, H) > 0
    assert 8 * W < L.p2phd_metrics_rows_workspace_bytes(1, T, n2, hop2, win2, 1, 8, W, H) < ok      # the window table, then per row


def test_python_names_and_geometry():
    from pix2pixhdaudiosr_amd.util import util as U
    assert U.METRIC_ROW_NAMES == R.NAMES
    assert U.metric_rows_geometry(32, 8000, 2000) == (8, 240, 60)
    assert U.metric_rows_geometry(1024, 48000, 8000) == (170, 1440, 360)          # 2048 * 8000 // 96000
    assert U.metric_rows_geometry(64, 48000, 48000) == (64, 1440, 360)         # equal rates: the high band is the Nyquist bin


def test_csv_rows_extended(tmp_path):
    """The --metrics_ext table: four more columns, the mean of a column over its entries that are not NaN; without the flag the
    rows are today's."""
    import csv
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_EXT, _parser, metrics_rows, write_metrics_csv
    assert METRICS_COLUMNS == ("file", "channel", "frames", "mse", "snr_sr", "snr_lr", "lsd")
    assert METRICS_COLUMNS_EXT == METRICS_COLUMNS + ("lsd_lf", "lsd_hf", "ssnr_sr", "ssnr_lr")
    nan = float("nan")
    e = lambda k, s: dict(zip(R.NAMES, (k + 0.0, k + 1.0, k + 2.0, k + 3.0, k + 4.0, k + 5.0, s, s)))
    m = lambda d: (d["mse"], d["snr_sr"], d["snr_lr"], 0, 0, 0, d["lsd"])
    ext = [[e(1, 10.0), e(2, nan)], None, [e(5, 20.0)]]
    records = [{"path": p, "out_frames": n, "metrics": x and [m(d) for d in x], "metrics_ext": x}
               for p, n, x in zip(("a.wav", "bad.wav", "b.wav"), (10, 0, 20), ext)]
    rows = metrics_rows(records, extended=True)
    assert [r[:3] for r in rows] == [("a.wav", 0, 10), ("a.wav", 1, 10), ("b.wav", 0, 20), ("mean", "", "")]
    assert rows[0][3:] == (1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 10.0, 10.0) and rows[1][3:9] == (2.0, 3.0, 4.0, 5.0, 6.0, 7.0)
    assert rows[-1][3:] == (8 / 3, 11 / 3, 14 / 3, 17 / 3, 20 / 3, 23 / 3, 15.0, 15.0)
    only_nan = metrics_rows([records[0] | {"metrics_ext": [e(2, nan)]}], extended=True)
    assert only_nan[-1][9] != only_nan[-1][9] and only_nan[-1][3] == 2.0
    assert metrics_rows([records[1]], extended=True) == []
    plain = metrics_rows(records)
    assert plain[0] == ("a.wav", 0, 10, 1.0, 2.0, 3.0, 4.0) and len(plain[-1]) == 7
    path = str(tmp_path / "m.csv")
    write_metrics_csv(path, records, extended=True)
    with open(path, newline="") as f:
        table = list(csv.reader(f))
    assert tuple(table[0]) == METRICS_COLUMNS_EXT and len(table) == 5 and table[2][9] == "nan" and float(table[-1][9]) == 15.0
    write_metrics_csv(path, records)
    with open(path, newline="") as f:
        assert tuple(next(csv.reader(f))) == METRICS_COLUMNS
    base = ["--input", "a", "--output", "b", "--load_pretrain", "c"]
    assert _parser().parse_args(base).metrics_ext is False and _parser().parse_args(base + ["--metrics_ext"]).metrics_ext is True
