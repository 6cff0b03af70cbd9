"""CPU checks of tests/_transform_ref.py: the direct float64 references against the FFT oracles, the conditions of the
operands, the measured constants K, and planted defects that the per-element comparison catches where `rel_err < 1e-4`
under a KBD window does not."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import mdct2 as O2
from oracle import mdct4 as O4
from oracle import model as OM

import _transform_ref as R
from _exact import U32

PIN = 1e-12


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


GEOMS = [(64, 32, 64, True, (3, 200)), (64, 16, 64, True, (2, 171)), (64, 24, 48, True, (2, 190)), (64, 32, 64, False, (2, 203)),
         (128, 64, 128, True, (5, 300)), (16, 8, 16, True, (2, 50))]


# ----------------------------------------------------------------------------------------------------------------------
# 1. the helper against the oracles
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,win,center,shape", GEOMS)
def test_mdct4_direct_equals_fft_oracle(n_fft, hop, win, center, shape):
    B, T = shape
    x = R.signal(shape, 11)
    w = R.window("ramp", win)
    sp, F = R.forward_layout(B, T, hop, win, center)
    assert (sp, F) == (O4.frame_layout(shape, hop, win, center)[0], O4.frame_layout(shape, hop, win, center)[2])
    ref = R.mdct4_ref(x, w, n_fft, hop, win, sp, F)
    fft = O4.mdct4_forward(x.astype(np.float64), n_fft, hop, win, w.astype(np.float64), center)
    assert ref.out.shape == fft.shape                                    # frame count incl. the len(signal) quirk
    assert _rel(ref.out, fft) <= PIN
    assert _rel(ref.out, O4.mdct4_direct(x, n_fft, hop, win, w, center)) <= PIN
    assert ref.frames.shape == (B, F, n_fft) and ref.norms.shape == (B, F)
    assert np.allclose(ref.norms, np.sqrt((fft ** 2).sum(-1)), rtol=1e-12)
    # inverse, with and without out_length
    S = R.signal((B, F, n_fft // 2), 12)
    for ol in (None, T - 7):
        crop, out_len = R.inverse_layout(F, hop, win, center, ol)
        inv = R.imdct4_ref(S, w, n_fft, hop, win, crop, out_len, 4.0 / n_fft)
        fft_inv = O4.imdct4_forward(S.astype(np.float64), n_fft, hop, win, w.astype(np.float64), center, ol).reshape(B, -1)
        assert inv.out.shape == fft_inv.shape
        assert _rel(inv.out, fft_inv) <= PIN
        assert inv.covered.all() and (inv.tol1 > 0).all()
    # the adjoints as the autograd functions lay them out (models/mdct.py _MDCT4Fn / _IMDCT4Fn)
    g = R.signal((B, F, n_fft // 2), 13)
    gx = R.imdct4_ref(g, w, n_fft, hop, win, sp, T, 1.0)
    assert _rel(gx.out, O4.mdct4_backward(g, shape, n_fft, hop, win, w, center)) <= PIN
    crop, out_len = R.inverse_layout(F, hop, win, center)
    ga = R.signal((B, out_len), 14)
    gs = R.mdct4_ref(ga, w, n_fft, hop, win, crop, F, 4.0 / n_fft)
    assert _rel(gs.out, O4.imdct4_backward(ga, F, n_fft, hop, win, w, center)) <= PIN
    # <A x, y> = <x, A^T y> for both pairs, in float64
    lhs, rhs = float((ref.out * g).sum()), float((x.astype(np.float64) * gx.out).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    inv = R.imdct4_ref(S, w, n_fft, hop, win, crop, out_len, 4.0 / n_fft)
    S2 = R.mdct4_ref(ga, w, n_fft, hop, win, crop, F, 4.0 / n_fft)
    lhs, rhs = float((inv.out * ga).sum()), float((S.astype(np.float64) * S2.out).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


@pytest.mark.parametrize("n_fft,hop,win,center,shape", GEOMS)
def test_mdct2_direct_equals_fft_oracle(n_fft, hop, win, center, shape):
    B, T = shape
    x = R.signal(shape, 21)
    w = R.window("ramp", win)
    sp, F = R.forward_layout(B, T, hop, win, center)
    ref = R.mdct2_ref(x, w, n_fft, hop, win, sp, F)
    fft = O2.mdct2_forward(x.astype(np.float64), n_fft, hop, win, w.astype(np.float64), center)
    assert ref.out.shape == fft.shape and _rel(ref.out, fft) <= PIN
    u = R.signal((4, n_fft), 22)
    assert _rel(R.dct2_rows(u), O2.dct_2n(u)) <= PIN
    assert _rel(R.dct3_rows(u), O2.idct_2n(u)) <= PIN
    assert _rel(R.dct3_rows(R.dct2_rows(u)), 2.0 * u) <= PIN             # idct(dct(a)) = 2 a
    S = R.signal((B, F, n_fft), 23)
    for ol in (None, T - 7):
        crop, out_len = R.inverse_layout(F, hop, win, center, ol)
        inv = R.imdct2_ref(S, w, n_fft, hop, win, crop, out_len, 0.5)
        fft_inv = O2.imdct2_forward(S.astype(np.float64), n_fft, hop, win, w.astype(np.float64), center, ol).reshape(B, -1)
        assert inv.out.shape == fft_inv.shape and _rel(inv.out, fft_inv) <= PIN
    # the adjoint pairs with the scale / k0_scale that models/mdct.py passes: _MDCT2Fn.backward = inverse kernel with
    # (scale / N, 2 k0); _IMDCT2Fn.backward = forward kernel with (scale N, k0 / 2)
    g = R.signal((B, F, n_fft), 24)
    for scale, k0 in ((1.0, 1.0), (0.5 * n_fft, 0.5)):
        A = R.mdct2_ref(x, w, n_fft, hop, win, sp, F, scale, k0)
        At = R.imdct2_ref(g, w, n_fft, hop, win, sp, T, scale / n_fft, 2.0 * k0)
        lhs, rhs = float((A.out * g).sum()), float((x.astype(np.float64) * At.out).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    crop, out_len = R.inverse_layout(F, hop, win, center)
    ga = R.signal((B, out_len), 25)
    for scale, k0 in ((0.5, 1.0), (1.0 / n_fft, 2.0)):
        A = R.imdct2_ref(S, w, n_fft, hop, win, crop, out_len, scale, k0)
        At = R.mdct2_ref(ga, w, n_fft, hop, win, crop, F, scale * n_fft, 0.5 * k0)
        lhs, rhs = float((A.out * ga).sum()), float((S.astype(np.float64) * At.out).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def test_frame_counts_follow_the_len_signal_quirk(golden_mdct):
    for B, T, frames in golden_mdct["quirk_frames_n1024"]:
        assert R.forward_layout(int(B), int(T), 512, 1024, True)[1] == int(frames)
    # a batch size that is no multiple of the hop lengthens the end pad: more frames than the hop-aligned count
    assert R.forward_layout(3, 128, 32, 64) == (32, (128 + 32 + 32 + 32 - 3 - 64) // 32 + 1)
    assert R.forward_layout(32, 128, 32, 64) == (32, (128 + 64 - 64) // 32 + 1)
    assert R.inverse_layout(5, 32, 64) == (32, 128) and R.inverse_layout(5, 32, 64, False) == (0, 192)
    assert R.inverse_layout(5, 32, 64, True, 100) == (32, 100)


def test_frames_f32_and_partial_frames():
    x = R.signal((2, 50), 31)
    w = R.window("ramp", 16)
    fr = R.frames_f32(x, w, 8, 16, 8, 9)                                 # frames 0 and 7, 8 hang over the ends
    assert fr.dtype == np.float32 and fr.shape == (2, 9, 16)
    assert not fr[:, 0, :8].any() and fr[:, 0, 8:].all()
    assert not fr[:, 8].any()                                            # wholly beyond the signal
    assert np.array_equal(fr[:, 1], x[:, 0:16] * w)
    ref = R.mdct4_ref(x, w, 16, 8, 16, 8, 9)
    assert not ref.out[:, 8].any() and ref.norms[:, 8].max() == 0.0


def test_spectro_references_restate_the_oracle():
    import torch
    s = R.spectro_spec(2, 9, 12, 41)
    for C in (1, 2):
        d, tol, pha = R.encode_db(s, C, 0.6, 1e-7)
        x = torch.from_numpy(s).double().unsqueeze(1).permute(0, 1, 3, 2)
        a, mv = float(np.float32(0.6)), float(np.float32(1e-7))
        if C == 2:
            neg = 0.5 * (x.abs() - x)
            pos = x + neg
            want = torch.cat((OM.amplitude_to_DB(a * pos + (1 - a) * neg, 20, mv, 1), OM.amplitude_to_DB((1 - a) * pos + a * neg, 20, mv, 1)), 1)
        else:
            want = OM.amplitude_to_DB(x.abs() + mv, 20, mv, 1)
        assert _rel(d, want.numpy()) <= PIN
        assert np.array_equal(pha, torch.sign(x).float().numpy())
        assert (tol > 0).all() and (tol < 1e-4).all()
    xs, ph, mm = R.decode_operands(2, 9, 12, 2, 42)
    v, tol = R.decode_ref(xs, mm, 0.6, 1e-7)
    t = torch.from_numpy(xs).double()
    den = 10.0 * torch.pow(10.0, (t.abs() * (float(mm[1]) - float(mm[0])) + float(mm[0])) * R.C005) - float(np.float32(1e-7))
    want = ((den[:, 0] - den[:, 1]) / (2 * float(np.float32(0.6)) - 1)).permute(0, 2, 1).numpy()
    assert _rel(v, want) <= PIN and (tol > 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 2. conditions of the operands, on the reference alone
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 48, 64, 1024, 2048, 4096])
def test_window_conditions(n):
    for seed in (0, 1):
        r, s = R.window("ramp", n, seed), R.window("sine", n)
        assert r.dtype == s.dtype == np.float32
        assert r.min() >= 0.5 and r.max() <= 1.5 and s.min() >= 0.3 and r.min() >= 0.3
        assert (r != r[::-1]).all(), "ramp must differ from its mirror image at every position"
        assert np.array_equal(s, s[::-1]) or np.abs(s - s[::-1]).max() <= 1e-7
    assert not np.array_equal(R.window("ramp", n, 0), R.window("ramp", n, 1))
    if n % 2 == 0 and n >= 64:
        k = R.window("kbd", n)
        assert (k < 1e-4).mean() > 0.05                                  # the blind spot the other two windows close


@pytest.mark.parametrize("n_fft", [64, 1024, 4096])
def test_signal_and_reference_conditions(n_fft):
    hop = n_fft // 2
    x = R.signal((3, 6 * hop - 4), 51)
    assert x.min() >= -1 and x.max() <= 1 and (np.abs(x) > 0.01).mean() > 0.95
    for kind in ("ramp", "sine"):
        w = R.window(kind, n_fft)
        ref = R.mdct4_ref(x, w, n_fft, hop, n_fft, hop, 8)                # frame 7 lies wholly beyond the signal
        live = ref.norms > 0
        assert not live[:, 7].any() and live[:, :7].all()
        tol = R.k_mdct4(n_fft) * U32 * ref.norms[..., None]
        assert (np.abs(ref.out)[live] > 100 * np.broadcast_to(tol, ref.out.shape)[live]).mean() >= 0.9
        S = R.signal((3, 7, n_fft // 2), 52)
        inv = R.imdct4_ref(S, w, n_fft, hop, n_fft, hop, 6 * hop - 4, 4.0 / n_fft)
        assert (np.abs(inv.out) > 100 * R.k_mdct4(n_fft) * U32 * inv.tol1).mean() >= 0.9
    if n_fft <= 2048:
        w = R.window("ramp", n_fft)
        ref = R.mdct2_ref(x, w, n_fft, hop, n_fft, hop, 7)
        tol = R.k_dct(n_fft) * U32 * ref.norms[..., None]
        assert (np.abs(ref.out) > 100 * tol).mean() >= 0.9


def test_decode_operands_have_no_ambiguous_sign():
    for (B, F, M) in ((2, 33, 40), (1, 1, 1), (3, 31, 64), (2, 64, 32)):
        x, pha, mm = R.decode_operands(B, F, M, 2, 100 * F + M)
        for keep in (0, M // 3, M):
            v, tol, amb = R.decode_signed_ref(x, pha, mm, 2, keep, R.MIN_VALUE, 0.5)
            assert not amb.any()
        if M > 2:
            v, _, _ = R.decode_signed_ref(x, pha, mm, 2, 0, R.MIN_VALUE, 1.0)
            assert not v[:, :, M // 2].any()                             # equal channels: sign 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. K
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", R.N_FFTS_MDCT4)
def test_k_mdct4_is_eight_times_the_measured_ratio_and_below_the_ceiling(n_fft):
    fwd, inv = R.measure_k_mdct4(n_fft)
    rec_f, rec_i, K = R.K_MDCT4_TABLE[n_fft]
    print(f"mdct4 n_fft {n_fft}: measured {fwd:.3f} / {inv:.3f}, recorded {rec_f} / {rec_i}, K {K}, ceiling {R.k_ceiling(n_fft)}")
    assert K >= 8.0 * max(fwd, inv), (n_fft, fwd, inv, K)
    assert K >= 8.0 * max(rec_f, rec_i) and K <= R.k_ceiling(n_fft)
    assert K < 8.0 * max(rec_f, rec_i) + 1.0                             # 8 x, rounded up to the next integer: no more


@pytest.mark.parametrize("n_fft", R.N_FFTS_DCT)
def test_k_dct_is_eight_times_the_measured_ratio_and_below_the_ceiling(n_fft):
    fwd, inv = R.measure_k_dct(n_fft)
    rec_f, rec_i, K = R.K_DCT_TABLE[n_fft]
    print(f"dct n_fft {n_fft}: measured {fwd:.3f} / {inv:.3f}, recorded {rec_f} / {rec_i}, K {K}, ceiling {R.k_ceiling(n_fft)}")
    assert K >= 8.0 * max(fwd, inv), (n_fft, fwd, inv, K)
    assert K >= 8.0 * max(rec_f, rec_i) and K <= R.k_ceiling(n_fft)
    assert K < 8.0 * max(rec_f, rec_i) + 1.0


# ----------------------------------------------------------------------------------------------------------------------
# 4. planted defects
# ----------------------------------------------------------------------------------------------------------------------
def _model32(x, w, n_fft, hop, start_pad, F, defect=None):
    """float32 model of p2phd_mdct4_fwd (win = n_fft): float32 gather and window product, the cosine sum in float64, rounded once."""
    x = np.array(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    if defect == "row_tail":                                             # (c) the last 4 samples of a row zeroed
        x[:, -4:] = 0
    fr = R.gather_frames(x, hop, n_fft, start_pad, F, dtype=np.float32)
    if defect == "fold":                                                 # (b) the first 16 positions of a 1024-frame (the same
        e = max(1, n_fft // 64)                                          # share of a shorter one) read one sample on
        fr[:, :, :e] = R.gather_frames(x, hop, n_fft, start_pad - 1, F, dtype=np.float32)[:, :, :e]
    fr = fr * (w[::-1] if defect == "mirror" else w)                     # (a) the window read mirrored
    S = (fr.astype(np.float64) @ R.cos4(n_fft)).astype(np.float32)
    if defect == "one_bin":                                              # (d) one element off by 1e-5 x the frame's RMS
        rms = float(np.sqrt((S[1, 2].astype(np.float64) ** 2).mean()))
        S[1, 2, 5] += np.float32(1e-5 * rms)
    return S


@pytest.mark.parametrize("n_fft", [64, 1024])
def test_planted_defects_fail_the_new_comparison_and_pass_the_old_one(n_fft):
    hop, F = n_fft // 2, 6
    T = (F - 1) * hop - 4
    x = R.signal((2, T), 61)
    K = R.k_mdct4(n_fft)
    ramp, kbd = R.window("ramp", n_fft), R.window("kbd", n_fft)
    ref = R.mdct4_ref(x, ramp, n_fft, hop, n_fft, hop, F)
    worst = R.assert_frames_close(_model32(x, ramp, n_fft, hop, hop, F), ref, K, "sound model")
    assert worst < 0.5                                                   # the sound model sits well inside the bound
    for defect in ("mirror", "fold", "row_tail", "one_bin"):
        with pytest.raises(AssertionError) as e:
            R.assert_frames_close(_model32(x, ramp, n_fft, hop, hop, F, defect), ref, K, defect)
        assert "histograms" in str(e.value) and defect in str(e.value)
    # the same defects under the shipped window and measure: invisible (why these tests exist)
    ref_kbd = R.mdct4_ref(x, kbd, n_fft, hop, n_fft, hop, F)
    for defect in ("mirror", "fold", "one_bin"):
        assert rel_err(_model32(x, kbd, n_fft, hop, hop, F, defect), ref_kbd.out) < 1e-4, defect
    # ... while the per-element bound sees the single bin even there
    for defect in ("one_bin",):
        with pytest.raises(AssertionError):
            R.assert_frames_close(_model32(x, kbd, n_fft, hop, hop, F, defect), ref_kbd, K, defect)


def test_comparison_functions_report_where():
    n_fft, hop, F = 64, 32, 9
    x = R.signal((2, 8 * hop), 71)
    w = R.window("ramp", n_fft)
    ref = R.mdct4_ref(x, w, n_fft, hop, n_fft, hop, F + 1)               # + a frame beyond the signal: must be exactly zero
    good = ref.out.astype(np.float32)
    assert R.assert_frames_close(good, ref, R.k_mdct4(n_fft), "ok") <= 1.0
    bad = good.copy()
    bad[0, F, 3] = 1e-30                                                 # anything but zero in a zero frame
    with pytest.raises(AssertionError, match="'t': {9: 1}"):
        R.assert_frames_close(bad, ref, R.k_mdct4(n_fft), "zero frame")
    neg = good.copy()
    neg[0, F, 3] = -0.0                                                  # the sign of a zero is not compared
    R.assert_frames_close(neg, ref, R.k_mdct4(n_fft), "minus zero")
    nan = good.copy()
    nan[1, 2, 7] = np.nan
    with pytest.raises(AssertionError):
        R.assert_frames_close(nan, ref, R.k_mdct4(n_fft), "nan")
    S = R.signal((2, 3, n_fft // 2), 72)
    inv = R.imdct4_ref(S, w, n_fft, hop, n_fft, 0, 6 * hop, 4.0 / n_fft)  # 3 frames cover 4 hops of the 6
    assert inv.covered[:4 * hop].all() and not inv.covered[4 * hop:].any()
    y = inv.out.astype(np.float32)
    assert R.assert_samples_close(y, inv, R.k_mdct4(n_fft), "ok", hop) <= 1.0
    y[1, 5 * hop + 3] = 1e-30
    with pytest.raises(AssertionError, match="'m//hop': {5: 1}"):
        R.assert_samples_close(y, inv, R.k_mdct4(n_fft), "uncovered", hop)
    y = inv.out.astype(np.float32)
    y[0, hop + 1] += np.float32(1e-4)
    with pytest.raises(AssertionError, match="'m%hop': {1: 1}"):
        R.assert_samples_close(y, inv, R.k_mdct4(n_fft), "seam", hop)
