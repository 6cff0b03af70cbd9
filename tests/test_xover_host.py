"""Host side of the time-domain crossover (no GPU): generate.crossover_plan against its restatement, p2phd_xover_taps_fill
against the float64 formula, the quality of the filter it fills, and the command-line / constructor plumbing."""
import ctypes
import os

import numpy as np
import pytest

import _xover_ref as R

TAPS = (1, 3, 63, 255, 1023, 4095)
CUTOFFS = (0.05, 0.11875, 0.2375, 0.45)
RATES = ((48000, 12000), (48000, 24000), (16000, 8000), (44100, 11025))


def _fill(taps, cutoff, beta=R.BETA, n=None):
    from pix2pixhdaudiosr_amd import _lib
    buf = np.full(max(taps, 1) if n is None else n, np.float32(7.0))
    rc = _lib.lib().p2phd_xover_taps_fill(taps, cutoff, beta, ctypes.c_void_p(buf.ctypes.data))
    return rc, buf


# ------------------------------------------------------------------------------------------
# crossover_plan
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hr,lr", RATES)
def test_plan_defaults_equal_the_restatement_and_are_minimal(hr, lr):
    from pix2pixhdaudiosr_amd.generate import crossover_plan
    taps, cutoff, beta = crossover_plan(hr, lr)
    assert (taps, cutoff, beta) == R.crossover_plan_ref(hr, lr)
    assert beta == 8.96 and cutoff == 0.95 * lr / 2.0 / hr
    fc = cutoff * hr
    assert taps % 2 == 1 and fc + R.width_ref(hr, taps) / 2 <= lr / 2
    assert fc + R.width_ref(hr, taps - 2) / 2 > lr / 2             # taps - 2 violates the condition
    # the same taps handed in are accepted and come back; another crossover frequency moves the default
    assert crossover_plan(hr, lr, taps=taps) == (taps, cutoff, beta)
    assert crossover_plan(hr, lr, crossover_hz=0.8 * lr / 2) == R.crossover_plan_ref(hr, lr, 0.8 * lr / 2)


def test_plan_of_the_published_rates():
    from pix2pixhdaudiosr_amd.generate import crossover_plan
    assert crossover_plan(48000, 12000) == (459, 0.11875, 8.96)


def test_plan_refusals_name_their_numbers():
    from pix2pixhdaudiosr_amd.generate import crossover_plan
    for lr in (48000, 96000):                                      # nothing to cross over
        with pytest.raises(ValueError, match=r"nothing to cross over.*%d" % lr):
            crossover_plan(48000, lr)
    for hz in (0.0, -5.0, 6000.0, 7000.0):                         # outside (0, lr / 2)
        with pytest.raises(ValueError, match=r"crossover_hz must lie in \(0, 6000\).*got %g" % hz):
            crossover_plan(48000, 12000, crossover_hz=hz)
    for taps in (0, 2, 458, 4096, 4097, -3):                       # even, or outside [1, 4095]
        with pytest.raises(ValueError, match=r"taps must be an odd int in \[1, 4095\], got %d" % taps):
            crossover_plan(48000, 12000, taps=taps)
    for taps in (1, 101, 457):                                     # the transition band ends above the low rate's Nyquist frequency
        with pytest.raises(ValueError, match=r"with %d taps the transition band .* above the low rate's Nyquist frequency 6000" % taps):
            crossover_plan(48000, 12000, taps=taps)
    with pytest.raises(ValueError, match=r"needs 5487 taps at 48000 Hz, more than 4095"):      # a default beyond 4095
        crossover_plan(48000, 1000)
    assert R.crossover_plan_ref(48000, 1000)[0] == 5487
    crossover_plan(48000, 12000, taps=4095)


# ------------------------------------------------------------------------------------------
# p2phd_xover_taps_fill
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", TAPS)
def test_taps_fill_matches_the_float64_formula(taps):
    for cutoff in CUTOFFS:
        rc, got = _fill(taps, cutoff)
        assert rc == 0 and got.dtype == np.float32 and got.shape == (taps,)
        want = R.taps_ref(taps, cutoff, R.BETA)
        w32 = want.astype(np.float32)
        # within 1 fp32 ulp of the restatement rounded to fp32: two float64 evaluations of I0 may round one tap differently
        assert (np.sign(got) == np.sign(w32)).all() and (got != 0).all()
        ulps = np.abs(got.view(np.int32).astype(np.int64) - w32.view(np.int32).astype(np.int64))
        print(f"taps {taps} cutoff {cutoff}: {int((ulps > 0).sum())} taps differ, by at most {int(ulps.max())} ulp")
        assert ulps.max() <= 1, (taps, cutoff, int(ulps.max()))
        assert abs(got.astype(np.float64).sum() - 1.0) <= taps * 2.0 ** -25
        assert np.array_equal(got.view(np.int32), got[::-1].view(np.int32))           # symmetric bit for bit
    if taps == 1:
        assert got[0] == 1.0


def test_taps_fill_other_beta_and_canary():
    for beta in (0.0, 5.0):
        rc, got = _fill(63, 0.2, beta, n=64)
        want = R.taps_ref(63, 0.2, beta).astype(np.float32)
        assert rc == 0 and got[63] == 7.0                          # writes `taps` values, no more
        assert np.abs(got[:63].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max() <= 1


def test_taps_fill_refusals():
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    einval = L.p2phd_mdct4_tables_fill(100, None)                  # P2PHD_EINVAL, as a neighbouring host entry gives it
    assert einval != 0
    for taps, cutoff, beta, word in ((2, 0.1, 8.96, "taps"), (0, 0.1, 8.96, "taps"), (4097, 0.1, 8.96, "taps"), (-1, 0.1, 8.96, "taps"),
                                     (63, 0.0, 8.96, "cutoff"), (63, 0.5, 8.96, "cutoff"), (63, 0.1, -1.0, "beta")):
        rc, got = _fill(taps, cutoff, beta, n=8)
        text = L.p2phd_last_error().decode()
        assert rc == einval and "xover_taps_fill" in text and word in text, (taps, cutoff, beta, rc, text)
        assert (got == 7.0).all()                                  # refused before anything was written
    assert L.p2phd_xover_taps_fill(63, 0.1, 8.96, None) == einval and "null" in L.p2phd_last_error().decode()
    assert L.p2phd_xover_tile_len() >= 1024


# ------------------------------------------------------------------------------------------
# what the filled filter does
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hr,lr", [(48000, 12000), (16000, 8000)])
def test_filter_quality(hr, lr):
    """Pass band |H - 1| <= 1e-4 up to crossover_hz - width / 2, stop band |H| <= -85 dB from crossover_hz + width / 2, from a
    2^18-point FFT of the fp32 taps (the float64 restatement gives 3.1e-5 .. 3.4e-5 and -89.7 .. -90.1 dB: about 3 x and 5 dB
    of room).  H is taken zero-phase: the taps are centred."""
    from pix2pixhdaudiosr_amd.generate import crossover_plan
    taps, cutoff, beta = crossover_plan(hr, lr)
    rc, h = _fill(taps, cutoff, beta)
    assert rc == 0
    N = 1 << 18
    c0 = (taps - 1) // 2
    x = np.zeros(N)
    x[:taps - c0] = h[c0:]                                         # centred at index 0, wrapped
    x[N - c0:] = h[:c0]
    H = np.fft.rfft(x)
    assert np.abs(H.imag).max() < 1e-12                            # symmetric taps: a real response
    f = np.arange(N // 2 + 1) * hr / N
    fc, width = cutoff * hr, R.width_ref(hr, taps)
    passband = np.abs(H[f <= fc - width / 2] - 1.0).max()
    stop = 20 * np.log10(np.abs(H[f >= fc + width / 2]).max())
    half = np.abs(H[np.argmin(np.abs(f - fc))])
    print(f"{hr}/{lr}: {taps} taps, pass band deviation {passband:.3e}, stop band {stop:.2f} dB, |H(fc)| {half:.4f}")
    assert passband <= 1e-4
    assert stop <= -85.0
    assert abs(half - 0.5) < 5e-3                                  # the cutoff is the -6 dB point
    assert fc + width / 2 <= lr / 2


# ------------------------------------------------------------------------------------------
# plumbing that needs no device
# ------------------------------------------------------------------------------------------
def test_parser_accepts_the_flags_and_defaults_to_off():
    from pix2pixhdaudiosr_amd import generate as G
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ckpt"]
    a = G._parser().parse_args(base)
    assert (a.crossover, a.crossover_hz, a.crossover_taps) == (None, None, None)
    assert (a.lowband, a.clip, a.dither) == ("model", "clamp", None)            # the neighbours' defaults are where they were
    a = G._parser().parse_args(base + ["--crossover", "input", "--crossover_hz", "5000.5", "--crossover_taps", "255"])
    assert (a.crossover, a.crossover_hz, a.crossover_taps) == ("input", 5000.5, 255)
    with pytest.raises(SystemExit):
        G._parser().parse_args(base + ["--crossover", "model"])
    assert G.LOWBANDS == ('model', 'input') and G.CROSSOVERS == (None, 'input')


def test_check_paths_is_unchanged(tmp_path):
    from pix2pixhdaudiosr_amd import generate as G
    f = tmp_path / "a.wav"
    f.write_bytes(b"")
    d = tmp_path / "d"
    d.mkdir()
    assert G.check_paths(str(f), str(tmp_path / "out.wav")) is False
    assert G.check_paths(str(d), str(tmp_path / "new")) is True
    with pytest.raises(ValueError):
        G.check_paths(str(f), str(d))
    with pytest.raises(ValueError):
        G.check_paths(str(d), str(f))
    assert G.select_channels('all', 3) == 3 and G.check_output_options('pcm16') is None


def test_check_crossover():
    from pix2pixhdaudiosr_amd import generate as G
    assert G.check_crossover(None, None, None, 48000, 48000) is None             # off: the rates are not looked at
    assert G.check_crossover('input', None, None, 48000, 12000) == (459, 0.11875, 8.96)
    assert G.check_crossover('input', 5000.0, 255, 48000, 12000) == (255, 5000.0 / 48000, 8.96)
    with pytest.raises(ValueError, match=r"crossover must be None or 'input'"):
        G.check_crossover('model', None, None, 48000, 12000)
    with pytest.raises(ValueError, match=r"nothing to cross over"):
        G.check_crossover('input', None, None, 48000, 48000)
    for kw in (dict(crossover_hz=5000.0), dict(crossover_taps=255)):
        with pytest.raises(ValueError, match=r"options of crossover='input'"):
            G.check_crossover(None, kw.get('crossover_hz'), kw.get('crossover_taps'), 48000, 12000)
