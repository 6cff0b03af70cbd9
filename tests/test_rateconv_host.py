"""The host side of the output stage's rate converter (csrc/rateconv.hip: p2phd_rateconv_plan, p2phd_rateconv_taps_fill,
p2phd_rateconv_out_len; generate.rateconv_plan, rateconv_coefficients, check_output_rate) against the float64 restatement of
tests/_rateconv_ref.py: the plan, the table, the response of the fp32 table, tones through the restated sum, lengths and every
refusal.  No GPU: the three entry points are host arithmetic."""
import ctypes
import math

import numpy as np
import pytest

import _rateconv_ref as R

PAIRS = ((48000, 44100), (44100, 48000), (48000, 96000), (48000, 32000), (48000, 16000))
TAPS = (92, 84, 84, 126, 252)


def _gen():
    from pix2pixhdaudiosr_amd import generate
    return generate


@pytest.fixture(scope="module")
def tables():
    """(plan of the library, its fp32 table, the restatement's float64 table) per rate pair, computed once."""
    g = _gen()
    out = {}
    for pair in PAIRS:
        plan = g.rateconv_plan(*pair)
        ref = R.plan(*pair)
        out[pair] = (plan, g.rateconv_coefficients(plan).numpy(), R.table(ref['o'], ref['n'], ref['taps_per_phase'], ref['beta'], ref['cutoff']))
    return out


def test_plan_reads_the_stated_lengths(tables):
    g = _gen()
    assert g.RATECONV_DEFAULTS == {'passband': 0.907, 'atten_db': 120.0}
    for pair, P in zip(PAIRS, TAPS):
        plan, ref = tables[pair][0], R.plan(*pair)
        gcd = math.gcd(*pair)
        assert (plan['o'], plan['n'], plan['taps_per_phase']) == (pair[0] // gcd, pair[1] // gcd, P) == (ref['o'], ref['n'], ref['taps_per_phase'])
        assert round(plan['beta'], 3) == 12.265 and plan['beta'] == pytest.approx(ref['beta'], rel=1e-15)
        assert plan['cutoff'] == ref['cutoff'] == min(pair) / pair[0]
        assert plan['passband_hz'] == pytest.approx(0.907 * min(pair) / 2, rel=1e-15)
        assert plan['stopband_hz'] == pytest.approx(min(pair) - plan['passband_hz'], rel=1e-15)
        assert plan['atten_db'] == 120.0
    assert tables[(48000, 44100)][0]['passband_hz'] == pytest.approx(19999.35) and tables[(48000, 44100)][0]['stopband_hz'] == pytest.approx(24100.65)
    # options of the plan: a narrower passband asks for fewer taps, less attenuation too
    assert g.rateconv_plan(48000, 44100, passband=0.8)['taps_per_phase'] < 92 > g.rateconv_plan(48000, 44100, atten_db=90.0)['taps_per_phase']
    assert g.rateconv_plan(48000, 44100, atten_db=90.0)['beta'] == pytest.approx(0.1102 * (90.0 - 8.7))


def test_plan_refusals():
    g = _gen()
    with pytest.raises(ValueError, match="504 taps per phase"):
        g.rateconv_plan(48000, 8000)                                        # P > 256
    with pytest.raises(ValueError, match="nothing to convert"):
        g.rateconv_plan(48000, 48000)
    with pytest.raises(ValueError, match="more than 1048576 coefficients"):
        g.rateconv_plan(48000, 44101)                                       # n * P > 2^20: the rates share no divisor
    for passband in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError, match="passband"):
            g.rateconv_plan(48000, 44100, passband=passband)
    for atten in (39.9, 160.1, float('nan')):
        with pytest.raises(ValueError, match="attenuation"):
            g.rateconv_plan(48000, 44100, atten_db=atten)
    for bad in (0, -1, 44100.0, True, None, "44100"):
        with pytest.raises(ValueError, match="must be an int"):
            g.rateconv_plan(48000, bad)
        with pytest.raises(ValueError, match="must be an int"):
            g.rateconv_plan(bad, 48000)
    # (P < 4 cannot be reached through the rates: the widest transition band, passband -> 0 at 40 dB, still asks for 4 taps)
    assert g.rateconv_plan(8000, 16000, passband=0.001, atten_db=40.0)['taps_per_phase'] == 4


def test_entry_points_run_without_a_device_and_refuse_bad_arguments():
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    o, n, P, beta = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    assert L.p2phd_rateconv_plan(48000, 44100, 0.907, 120.0, ctypes.byref(o), ctypes.byref(n), ctypes.byref(P), ctypes.byref(beta)) == 0
    assert (o.value, n.value, P.value) == (160, 147, 92)
    assert L.p2phd_rateconv_plan(48000, 44100, 0.907, 120.0, None, ctypes.byref(n), ctypes.byref(P), ctypes.byref(beta)) != 0
    buf = np.full(147 * 92 + 1, 7.0, dtype=np.float32)
    assert L.p2phd_rateconv_taps_fill(160, 147, 92, beta.value, 147 / 160, ctypes.c_void_p(buf.ctypes.data)) == 0
    assert buf[-1] == 7.0 and np.all(np.abs(buf[:-1]) < 1.0)
    for args in ((160, 147, 91, 12.0, 0.9), (160, 147, 2, 12.0, 0.9), (160, 147, 258, 12.0, 0.9), (0, 147, 92, 12.0, 0.9), (160, 0, 92, 12.0, 0.9),
                 (1, 8192, 256, 12.0, 0.9), (160, 147, 92, -1.0, 0.9), (160, 147, 92, float('inf'), 0.9), (160, 147, 92, 12.0, 0.0),
                 (160, 147, 92, 12.0, 1.5)):
        assert L.p2phd_rateconv_taps_fill(*args, ctypes.c_void_p(buf.ctypes.data)) != 0, args
        assert b"rateconv_taps_fill" in L.p2phd_last_error()
    assert L.p2phd_rateconv_taps_fill(160, 147, 92, 12.0, 0.9, None) != 0
    assert L.p2phd_rateconv_out_len(-1, 48000, 44100) == -1 and L.p2phd_rateconv_out_len(10, 0, 44100) == -1
    assert L.p2phd_rateconv_out_len((1 << 40) + 1, 48000, 44100) == -1 and b"rateconv_out_len" in L.p2phd_last_error()
    assert L.p2phd_rateconv_tile_len(160, 147, 92) > 0 and L.p2phd_rateconv_tile_len(160, 147, 91) == -1


def test_output_lengths():
    g = _gen()
    for pair in PAIRS + ((44100, 8000), (8000, 192000)):
        gcd = math.gcd(*pair)
        o, n = pair[0] // gcd, pair[1] // gcd
        for L in (0, 1, 2, o - 1, o, o + 1, 7 * o + 3, 48000 * 15, 48000 * 3600, 1 << 36):
            want = -((-L * pair[1]) // pair[0])
            assert g.rateconv_out_len(L, *pair) == want == R.out_len(L, o, n) == g.rateconv_out_len(L, o, n), (pair, L)
    assert g.rateconv_out_len(720000, 48000, 44100) == 661500
    with pytest.raises(ValueError):
        g.rateconv_out_len(-1, 48000, 44100)


def test_table_agrees_with_the_restatement(tables):
    for pair in PAIRS:
        plan, c32, c64 = tables[pair]
        P = plan['taps_per_phase']
        assert c32.shape == c64.shape == (plan['n'], P) and c32.dtype == np.float32
        ulp = float(np.spacing(np.float32(np.abs(c64).max())))
        assert np.abs(c32.astype(np.float64) - c64).max() <= 2 * ulp, pair
        # every phase has DC gain 1: within P spacings of the numbers below 1
        assert np.abs(c32.astype(np.float64).sum(axis=1) - 1.0).max() <= P * 2.0 ** -24, pair
        assert np.abs(c64.sum(axis=1) - 1.0).max() <= 1e-15


def test_response_of_the_fp32_table(tables):
    """Flat within +-1e-4 dB up to the passband's end, at most -118 dB from the stopband's start to the fine rate's Nyquist frequency
    -- where every alias (going down) and every image (going up) comes from.  Measured when this was written: +-1.05e-5 dB and -118.8 to
    -119.9 dB, with the float64 and the fp32 table alike."""
    for pair in PAIRS:
        plan, c32, c64 = tables[pair]
        for c in (c32, c64):
            f, db = R.response_db(c, plan['o'], plan['n'], pair[0])
            ripple = np.abs(db[f <= plan['passband_hz']]).max()
            stop = db[f >= plan['stopband_hz']].max()
            print("%d -> %d (%s): ripple %.2e dB, stopband %.2f dB" % (pair + (c.dtype, ripple, stop)))
            assert ripple <= 1e-4, (pair, ripple)
            assert stop <= -118.0, (pair, stop)


def _tone(f, rate, count):
    return 0.5 * np.sin(2.0 * np.pi * f * np.arange(count, dtype=np.float64) / rate)


@pytest.mark.parametrize("pair", ((48000, 44100), (44100, 48000)))
@pytest.mark.parametrize("f", (997.0, 19000.0))
def test_a_tone_comes_out_as_the_tone_at_the_new_rate(tables, pair, f):
    """Output m of the sum stands at time m / out_rate: a passband tone through the restatement is the analytic tone sampled at the
    new rate, within 1e-6 away from the 2 P samples at either end (measured when this was written: 1.7e-8 to 3.3e-7)."""
    plan, _, c64 = tables[pair]
    P = plan['taps_per_phase']
    y = R.convert(_tone(f, pair[0], 6000), c64, plan['o'], plan['n'])
    assert len(y) == R.out_len(6000, plan['o'], plan['n'])
    err = np.abs(y - _tone(f, pair[1], len(y)))[2 * P:-2 * P].max()
    print("%d -> %d, %g Hz: %.2e" % (pair + (f, err)))
    assert err <= 1e-6


def test_a_tone_above_the_new_band_is_removed(tables):
    """20 kHz lies above the stopband's start of 48000 -> 32000 (17.488 kHz): what is left is under -118 dB of the tone (measured
    when this was written: -132.5 dB)."""
    plan, _, c64 = tables[(48000, 32000)]
    P = plan['taps_per_phase']
    y = R.convert(_tone(20000.0, 48000, 6000), c64, plan['o'], plan['n'])
    left = 20.0 * np.log10(np.abs(y[2 * P:-2 * P]).max() / 0.5)
    print("left: %.1f dB" % left)
    assert left < -118.0


def test_check_output_rate():
    g = _gen()
    assert g.check_output_rate(None, 48000) is None
    assert g.check_output_rate(48000, 48000) is None and g.check_output_rate(48000, 48000.0) is None
    assert g.check_output_rate(48000, 48000, "x", 'folder', "p.png") is None          # off: nothing to refuse
    rc = g.check_output_rate(44100, 48000)
    assert (rc['rate'], rc['model_rate']) == (44100, 48000) and rc['plan'] == g.rateconv_plan(48000, 44100)
    assert g.check_output_rate(96000, 48000.0)['plan']['n'] == 2
    for bad in (7999, 0, -44100, 44100.0, True, "44100"):
        with pytest.raises(ValueError, match="enhance_file: output_rate must be an int >= 8000"):
            g.check_output_rate(bad, 48000)
    with pytest.raises(ValueError, match="who: spectrogram is not built with output_rate"):
        g.check_output_rate(44100, 48000, "who", 'file', "p.png")
    with pytest.raises(ValueError, match="who: output_rate is not built for loudness_scope='folder'"):
        g.check_output_rate(44100, 48000, "who", 'folder')
    with pytest.raises(ValueError, match="who: output_rate 8000: rateconv_plan: 48000 -> 8000 Hz .* 504 taps"):
        g.check_output_rate(8000, 48000, "who")
    with pytest.raises(ValueError, match="whole number of Hz"):
        g.check_output_rate(44100, 47999.5)
    line = g.plans.output_rate_line(rc)
    assert line == "output rate: 44100 Hz (92 taps x 147 phases, flat to 20.00 kHz, -120 dB from 24.10 kHz)"
