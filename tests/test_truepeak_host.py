"""The true-peak measurement without a GPU: the host fill of the polyphase table (p2phd_truepeak_taps_fill needs only the built
library) against the float64 restatement of tests/_truepeak_ref.py, its refusals, the plan per rate, what the restatement measures
on tones whose true peak is known, and the option on its way through enhance_file / enhance_folder / the command line / the CSV."""
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import _truepeak_ref as R

FACTORS, TAPS, BETAS = (1, 2, 4), (4, 12, 24, 64), (0.0, 5.0, 9.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _ulps(a, b):
    """Distance of two float32 arrays in units in the last place (both finite, signs handled through the ordered integers)."""
    def ordered(x):
        i = _bits(x).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


@pytest.mark.parametrize("F,P,beta", list(itertools.product(FACTORS, TAPS, BETAS)))
def test_table(F, P, beta):
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients
    c = true_peak_coefficients(F, P, beta).numpy()
    want = R.table(F, P, beta)
    assert c.shape == (F, P) and c.dtype == np.float32
    worst = int(_ulps(c, want.astype(np.float32)).max())
    print("F %d P %d beta %g: worst distance from the rounded restatement %d ulp" % (F, P, beta, worst))
    assert worst <= 2
    impulse = np.zeros(P, dtype=np.float32)
    impulse[P // 2 - 1] = 1.0
    assert np.array_equal(_bits(c[0]), _bits(impulse))             # (+0 everywhere else, bit for bit)
    for p in range(1, F):
        assert np.array_equal(_bits(c[p]), _bits(c[F - p][::-1])), p
        assert abs(c[p].astype(np.float64).sum() - 1.0) <= P * 2.0 ** -24, p
    # the restatement has the same structure in float64
    assert all(np.allclose(want[p], want[F - p][::-1], rtol=0, atol=1e-15) for p in range(1, F))


def test_refusals():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients
    lib = _lib.lib()
    out = np.full(4 * 66 + 8, 7.0, dtype=np.float32)
    p = ctypes.c_void_p(out.ctypes.data)
    assert lib.p2phd_truepeak_taps_fill(4, 24, 9.0, p) == 0
    out[:] = 7.0
    for args, word in (((3, 24, 9.0, p), "factor"), ((0, 24, 9.0, p), "factor"), ((8, 24, 9.0, p), "factor"), ((4, 23, 9.0, p), "even"),
                       ((4, 2, 9.0, p), "[4, 64]"), ((4, 66, 9.0, p), "[4, 64]"), ((4, 24, float('nan'), p), "beta"),
                       ((4, 24, -1.0, p), "beta"), ((4, 24, float('inf'), p), "beta"), ((4, 24, 9.0, None), "null")):
        rc = lib.p2phd_truepeak_taps_fill(*args)
        text = lib.p2phd_last_error().decode()
        assert rc != 0 and "truepeak_taps_fill" in text and word in text, (args[:3], rc, text)
    assert (out == 7.0).all()                                      # nothing written by a refused call
    with pytest.raises(_lib.P2PHDError, match="truepeak_taps_fill"):
        true_peak_coefficients(3, 24, 9.0)
    assert lib.p2phd_truepeak_tile_len() >= 64


def test_truepeak_plan():
    from pix2pixhdaudiosr_amd.generate import TRUEPEAK_BETA, TRUEPEAK_TAPS_PER_PHASE, truepeak_plan
    assert (TRUEPEAK_TAPS_PER_PHASE, TRUEPEAK_BETA) == (24, 9.0)
    for rate, factor in ((8000, 4), (44100, 4), (48000, 4), (95999, 4), (96000, 2), (191999, 2), (192000, 1), (384000, 1)):
        assert truepeak_plan(rate) == {'factor': factor, 'taps_per_phase': 24, 'beta': 9.0}, rate
        assert rate * factor >= 192000 or factor == 4
    for bad in (0, -48000, float('nan'), float('inf'), '48000', None, True):
        with pytest.raises(ValueError, match="truepeak_plan"):
            truepeak_plan(bad)


TONES = ((0.25, np.pi / 4), (0.125, np.pi / 8), (0.2, 0.3), (0.3, 0.7))


def _plan_table(rate=48000):
    from pix2pixhdaudiosr_amd.generate import truepeak_plan
    plan = truepeak_plan(rate)
    return R.table(plan['factor'], plan['taps_per_phase'], plan['beta'])


@pytest.mark.parametrize("f,phi", TONES)
def test_the_restatement_reads_the_true_peak_of_a_tone(f, phi):
    """sin(2 pi f n + phi) under raised-cosine ramps: the restatement's true peak against the largest |sin| on the 4x grid of the
    flat part, within 0.005 dB."""
    c = _plan_table()
    x = R.ramped_tone(f, phi)
    t4 = np.arange(4 * 2400, 4 * 7200) / 4.0
    want = np.abs(np.sin(2.0 * np.pi * f * t4 + phi)).max()
    got = R.true_peak(x, c)
    diff = 20.0 * np.log10(got / want)
    print("f %g phi %.4f: true peak %.6f, on the 4x grid %.6f, %+.4f dB; sample peak %+.4f dB" % (f, phi, got, want, diff, 20.0 * np.log10(np.abs(x).max())))
    assert abs(diff) <= 0.005
    assert got >= np.abs(x).max()
    if (f, phi) == TONES[0]:
        assert abs(20.0 * np.log10(np.abs(x).max()) - (-3.0103)) <= 1e-4


@pytest.mark.parametrize("f,phi", ((0.4, 0.1), (0.45, 0.2)))
def test_beyond_the_passband_the_true_peak_is_at_least_the_sample_peak(f, phi):
    x = R.ramped_tone(f, phi)
    assert R.true_peak(x, _plan_table()) >= np.abs(x).max()


def test_restatement_edges():
    c = R.table(4, 4, 9.0)
    y = R.oversampled(np.array([1.0, np.nan, -np.inf, 2.0]), c)
    assert y.shape == (5, 4) and (y[:, 0] == [0.0, 1.0, 0.0, 0.0, 2.0]).all()
    # instant i = -1, phase 3: c[3][2] x[0] + c[3][3] x[1] with x[1] taken as 0
    assert y[0, 3] == c[3, 2] * 1.0
    assert R.true_peak(np.zeros(0), c) == 0.0 and R.gain([0.0], 0.5) == 1.0
    assert R.gain([0.25, 2.0], 0.5) == np.float32(0.5) / np.float32(2.0) and R.gain([0.5], 0.5) == 1.0
    assert R.dot_bound(np.ones((2, 5)), R.table(1, 4, 9.0)).tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------
# the option
# ------------------------------------------------------------------------------------------
def test_true_peak_must_be_a_bool_and_comes_with_a_stage(tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, check_true_peak, encoding_limit
    assert check_true_peak(False, None, 'pcm16', 48000) == (None, None)
    stage = {'clip': 'guard', 'ceiling': 0.5, 'dither': None, 'seed': 0, 'report': False}
    assert check_true_peak(False, stage, 'pcm16', 48000) == (stage, None)
    got, tp = check_true_peak(True, None, 'pcm16', 48000)
    assert got == {'clip': 'clamp', 'ceiling': None, 'dither': None, 'seed': 0, 'report': False}
    assert tp == {'rate': 48000, 'ceiling': encoding_limit('pcm16'), 'limit': encoding_limit('pcm16')}
    got, tp = check_true_peak(True, stage, 'float32', 44100)
    assert got is stage and tp == {'rate': 44100, 'ceiling': 0.5, 'limit': 1.0}
    sr = SuperResolver.__new__(SuperResolver)                      # no model, no device: the checks come first
    sr.opt = SimpleNamespace(hr_sampling_rate=48000)
    missing = str(tmp_path / "missing.wav")
    for bad in (1, 0, None, 'yes', 1.0):
        with pytest.raises(ValueError, match="true_peak must be a bool"):
            check_true_peak(bad, None, 'pcm16', 48000)
        with pytest.raises(ValueError, match="true_peak must be a bool"):
            sr.enhance_file(missing, str(tmp_path / "out.wav"), true_peak=bad)
        with pytest.raises(ValueError, match="true_peak must be a bool"):
            sr.enhance_folder(str(tmp_path / "no_such_folder"), str(tmp_path / "out"), true_peak=bad)
    assert not (tmp_path / "out.wav").exists() and not (tmp_path / "out").exists()


def test_check_output_options_is_unchanged():
    from pix2pixhdaudiosr_amd.generate import check_output_options
    assert check_output_options('pcm16') is None
    assert check_output_options('float32', 'clamp', None, None, 0, False, "x") is None
    assert check_output_options('pcm16', 'guard', -1.0, 'tpdf', 11, True) == \
        {'clip': 'guard', 'ceiling': 10.0 ** (-1.0 / 20.0), 'dither': 'tpdf', 'seed': 11, 'report': True}
    assert check_output_options('pcm24', report_peaks=True) == {'clip': 'clamp', 'ceiling': None, 'dither': None, 'seed': 0, 'report': True}
    assert check_output_options('float32', 'error') == {'clip': 'error', 'ceiling': None, 'dither': None, 'seed': 0, 'report': False}
    with pytest.raises(TypeError):
        check_output_options('pcm16', true_peak=True)              # the option travels beside the stage, not inside


def test_csv_column_only_with_the_option(tmp_path):
    from pix2pixhdaudiosr_amd.generate import (METRICS_COLUMNS, METRICS_COLUMNS_LOUDNESS, METRICS_COLUMNS_PEAKS, METRICS_COLUMNS_TRUE_PEAK,
                                                metrics_rows, write_metrics_csv)
    assert METRICS_COLUMNS_TRUE_PEAK == ("true_peak_dbtp",)
    rec = {'path': 'a.wav', 'out_frames': 10, 'metrics': [(1.0, 2.0, 3.0, 0, 0, 0, 4.0)] * 2,
           'output': {'peak_dbfs': [-1.0, -2.0], 'clipped': [0, 1], 'gain': 1.0, 'true_peak_dbtp': [-0.5, -1.5]},
           'loudness': {'input': -30.0, 'measured': -20.0, 'gain_db': -3.0, 'output': -23.0, 'momentary_max': -21.0, 'target': -23.0}}
    assert metrics_rows([rec])[0] == ('a.wav', 0, 10, 1.0, 2.0, 3.0, 4.0)
    assert metrics_rows([rec], False, True)[1] == ('a.wav', 1, 10, 1.0, 2.0, 3.0, 4.0, -2.0, 1, 1.0)
    rows = metrics_rows([rec], true_peak=True)
    assert rows[0] == ('a.wav', 0, 10, 1.0, 2.0, 3.0, 4.0, -0.5) and rows[1][-1] == -1.5 and rows[-1][-1] == -1.0
    rows = metrics_rows([rec], False, True, True, True)
    assert rows[1] == ('a.wav', 1, 10, 1.0, 2.0, 3.0, 4.0, -2.0, 1, 1.0, -30.0, -23.0, -3.0, -1.5)
    write_metrics_csv(str(tmp_path / "off.csv"), [rec])
    write_metrics_csv(str(tmp_path / "peaks.csv"), [rec], False, True)
    write_metrics_csv(str(tmp_path / "on.csv"), [rec], true_peak=True)
    write_metrics_csv(str(tmp_path / "all.csv"), [rec], False, True, True, True)
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(METRICS_COLUMNS)
    assert open(str(tmp_path / "peaks.csv")).readline().strip() == ",".join(METRICS_COLUMNS + METRICS_COLUMNS_PEAKS)
    assert open(str(tmp_path / "on.csv")).readline().strip() == ",".join(METRICS_COLUMNS + METRICS_COLUMNS_TRUE_PEAK)
    assert open(str(tmp_path / "all.csv")).readline().strip() == \
        ",".join(METRICS_COLUMNS + METRICS_COLUMNS_PEAKS + METRICS_COLUMNS_LOUDNESS + METRICS_COLUMNS_TRUE_PEAK)
    assert open(str(tmp_path / "on.csv")).read().splitlines()[1].endswith(",-0.5")


def test_command_line_parses_the_option(capsys):
    from pix2pixhdaudiosr_amd.generate import _parser
    from pix2pixhdaudiosr_amd.generate.report import _print_peaks
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "d"]
    assert _parser().parse_args(base).true_peak is False
    a = _parser().parse_args(base + ["--true_peak", "--clip", "guard", "--ceiling_dbfs", "-1"])
    assert a.true_peak is True and a.clip == "guard" and a.ceiling_dbfs == -1.0
    o = {'peak_dbfs': [-3.0103, -6.0], 'clipped': [0, 0], 'nonfinite': [0, 0], 'gain': 1.0}
    _print_peaks("b.wav", o)
    _print_peaks("b.wav", dict(o, true_peak_dbtp=[0.0002, -5.5]))
    off, on = capsys.readouterr().out.splitlines()
    assert off == "b.wav: peak -3.01 -6.00 dBFS, 0 clipped, 0 non-finite, gain 1.000000"
    assert on == "b.wav: peak -3.01 -6.00 dBFS, true peak +0.00 -5.50 dBTP, 0 clipped, 0 non-finite, gain 1.000000"
