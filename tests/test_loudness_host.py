"""The loudness option without a GPU: the K-weighting coefficients of the library against the restatement and against the values
BS.1770 prints, the restatement against the standard's sine, the gates on hand-made hop energies, and the host side of the
option (plans.check_loudness, the channel weights, the command line, the refusal of a bad rate before a file is opened)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import _loudness_ref as R

HOP = 4800
LEVELS = list(R.GATING_LEVELS)


def test_library_coefficients_match_the_restatement_and_the_printed_values():
    from pix2pixhdaudiosr_amd.generate import loudness_coefficients
    for rate in (8000, 16000, 22050, 44100, 48000, 96000, 192000, 384000):
        got = loudness_coefficients(rate).numpy()
        assert got.dtype == np.float64 and got.shape == (10,)
        assert np.abs(got - R.coefficients(rate)).max() <= 1e-12, rate
    c = loudness_coefficients(48000).numpy()
    seven = np.array([c[0], c[1], c[2], c[3], c[4], c[8], c[9]])
    assert np.abs(seven - np.array(R.BS1770_48K)).max() <= 1e-12
    assert tuple(c[5:8]) == (1.0, -2.0, 1.0)


@pytest.mark.parametrize("rate", [7990, 8001, 44101, 384010, 0, -48000, 48000.5, float('nan'), float('inf')])
def test_library_and_plans_refuse_the_same_rates(rate):
    from pix2pixhdaudiosr_amd.generate import check_loudness, check_loudness_rate, loudness_coefficients
    with pytest.raises(ValueError, match="multiple of 10"):
        loudness_coefficients(rate)
    with pytest.raises(ValueError, match="multiple of 10"):
        check_loudness_rate(rate, "t")
    with pytest.raises(ValueError, match="multiple of 10"):
        check_loudness(-23.0, rate, "t")
    assert check_loudness(None, rate, "t") is None                # off: the rate is nobody's business


def test_full_scale_sine_reads_what_the_standard_says():
    n = 3 * 48000
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(n) / 48000.0)
    mono = R.integrated(x[None], 48000)
    assert abs(mono - (-3.01)) <= 0.01, mono
    both = R.integrated(np.stack([x, x]), 48000)
    assert abs(both - 0.0) <= 0.01, both


def _margin(g):
    """Distance of the nearest block to either threshold."""
    l = g['l'][np.isfinite(g['l'])]
    return min(np.abs(l - (-70.0)).min(), np.abs(l - g['gamma']).min())


def test_gating_on_hand_made_hops_both_gates_act():
    z = R.hops_at_level(LEVELS, HOP)[None]
    g = R.gating(z, 48000)
    assert _margin(g) >= 1.5                                       # no block near a threshold: the figures below are robust
    assert (g['l'] <= -70.0).sum() == 3                           # the absolute gate takes the silent blocks ...
    assert ((g['l'] > -70.0) & (g['l'] <= g['gamma'])).sum() == 6  # ... the relative one the quiet ones
    assert g['kept'] == len(LEVELS) - 3 - 3 - 6
    assert abs(g['I'] - (-21.5197)) <= 1e-4 and abs(g['gamma'] - (-33.4741)) <= 1e-4
    assert abs(g['max'] - (-20.0)) <= 1e-9


def test_gating_with_a_second_weighted_channel():
    z = np.stack([R.hops_at_level(LEVELS, HOP), R.hops_at_level([-26.0] * len(LEVELS), HOP)])
    g = R.gating(z, 48000, (1.0, 1.41))
    assert _margin(g) >= 1.5
    assert abs(g['I'] - (-21.3514)) <= 1e-4
    assert g['kept'] == len(LEVELS) - 3                           # the second channel lifts every block over both gates


def test_gating_edge_cases_and_gain():
    ninf = float('-inf')
    assert R.gating(np.ones((1, 3)), 48000) == {'I': ninf, 'max': ninf, 'gamma': ninf, 'kept': 0, 'l': pytest.approx([]), 'p': pytest.approx([])}
    g = R.gating(np.zeros((2, 9)), 48000)
    assert (g['I'], g['max'], g['gamma'], g['kept']) == (ninf, ninf, ninf, 0)
    z = R.hops_at_level([-30.0] * 8, HOP)[None].copy()
    z[0, 5] = np.nan
    g = R.gating(z, 48000)
    assert math.isnan(g['I']) and g['max'] == pytest.approx(-30.0)
    assert R.gain(-30.0, -23.0, 40.0) == pytest.approx(10.0 ** (7.0 / 20.0))
    assert R.gain(-30.0, -23.0, 3.0) == pytest.approx(10.0 ** (3.0 / 20.0))
    assert R.gain(0.0, -70.0, 40.0) == pytest.approx(0.01)
    assert R.gain(ninf, -23.0, 40.0) == 1.0 and R.gain(float('nan'), -23.0, 40.0) == 1.0 and R.gain(-30.0, None, 40.0) == 1.0


def test_warm_up_restatement_is_the_sequential_one_within_the_documented_bound():
    """The parallel scheme of the kernel, restated on the CPU: 200 ms of zero-state warm-up against the sequential recursion on
    noise with a DC offset, a stretch 60 dB down and a burst -- far inside the 1e-8 the GPU test allows."""
    rng = np.random.default_rng(3)
    rate, hop = 8000, 800
    x = 0.1 * rng.standard_normal((1, 7 * hop + 123)) + 0.05
    x[:, 2 * hop + 17:4 * hop] *= 1e-3
    x[:, 5 * hop:5 * hop + 60] *= 8.0
    x = x.astype(np.float32)
    z, zw = R.hop_energies(x, rate), R.warmup_hop_energies(x, rate)
    assert z.shape == (1, 7) and (zw[:, :3] == z[:, :3]).all()     # the first hops start at sample 0: the same recursion
    # hop by hop: float64 rounding through the double pole, 2^-53 / (1 - r)^2 <= 4e-12, and a truncation of about 1e-17
    assert (np.abs(zw - z) <= 1e-10 * z).all()


def test_check_loudness_and_channel_weights():
    from pix2pixhdaudiosr_amd.generate import LOUDNESS_MAX_GAIN_DB, check_loudness, loudness_channel_weights
    assert LOUDNESS_MAX_GAIN_DB == 40.0
    assert check_loudness(None, 48000, "t") is None
    assert check_loudness('report', 48000, "t") == {'mode': 'report', 'target': None, 'max_gain_db': 40.0}
    assert check_loudness('input', 44100, "t") == {'mode': 'input', 'target': None, 'max_gain_db': 40.0}
    assert check_loudness(-23, 48000, "t") == {'mode': 'target', 'target': -23.0, 'max_gain_db': 40.0}
    assert check_loudness(-70.0, 8000, "t", 6)['max_gain_db'] == 6.0 and check_loudness(0.0, 384000, "t")['target'] == 0.0
    for bad in ('loud', 'Report', 0.1, -70.5, float('nan'), True, [-23], b'input'):
        with pytest.raises(ValueError, match="loudness"):
            check_loudness(bad, 48000, "t")
    for bad in (-1.0, float('inf'), float('nan'), 'x', True):
        with pytest.raises(ValueError, match="loudness_max_gain_db"):
            check_loudness(-23.0, 48000, "t", bad)
    with pytest.raises(ValueError, match="option of loudness"):
        check_loudness(None, 48000, "t", 6.0)
    assert loudness_channel_weights(1) == (1.0,) and loudness_channel_weights(2) == (1.0, 1.0)
    assert loudness_channel_weights(6) == (1.0, 1.0, 1.0, 0.0, 1.41, 1.41)
    assert loudness_channel_weights(5) == (1.0,) * 5 and loudness_channel_weights(8) == (1.0,) * 8
    with pytest.raises(ValueError):
        loudness_channel_weights(0)


def test_command_line_parses_the_option():
    from pix2pixhdaudiosr_amd.generate import _parser
    from pix2pixhdaudiosr_amd.generate.cli import _loudness_args
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "d"]
    ap = _parser()
    a = ap.parse_args(base)
    assert a.loudness is None and a.loudness_max_gain_db is None and _loudness_args(a) == {}
    assert ap.parse_args(base + ["--loudness", "report"]).loudness == 'report'
    assert ap.parse_args(base + ["--loudness", "input"]).loudness == 'input'
    a = ap.parse_args(base + ["--loudness", "-23", "--loudness_max_gain_db", "12"])
    assert a.loudness == -23.0 and a.loudness_max_gain_db == 12.0
    assert _loudness_args(a) == dict(loudness=-23.0, loudness_max_gain_db=12.0)
    assert _loudness_args(a, 44100) == dict(loudness=-23.0, loudness_max_gain_db=12.0)
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--loudness", "loud"])
    with pytest.raises(ValueError, match=r"\[-70, 0\]"):
        _loudness_args(ap.parse_args(base + ["--loudness", "3"]))
    with pytest.raises(ValueError, match="option of --loudness"):
        _loudness_args(ap.parse_args(base + ["--loudness_max_gain_db", "12"]))
    with pytest.raises(ValueError, match="multiple of 10"):        # once the options file has given the rate
        _loudness_args(a, 44101)


def test_a_bad_rate_is_refused_before_a_file_is_opened(tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver.__new__(SuperResolver)                      # no model, no device: the checks come first
    sr.opt = SimpleNamespace(hr_sampling_rate=44101)
    missing = str(tmp_path / "missing.wav")
    for how in ('report', 'input', -23.0):
        with pytest.raises(ValueError, match="multiple of 10"):
            sr.enhance_file(missing, str(tmp_path / "out.wav"), loudness=how)
        with pytest.raises(ValueError, match="multiple of 10"):
            sr.enhance_folder(str(tmp_path / "no_such_folder"), str(tmp_path / "out"), loudness=how)
    with pytest.raises(ValueError, match="loudness must be"):
        sr.enhance_file(missing, None, loudness='normalise')
    assert not (tmp_path / "out.wav").exists() and not (tmp_path / "out").exists()


def test_csv_columns_only_with_the_option(tmp_path):
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_LOUDNESS, METRICS_COLUMNS_PEAKS, metrics_rows, write_metrics_csv
    assert METRICS_COLUMNS_LOUDNESS == ("lufs_in", "lufs_out", "loudness_gain_db")
    rec = {'path': 'a.wav', 'out_frames': 10, 'metrics': [(1.0, 2.0, 3.0, 0, 0, 0, 4.0)] * 2,
           'output': {'peak_dbfs': [-1.0, -2.0], 'clipped': [0, 1], 'gain': 1.0},
           'loudness': {'input': -30.0, 'measured': -20.0, 'gain_db': -3.0, 'output': -23.0, 'momentary_max': -21.0, 'target': -23.0}}
    assert metrics_rows([rec])[0] == ('a.wav', 0, 10, 1.0, 2.0, 3.0, 4.0)
    rows = metrics_rows([rec], False, True, True)
    assert rows[1] == ('a.wav', 1, 10, 1.0, 2.0, 3.0, 4.0, -2.0, 1, 1.0, -30.0, -23.0, -3.0) and rows[-1][-3:] == (-30.0, -23.0, -3.0)
    write_metrics_csv(str(tmp_path / "off.csv"), [rec])
    write_metrics_csv(str(tmp_path / "on.csv"), [rec], False, True, True)
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(METRICS_COLUMNS)
    assert open(str(tmp_path / "on.csv")).readline().strip() == ",".join(METRICS_COLUMNS + METRICS_COLUMNS_PEAKS + METRICS_COLUMNS_LOUDNESS)
