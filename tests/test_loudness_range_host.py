"""The loudness-range option without a GPU: the restatement of tests/_loudness_range_ref.py on the four minimum-requirement
sequences of EBU Tech 3342, the integer ranks, the shortest clips, the option checks of plans, resolver and command line (all
before anything is loaded) and the CSV columns."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import _loudness_range_ref as RR
import _loudness_ref as R
from pix2pixhdaudiosr_amd.generate.ops import LOUDNESS_SHORT_TERM_HOPS

assert RR.BLOCK_HOPS == LOUDNESS_SHORT_TERM_HOPS                   # the restatement and the tensor functions cut the same blocks

# EBU Tech 3342, table 1: the levels of the test sequences (here 20 s each, both channels alike) and the range a meter must show
TECH_3342 = (((-20.0, -30.0), 10.0, 371), ((-20.0, -15.0), 5.0, 371), ((-40.0, -20.0), 20.0, 371),
             ((-50.0, -35.0, -20.0, -35.0, -50.0), 15.0, 627))


def _sequence(levels, hops_per_level=200, hop=4800):
    row = R.hops_at_level([l for l in levels for _ in range(hops_per_level)], hop)
    return np.stack([row, row])


@pytest.mark.parametrize("levels,want,n", TECH_3342)
def test_tech_3342_minimum_requirements(levels, want, n):
    """Each sequence within the standard's +-1 LU; the gates keep the number of blocks a hand count gives, and no block is
    anywhere near a threshold, so the figure does not hang on a rounding."""
    m = RR.measure(_sequence(levels), 48000, (1.0, 1.0))
    print("levels %s: LRA %.6f LU (%.4f .. %.4f LUFS), threshold %.4f, n %d, margin %.4f, short-term max %.4f"
          % (levels, m['lra'], m['low'], m['high'], m['threshold'], m['n'], m['margin'], m['short_term_max']))
    assert abs(m['lra'] - want) <= 1.0
    assert m['n'] == n and m['margin'] > 0.01                      # (the nearest is 7.9 % off; rounding moves a power by 1e-15)
    # two channels at the level: 3.01 dB over one
    assert abs(m['short_term_max'] - (max(levels) + 10.0 * math.log10(2.0))) <= 1e-9
    # a gain moves the levels and leaves the range
    g = RR.measure(_sequence(levels), 48000, (1.0, 1.0), gain=np.float32(0.5))
    assert abs(g['lra'] - m['lra']) <= 1e-9 and abs(g['high'] - (m['high'] + 20.0 * math.log10(0.5))) <= 1e-9 and g['n'] == m['n']


def test_integer_ranks():
    """round((n - 1) PRC / 100 + 1) of the Tech 3342 reference code, zero-based, in integers."""
    want = {1: (0, 0), 2: (0, 1), 3: (0, 2), 10: (1, 9), 11: (1, 10), 20: (2, 18), 21: (2, 19)}
    for n, k in want.items():
        assert RR.ranks(n) == k, n
    for n in range(1, 2000):                                       # inside the set, ordered, and the float formula where it is exact
        lo, hi = RR.ranks(n)
        assert 0 <= lo <= hi < n
        assert lo == math.floor((n - 1) * 0.1 + 0.5 + 1e-9) and hi == math.floor((n - 1) * 0.95 + 0.5 + 1e-9)


def test_the_shortest_clips():
    ninf = float('-inf')
    z = R.hops_at_level([-23.0] * 30, 4800)[None]
    m = RR.measure(z[:, :29], 48000)                               # 2.9 s: no block
    assert RR.block_powers(z[:, :LOUDNESS_SHORT_TERM_HOPS - 1], 48000).shape == (0,)
    assert (m['lra'], m['low'], m['high'], m['n'], m['short_term_max'], m['threshold']) == (0.0, ninf, ninf, 0, ninf, ninf)
    m = RR.measure(z, 48000)                                       # 3 s: one block, both ranks select it
    assert m['n'] == 1 and m['lra'] == 0.0 and m['q_lo'] == m['q_hi'] and abs(m['low'] - (-23.0)) <= 1e-9
    assert abs(m['short_term_max'] - (-23.0)) <= 1e-9 and abs(m['threshold'] - (-43.0)) <= 1e-9
    m = RR.measure(np.zeros((2, 100)), 48000)                      # silence: nothing passes
    assert (m['lra'], m['low'], m['high'], m['n'], m['short_term_max']) == (0.0, ninf, ninf, 0, ninf)
    # a block at a threshold is out: equality gates
    m = RR.loudness_range(np.array([RR.P_ABS, np.nextafter(RR.P_ABS, 1.0)]))
    assert m['n'] == 1 and m['q_lo'] == np.nextafter(RR.P_ABS, 1.0)
    # a NaN block shows in the range and the levels, not in the short-term maximum
    m = RR.loudness_range(np.array([1e-3, float('nan'), 2e-3]))
    assert math.isnan(m['lra']) and math.isnan(m['low']) and math.isnan(m['high']) and abs(m['short_term_max'] - R._lufs(2e-3)) <= 1e-12


def test_check_loudness_takes_the_option():
    from pix2pixhdaudiosr_amd.generate import check_loudness
    assert check_loudness('report', 48000, "t", None, False) == {'mode': 'report', 'target': None, 'max_gain_db': 40.0}
    assert check_loudness('report', 48000, "t", None, True) == {'mode': 'report', 'target': None, 'max_gain_db': 40.0, 'range': True}
    assert check_loudness(-23, 48000, "t", 6.0, loudness_range=True) == {'mode': 'target', 'target': -23.0, 'max_gain_db': 6.0, 'range': True}
    assert check_loudness(None, 48000, "t", None, False) is None
    with pytest.raises(ValueError, match="loudness_range is an option of loudness"):
        check_loudness(None, 48000, "t", None, True)
    for bad in (1, 'yes', None):
        with pytest.raises(ValueError, match="loudness_range must be a bool"):
            check_loudness('report', 48000, "t", None, bad)


def test_the_resolver_refuses_before_a_file_is_opened(tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver.__new__(SuperResolver)                      # no model, no device: the checks come first
    sr.opt = SimpleNamespace(hr_sampling_rate=48000)
    missing = str(tmp_path / "missing.wav")
    with pytest.raises(ValueError, match="loudness_range is an option of loudness"):
        sr.enhance_file(missing, str(tmp_path / "out.wav"), loudness_range=True)
    with pytest.raises(ValueError, match="loudness_range is an option of loudness"):
        sr.enhance_folder(str(tmp_path / "no_such_folder"), str(tmp_path / "out"), loudness_range=True)
    sr.opt = SimpleNamespace(hr_sampling_rate=44101)
    with pytest.raises(ValueError, match="multiple of 10"):
        sr.enhance_file(missing, str(tmp_path / "out.wav"), loudness='report', loudness_range=True)
    assert not (tmp_path / "out.wav").exists() and not (tmp_path / "out").exists()


def test_command_line_parses_the_option(tmp_path, capsys):
    from pix2pixhdaudiosr_amd import generate as G
    from pix2pixhdaudiosr_amd.generate.cli import _loudness_args
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "d"]
    ap = G._parser()
    assert ap.parse_args(base).loudness_range is False
    a = ap.parse_args(base + ["--loudness", "report", "--loudness_range"])
    assert a.loudness_range is True
    assert _loudness_args(a) == dict(loudness='report', loudness_max_gain_db=None, loudness_range=True)
    assert _loudness_args(ap.parse_args(base + ["--loudness", "report"])) == dict(loudness='report', loudness_max_gain_db=None)
    with pytest.raises(ValueError, match="--loudness_range is an option of --loudness"):
        _loudness_args(ap.parse_args(base + ["--loudness_range"]))
    with pytest.raises(SystemExit):                                # a flag: it takes no value
        ap.parse_args(base + ["--loudness_range=1"])
    # main(): the parser's error, before the options file or a checkpoint is looked for (neither exists)
    src = tmp_path / "in.wav"
    src.write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        G.main(["--input", str(src), "--output", str(tmp_path / "out.wav"), "--load_pretrain", str(tmp_path / "none"), "--loudness_range"])
    assert e.value.code == 2 and "--loudness_range is an option of --loudness" in capsys.readouterr().err
    assert not (tmp_path / "out.wav").exists()


def test_csv_columns_and_the_mean_row(tmp_path):
    from pix2pixhdaudiosr_amd.generate import (METRICS_COLUMNS, METRICS_COLUMNS_LOUDNESS, METRICS_COLUMNS_LOUDNESS_RANGE, METRICS_COLUMNS_TRUE_PEAK,
                                               metrics_rows, write_metrics_csv)
    assert METRICS_COLUMNS_LOUDNESS_RANGE == ("lra_in", "lra_out", "short_term_max")

    def rec(path, channels, lra_in, lra_out, top):
        return {'path': path, 'out_frames': 10, 'metrics': [(1.0, 2.0, 3.0, 0, 0, 0, 4.0)] * channels,
                'output': {'peak_dbfs': [-1.0] * channels, 'clipped': [0] * channels, 'gain': 1.0, 'true_peak_dbtp': [-0.5] * channels},
                'loudness': {'input': -30.0, 'measured': -20.0, 'gain_db': -3.0, 'output': -23.0, 'momentary_max': -21.0, 'target': -23.0,
                             'range': {'input': lra_in, 'output': lra_out, 'low': -31.0, 'high': -23.0, 'threshold': -45.0, 'blocks': 7,
                                       'short_term_max': top}}}
    recs = [rec('a.wav', 2, 7.5, 8.0, -19.0), rec('b.wav', 1, 1.5, 2.0, -22.0)]
    rows = metrics_rows(recs, False, False, True, loudness_range=True)
    assert rows[0] == ('a.wav', 0, 10, 1.0, 2.0, 3.0, 4.0, -30.0, -23.0, -3.0, 7.5, 8.0, -19.0)
    assert rows[2] == ('b.wav', 0, 10, 1.0, 2.0, 3.0, 4.0, -30.0, -23.0, -3.0, 1.5, 2.0, -22.0)
    assert rows[-1][0] == "mean" and rows[-1][-3:] == (5.5, 6.0, -20.0) and len(rows) == 4      # plain means over the three rows
    # behind the loudness columns, in front of the true peak's
    rows = metrics_rows(recs, False, False, True, True, loudness_range=True)
    assert rows[0][-4:] == (7.5, 8.0, -19.0, -0.5)
    # without the option: the rows of before
    assert metrics_rows(recs, False, False, True)[0] == ('a.wav', 0, 10, 1.0, 2.0, 3.0, 4.0, -30.0, -23.0, -3.0)
    write_metrics_csv(str(tmp_path / "off.csv"), recs, False, False, True)
    write_metrics_csv(str(tmp_path / "on.csv"), recs, False, False, True, True, loudness_range=True)
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(METRICS_COLUMNS + METRICS_COLUMNS_LOUDNESS)
    assert open(str(tmp_path / "on.csv")).readline().strip() == \
        ",".join(METRICS_COLUMNS + METRICS_COLUMNS_LOUDNESS + METRICS_COLUMNS_LOUDNESS_RANGE + METRICS_COLUMNS_TRUE_PEAK)
    # a clip under 3 s: 0.0 and -inf go through the table as they are
    short = rec('c.wav', 1, 0.0, 0.0, float('-inf'))
    assert metrics_rows([short], False, False, True, loudness_range=True)[-1][-3:] == (0.0, 0.0, float('-inf'))


def test_the_printed_line(capsys):
    from pix2pixhdaudiosr_amd.generate.report import _print_loudness_range
    _print_loudness_range("out.wav", {'input': 7.314, 'output': 8.02, 'low': -31.2, 'high': -23.18, 'threshold': -44.0, 'blocks': 120,
                                      'short_term_max': -19.87})
    _print_loudness_range("s.wav", {'input': 0.0, 'output': 0.0, 'low': float('-inf'), 'high': float('-inf'), 'threshold': float('-inf'),
                                    'blocks': 0, 'short_term_max': float('-inf')})
    assert capsys.readouterr().out.splitlines() == [
        "out.wav: loudness range input 7.31 LU, output 8.02 LU (-31.20 .. -23.18 LUFS), short-term max -19.87 LUFS",
        "s.wav: loudness range input 0.00 LU, output 0.00 LU (-inf .. -inf LUFS), short-term max -inf LUFS"]
