"""Host side of the active speech level (ITU-T P.56 method B; csrc/speechlevel.hip, include/p2phd.h "Active speech level"): the
constants the library fills against Python's, the contract's chunked order against the plain sequential recursion with per-threshold
hangover counters (tests/_speechlevel_ref.py), known answers, the exact scaling by a power of two, the edge cases of the decision,
the file's figure, and every refusal of check_speech_level and of the command line.  No GPU."""
import math
import os
import struct

import numpy as np
import pytest

import _speechlevel_ref as R


def _consts(rate):
    """The constants the restatement is fed: the library entry's own, as on the device (not Python's exp)."""
    from pix2pixhdaudiosr_amd.generate import speech_level_consts
    c, I = speech_level_consts(rate)
    return tuple(c[:4].tolist()), I


def _ulps(a, b):
    ia, ib = (struct.unpack("<q", struct.pack("<d", v))[0] for v in (a, b))
    return abs(ia - ib)


@pytest.mark.parametrize("rate,hang", [(8000, 1600), (44100, 8820), (48000, 9600), (192000, 38400)])
def test_constants_entry_against_python(rate, hang):
    from pix2pixhdaudiosr_amd.generate import speech_level_consts
    c, I = speech_level_consts(rate)
    (g, h, gL, hL), I_py = R.consts(rate)
    assert I == I_py == hang == math.ceil(rate / 5)
    c = c.tolist()
    assert _ulps(c[0], g) <= 1
    # what follows from g is formed from the entry's own g, exactly as the contract says
    g0 = c[0]
    gl = g0
    for _ in range(8):
        gl = gl * gl
    assert c[1] == 1.0 - g0 and c[2] == gl and c[3] == (256.0 * c[1]) * gl
    assert _ulps(c[1], h) <= 1 << 10                              # (1 - g cancels: an ulp of g is many of h)
    assert c[4:] == [15.9, 2.0 ** -15, 256.0, float(hang)]


def test_constants_entry_refuses_bad_rates():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import speech_level_consts
    for rate in (7999, 192001, 0, -8000, 44100.5, True, "8000", None):
        with pytest.raises(ValueError, match="whole rate in"):
            speech_level_consts(rate)
    import ctypes
    out = (ctypes.c_double * 8)()
    hang = ctypes.c_int32(0)
    L = _lib.lib()
    assert L.p2phd_speechlevel_consts_fill(7999, ctypes.cast(out, ctypes.c_void_p), ctypes.byref(hang)) != 0
    assert b"rate must be in [8000, 192000]" in L.p2phd_last_error()
    assert L.p2phd_speechlevel_consts_fill(8000, None, ctypes.byref(hang)) != 0 and b"null" in L.p2phd_last_error()
    assert L.p2phd_speechlevel_tile_len() == 16384
    assert L.p2phd_speechlevel_workspace_bytes(0, 1) == 0 and L.p2phd_speechlevel_workspace_bytes(257, 3) == 3 * 2 * 24
    assert L.p2phd_speechlevel_workspace_bytes(256, 65) == 0 and L.p2phd_speechlevel_workspace_bytes(-1, 1) == 0


@pytest.mark.parametrize("rate,seconds,seed", [(8000, 4, 1), (48000, 3, 1)])
def test_chunked_order_against_the_sequential_form(rate, seconds, seed):
    """All fifteen counts equal and the levels within 1e-9 dB (3e-14 observed).  A fixture on which a comparison sits within
    rounding of a threshold would be replaced, not tolerated."""
    x = R.modulated_noise(seconds * rate, rate, seed)
    k, I = _consts(rate)
    s, c = R.sequential_row(x, rate, k, I), R.chunked_row(x, k, I)
    print("a", s['a'], "levels", s['active'], c['active'], "diff", s['active'] - c['active'])
    assert s['a'] == c['a'] and s['a'][0] > s['a'][8] > 0
    assert 0 < s['bracket'] < 14 and s['bracket'] == c['bracket']
    for key in ('active', 'long_term'):
        assert abs(s[key] - c[key]) <= 1e-9
    assert abs(s['activity'] - c['activity']) <= 1e-9


def test_known_answers_at_8_khz():
    """A 997 Hz sine of amplitude 0.25 over 4 s, whole and gated 1 s on / 1 s off (the on-time plus 200 ms of hangover plus the
    envelope's decay per burst)."""
    rate, n = 8000, 32000
    k, I = _consts(rate)
    tone = R.gated_tone(n, rate, on_s=1e9)
    for x, want in ((tone, (-15.0515, -15.026, 0.994)), (R.gated_tone(n, rate), (-18.062, -16.114, 0.6386))):
        for r in (R.sequential_row(x, rate, k, I), R.chunked_row(x, k, I)):
            print(r['long_term'], r['active'], r['activity'])
            assert abs(r['long_term'] - want[0]) <= 0.01 and abs(r['active'] - want[1]) <= 0.01 and abs(r['activity'] - want[2]) <= 0.001
            assert abs(r['active'] - (r['long_term'] - 10.0 * math.log10(r['activity']))) <= 1e-9
    # units: a full-scale sine reads -3.01 dBov long-term
    full = R.chunked_row(R.gated_tone(n, rate, amp=1.0, on_s=1e9), k, I)
    assert abs(full['long_term'] - (-3.0103)) <= 0.001


def test_scaling_by_a_power_of_two_is_exact():
    """x * 2^-3: every q is the old one times 2^-3 bit for bit, so the counts move three thresholds, a'_j == a_{j+3}, and the level
    moves by 20 log10(8) = 60 log10(2) dB (the amplitude is scaled, so the power moves by 2^-6)."""
    rate = 8000
    k, I = _consts(rate)
    x = R.modulated_noise(4 * rate, rate, 3)
    a, b = R.chunked_row(x, k, I), R.chunked_row(x * np.float32(0.125), k, I)
    assert a['a'][3:] == b['a'][:12] and b['a'][12:] == [0, 0, 0] and a['a'][3] > 0
    assert b['sq'] == a['sq'] / 64.0
    assert abs((a['active'] - b['active']) - 60.0 * math.log10(2.0)) <= 1e-9
    assert abs(a['activity'] - b['activity']) <= 1e-12


def test_silence_nan_and_inf():
    rate = 8000
    k, I = _consts(rate)
    z = R.chunked_row(np.zeros(3000, np.float32), k, I)
    assert z['a'] == [0] * 15 and z['active'] == float('-inf') and z['activity'] == 0.0 and z['long_term'] == float('-inf') and z['bracket'] == -1
    assert R.gain_of(-26.0, z['active']) == np.float32(1.0)
    x = R.modulated_noise(3000, rate, 5)
    bad = x.copy(); bad[1500] = np.nan
    r = R.chunked_row(bad, k, I)
    good = R.chunked_row(x, k, I)
    # the NaN reaches every q behind it: the index is 0 from there on, the hangover runs out, the energy is NaN
    assert (r['m'][:1500] == good['m'][:1500]).all() and (r['m'][1500:] == 0).all()
    assert math.isnan(r['sq']) and not math.isfinite(r['active']) and R.gain_of(-26.0, r['active']) == np.float32(1.0)
    inf = x.copy(); inf[1500] = np.inf
    r = R.chunked_row(inf, k, I)
    assert (r['m'][1500:] == 15).all() and r['sq'] == float('inf') and not math.isfinite(r['active'])
    assert R.gain_of(-26.0, r['active']) == np.float32(1.0)
    s = R.sequential_row(inf, rate, k, I)
    assert s['a'] == r['a']


def test_short_clips():
    rate = 8000
    k, I = _consts(rate)
    x = R.modulated_noise(700, rate, 7, depth_hz=4.0, level=0.3)      # shorter than I: the hangover never runs out once it starts
    s, c = R.sequential_row(x, rate, k, I), R.chunked_row(x, k, I)
    assert len(x) < I and s['a'] == c['a'] and abs(s['active'] - c['active']) <= 1e-9
    first = int(np.argmax(c['m'] > 0))
    assert c['a'][0] == len(x) - first > 0
    one = R.chunked_row(np.array([0.5], np.float32), k, I)
    assert one['a'] == R.sequential_row(np.array([0.5], np.float32), rate, k, I)['a']
    # q_0 = h (h 0.5): far under 2^-15 at 8 kHz, so no activity
    assert one['a'][0] == 0 and one['active'] == float('-inf') and abs(one['long_term'] - 20 * math.log10(0.5)) <= 1e-12
    assert R.trailing_max(np.array([3], np.uint8), I).tolist() == [3]
    assert R.trailing_max(np.array([0, 5, 0, 0, 0, 1], np.uint8), 2).tolist() == [0, 5, 5, 5, 0, 1]


def test_file_figure_over_channels():
    rate = 8000
    k, I = _consts(rate)
    x = R.modulated_noise(2 * rate, rate, 11)
    quiet, silent = x * np.float32(0.25), np.zeros_like(x)
    rows, fig, ch = R.chunked(np.stack([quiet, x]), k, I)
    assert ch == 1 and fig is rows[1] and rows[1]['active'] > rows[0]['active']
    rows, fig, ch = R.chunked(np.stack([x, silent, x]), k, I)         # a tie: the lowest index; a silent channel never wins
    assert ch == 0 and rows[1]['active'] == float('-inf') and rows[0]['active'] == rows[2]['active']
    rows, fig, ch = R.chunked(np.stack([silent, quiet, x]), k, I)
    assert ch == 2
    rows, fig, ch = R.chunked(np.stack([silent, silent]), k, I)
    assert ch == 0 and fig['active'] == float('-inf') and R.gain_of(-26.0, fig['active']) == np.float32(1.0)
    # the gain: towards the target, clamped either way
    assert R.gain_of(-26.0, -30.0) == np.float32(10.0 ** (4.0 / 20.0)) and R.gain_of(-26.0, -30.0, 1.0) == np.float32(10.0 ** (1.0 / 20.0))
    assert R.gain_of(-26.0, -20.0, 1.0) == np.float32(10.0 ** (-1.0 / 20.0)) and R.gain_of(None, -20.0) == np.float32(1.0)


def test_check_speech_level():
    from pix2pixhdaudiosr_amd.generate import SPEECH_LEVEL_DEFAULTS, check_speech_level, check_speech_level_rate
    assert SPEECH_LEVEL_DEFAULTS == {'max_gain_db': 40.0}
    assert check_speech_level(None) is None
    assert check_speech_level('report') == {'mode': 'report', 'target': None, 'max_gain_db': 40.0}
    assert check_speech_level('input', max_gain_db=6) == {'mode': 'input', 'target': None, 'max_gain_db': 6.0}
    assert check_speech_level(-26) == {'mode': 'target', 'target': -26.0, 'max_gain_db': 40.0}
    assert check_speech_level(0.0, max_gain_db=120.0)['target'] == 0.0 and check_speech_level(-70, max_gain_db=0)['max_gain_db'] == 0.0
    for bad in ('loud', 'target', '', 1, 0.5, -70.5, float('nan'), float('inf'), float('-inf'), True, [-26]):
        with pytest.raises(ValueError, match="speech_level"):
            check_speech_level(bad, "t")
    with pytest.raises(ValueError, match="speech_level_max_gain_db is an option of speech_level"):
        check_speech_level(None, "t", 6.0)
    for bad in (-1, 120.5, float('nan'), float('inf'), True, "6"):
        with pytest.raises(ValueError, match=r"speech_level_max_gain_db must be in \[0, 120\]"):
            check_speech_level(-26, "t", bad)
    for loud in ('report', 'input', -23.0):
        with pytest.raises(ValueError, match="two claims on the one gain"):
            check_speech_level('report', "t", None, loud)
    for rate in (7999, 192001, 22050.5, True, None):
        with pytest.raises(ValueError, match=r"whole rate in \[8000, 192000\]"):
            check_speech_level_rate(rate, "t")
    assert check_speech_level_rate(44100.0, "t") == 44100


def test_cli_options_and_refusals(capsys):
    from pix2pixhdaudiosr_amd.generate import _parser, main
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]
    a = _parser().parse_args(base)
    assert (a.speech_level, a.speech_level_max_gain_db) == (None, None)
    b = _parser().parse_args(base + ["--speech_level", "-26", "--speech_level_max_gain_db", "12"])
    assert (b.speech_level, b.speech_level_max_gain_db) == (-26.0, 12.0)
    assert _parser().parse_args(base + ["--speech_level", "input"]).speech_level == 'input'
    for extra, word in ((["--speech_level", "loud"], "expected report, input or a target in dBov"),
                        (["--speech_level", "3"], "finite level in [-70, 0] dBov"),
                        (["--speech_level", "-71"], "finite level in [-70, 0] dBov"),
                        (["--speech_level", "nan"], "finite level in [-70, 0] dBov"),
                        (["--speech_level_max_gain_db", "6"], "option of speech_level"),
                        (["--speech_level", "-26", "--speech_level_max_gain_db", "121"], "must be in [0, 120]"),
                        (["--speech_level", "-26", "--loudness", "-23"], "two claims on the one gain"),
                        (["--speech_level", "report", "--loudness", "report", "--loudness_range"], "two claims on the one gain"),
                        (["--speech_level", "report", "--loudness_scope", "folder"], "option of --loudness"),
                        (["--speech_level", "report", "--loudness_range"], "option of --loudness"),
                        (["--speech_level", "report", "--output_rate", "384000"], "whole rate in [8000, 192000]")):
        with pytest.raises(SystemExit) as e:                      # ("ck" does not exist: loading anything would raise another error)
            main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_resolver_refuses_before_a_file_is_opened(tmp_path):
    """enhance_file / enhance_folder validate the option in front of everything else: a model rate outside 8000 .. 192000, the
    loudness option beside it, a bad value -- each a ValueError while the input does not even exist."""
    from types import SimpleNamespace
    from pix2pixhdaudiosr_amd.generate import SuperResolver

    def resolver(hr_rate):
        sr = SuperResolver.__new__(SuperResolver)                  # (no model: the options are validated from the rates alone)
        sr.opt = SimpleNamespace(hr_sampling_rate=hr_rate, lr_sampling_rate=4000)
        return sr

    missing, out = str(tmp_path / "missing.wav"), str(tmp_path / "out")
    for rate in (4000, 6000, 384000):
        for call in (lambda sr: sr.enhance_file(missing, None, speech_level='report'),
                     lambda sr: sr.enhance_folder(str(tmp_path / "nowhere"), out, speech_level=-26.0)):
            with pytest.raises(ValueError, match=r"whole rate in \[8000, 192000\]"):
                call(resolver(rate))
    ok = resolver(48000)
    with pytest.raises(ValueError, match="two claims on the one gain"):
        ok.enhance_file(missing, None, speech_level=-26.0, loudness=-23.0)
    with pytest.raises(ValueError, match="speech_level must be"):
        ok.enhance_folder(str(tmp_path / "nowhere"), out, speech_level='loud')
    with pytest.raises(ValueError, match="option of speech_level"):
        ok.enhance_file(missing, None, speech_level_max_gain_db=3.0)
    assert not os.path.exists(out)


def test_report_line_and_columns(tmp_path, capsys):
    import csv
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_SPEECH_LEVEL, write_metrics_csv
    from pix2pixhdaudiosr_amd.generate.report import _print_speech_level
    assert METRICS_COLUMNS_SPEECH_LEVEL == ("asl_in", "asl_out", "activity_out")
    s = {'input': -27.31, 'measured': -29.8, 'gain_db': 3.8, 'output': -26.0, 'target': -26.0, 'long_term': -28.1, 'activity': 0.612,
         'activity_input': 0.58, 'channels': [{'active': -26.0, 'long_term': -28.1, 'activity': 0.612}]}
    _print_speech_level("out.wav", s)
    assert capsys.readouterr().out == ("out.wav: speech level input -27.31 dBov (activity 58.0 %), measured -29.80 dBov (activity 61.2 %), "
                                       "gain +3.80 dB -> -26.00 dBov\n")
    rec = {'path': 'a.wav', 'out_frames': 10, 'metrics': [(1.0, 2.0, 3.0, 0, 0, 0, 4.0)], 'speech_level': s}
    write_metrics_csv(str(tmp_path / "on.csv"), [rec], speech_level=True)
    write_metrics_csv(str(tmp_path / "off.csv"), [rec])
    on, off = (list(csv.reader(open(str(tmp_path / n)))) for n in ("on.csv", "off.csv"))
    assert tuple(off[0]) == METRICS_COLUMNS and tuple(on[0]) == METRICS_COLUMNS + METRICS_COLUMNS_SPEECH_LEVEL
    assert [float(v) for v in on[1][-3:]] == [-27.31, -26.0, 0.612] and on[1][:7] == off[1] and len(on) == 3
