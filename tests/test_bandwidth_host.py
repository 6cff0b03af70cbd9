"""The bandwidth report and crossover_hz='auto' without a GPU: the restatement (tests/_bandwidth_ref.py) on brick-wall noise, the
plans and their refusals, the plumbing of the option through enhance_file / enhance_folder on a stub, the printed lines and the
columns of --metrics_csv -- and that nothing moves without the option."""
import csv
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _bandwidth_ref as BR

BASE = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [2048, 512])
def test_brickwall_noise_reads_within_eight_bins(n_fft):
    """2 s of white noise at 48 kHz made brick-wall at fc: at -60 dB with bands of 8 bins the band edge reads fc's bin or up to 8 bins
    more -- the excess is the Hann window's side lobes."""
    rate, plan = 48000, dict(n_fft=n_fft, hop=n_fft // 2, band_bins=8, threshold_db=60.0)
    for fc in (3400, 4000, 8000, 12000, 20000):
        for seed in (1, 2):
            x = BR.brickwall_noise(2 * rate, rate, fc, seed)
            hz, res = BR.bandwidth_ref(x, rate, plan)
            excess = res[0] - fc * n_fft / rate
            print(f"n_fft {n_fft} fc {fc} seed {seed}: k_top {int(res[0])}, {excess:+.2f} bins")
            assert 0.0 <= excess <= 8.0, (n_fft, fc, seed, res.tolist())
            assert hz == res[0] * rate / n_fft and res[1] == int(res[0]) // 8 and res[3] == res[2] * 1e-6


def test_short_clip_and_silence_read_zero():
    assert BR.bandwidth_ref(np.random.default_rng(0).standard_normal(2047), 48000)[0] == 0.0
    hz, res = BR.bandwidth_ref(np.zeros((2, 9000)), 48000)
    assert hz == 0.0 and res.tolist() == [-1.0, -1.0, 0.0, 0.0]
    assert BR.frames_ref(2047, 2048, 1024) == 0 and BR.frames_ref(2048, 2048, 1024) == 1 and BR.frames_ref(3071, 2048, 1024) == 1
    assert BR.frames_ref(3072, 2048, 1024) == 2


def test_decision_on_hand_made_spectra():
    K = 33
    s = np.full((1, K), 1e-9)
    s[0, :12] = 1.0
    s[0, 12] = 0.5                                                 # a lone bin above thr in a band whose mean is above thr
    res = BR.decide_ref(s, 1, 4, 1e-6)[0]
    assert res.tolist() == [12.0, 3.0, 1.0, 1e-6]
    # a band whose level equals thr exactly does not pass: band 3 = {1e-6} * 4 has the mean 1e-6 = thr
    t = np.zeros((1, K))
    t[0, :4], t[0, 12:16] = 1.0, 1e-6
    assert 1.0 * 1e-6 == 1e-6 and BR.decide_ref(t, 1, 4, 1e-6)[0].tolist() == [3.0, 0.0, 1.0, 1e-6]
    t[0, 12] = 1.5e-6                                              # now the mean is above it, and bin 12 alone is
    assert BR.decide_ref(t, 1, 4, 1e-6)[0][:2].tolist() == [12.0, 3.0]
    # rows of a group are added; NaN never wins and fails; all NaN, all zero
    two = np.stack([s[0], s[0]])
    assert BR.decide_ref(two, 2, 4, 1e-6)[0].tolist() == [12.0, 3.0, 2.0, 2e-6]
    n = s.copy()
    n[0, 20] = np.nan
    assert BR.decide_ref(n, 1, 4, 1e-6)[0].tolist() == [12.0, 3.0, 1.0, 1e-6]
    assert BR.decide_ref(np.full((1, K), np.nan), 1, 4, 1e-6)[0].tolist() == [-1.0, -1.0, 0.0, 0.0]
    # the last band is partial (one bin) and may be the top band
    s[0, 32] = 1.0
    assert BR.decide_ref(s, 1, 4, 1e-6)[0][:2].tolist() == [32.0, 8.0]


# ------------------------------------------------------------------------------------------
# plans
# ------------------------------------------------------------------------------------------
def test_check_bandwidth_and_its_error_texts():
    from pix2pixhdaudiosr_amd.generate import BANDWIDTH_DEFAULTS, bandwidth_rel, check_bandwidth
    assert BANDWIDTH_DEFAULTS == {'n_fft': 2048, 'hop': 1024, 'band_bins': 8, 'threshold_db': 60.0} == BR.DEFAULTS
    assert check_bandwidth() is None and check_bandwidth(False, None) is None
    assert check_bandwidth(True) == BANDWIDTH_DEFAULTS and check_bandwidth(True, {}) == BANDWIDTH_DEFAULTS
    assert check_bandwidth(True, {'n_fft': 512, 'threshold_db': 40, 'band_bins': None}) == {'n_fft': 512, 'hop': 256, 'band_bins': 8, 'threshold_db': 40.0}
    assert check_bandwidth(True, {'hop': 100, 'band_bins': 1025, 'threshold_db': 200.0})['hop'] == 100
    assert bandwidth_rel(60.0) == 1e-6 == BR.rel_of(60.0) and bandwidth_rel(33.0) == BR.rel_of(33.0)
    for kw, word in ((dict(bandwidth=1), "bandwidth must be a bool"), (dict(bandwidth=False, opts={'n_fft': 512}), "options of bandwidth=True"),
                     (dict(bandwidth=True, opts=[1]), "None or a dict"), (dict(bandwidth=True, opts={'nfft': 512}), r"unknown bandwidth_opts \['nfft'\]"),
                     (dict(bandwidth=True, opts={'n_fft': 1000}), "n_fft must be a power of two"), (dict(bandwidth=True, opts={'n_fft': 4096}), "n_fft must be"),
                     (dict(bandwidth=True, opts={'n_fft': 32}), "n_fft must be"), (dict(bandwidth=True, opts={'n_fft': 512.0}), "n_fft must be"),
                     (dict(bandwidth=True, opts={'hop': 0}), "hop must be"), (dict(bandwidth=True, opts={'hop': 2049}), "hop must be"),
                     (dict(bandwidth=True, opts={'band_bins': 0}), "band_bins must be"), (dict(bandwidth=True, opts={'band_bins': 1026}), "band_bins must be"),
                     (dict(bandwidth=True, opts={'n_fft': 64, 'band_bins': 34}), r"n_fft / 2 \+ 1 = 33"),
                     (dict(bandwidth=True, opts={'threshold_db': 0.0}), r"threshold_db must lie in \(0, 200\]"),
                     (dict(bandwidth=True, opts={'threshold_db': 200.5}), "threshold_db must lie"), (dict(bandwidth=True, opts={'threshold_db': True}), "threshold_db"),
                     (dict(bandwidth=True, opts={'threshold_db': float('nan')}), "threshold_db"),
                     (dict(bandwidth=True, loudness_scope='folder'), "not built for loudness_scope='folder'")):
        with pytest.raises(ValueError, match=word):
            check_bandwidth(who="t", **kw)


def test_auto_crossover_plan():
    from pix2pixhdaudiosr_amd.generate import (CROSSOVER_MAX_TAPS, check_crossover, crossover_auto_floor_hz, crossover_auto_plan, crossover_plan,
                                               crossover_width_hz)
    for hr, lr in ((48000, 8000), (48000, 16000), (44100, 11025), (16000, 8000)):
        default = crossover_plan(hr, lr)
        for edge in (lr / 2.0, lr / 2.0 + 1.0, 1e9):               # a full-band edge, or one beyond it: the default tuple exactly
            assert crossover_auto_plan(hr, lr, edge) == (default, lr / 2.0)
        assert check_crossover('input', 'auto', None, hr, lr) == default
    # a telephone-band input in an 8 kHz low rate: the crossover at 0.95 of the edge, the transition band ending at the edge
    (taps, cutoff, beta), edge = crossover_auto_plan(48000, 8000, 3400.0)
    assert edge == 3400.0 and cutoff * 48000 == pytest.approx(0.95 * 3400.0, rel=1e-12) and beta == 8.96
    assert cutoff * 48000 + crossover_width_hz(48000, taps) / 2.0 <= 3400.0 < cutoff * 48000 + crossover_width_hz(48000, taps - 2) / 2.0
    assert taps > crossover_plan(48000, 8000)[0]
    # the floor: the lowest edge a 4095-tap filter serves
    floor = crossover_auto_floor_hz(48000)
    assert floor == pytest.approx(10.0 * crossover_width_hz(48000, CROSSOVER_MAX_TAPS), rel=1e-8) and 600.0 < floor < 700.0
    for edge in (0.0, 100.0, floor - 1.0, floor):
        (taps, cutoff, _), used = crossover_auto_plan(48000, 8000, edge)
        assert used == floor and taps == CROSSOVER_MAX_TAPS and cutoff * 48000 == pytest.approx(0.95 * floor)
    (taps, _, _), used = crossover_auto_plan(48000, 8000, floor + 50.0)
    assert used == floor + 50.0 and taps < CROSSOVER_MAX_TAPS
    # fixed taps: the floor is theirs, and taps too short for the low rate's own Nyquist frequency are refused as before
    (taps, _, _), used = crossover_auto_plan(48000, 8000, 500.0, 2001)
    assert taps == 2001 and used == crossover_auto_floor_hz(48000, 2001) > floor
    with pytest.raises(ValueError, match="use more taps"):
        check_crossover('input', 'auto', 101, 48000, 8000)
    # the existing errors
    with pytest.raises(ValueError, match="options of crossover='input'"):
        check_crossover(None, 'auto', None, 48000, 8000)
    with pytest.raises(ValueError, match="'auto'"):
        check_crossover('input', 'automatic', None, 48000, 8000)
    with pytest.raises(ValueError, match="nothing to cross over"):
        check_crossover('input', 'auto', None, 48000, 48000)


def test_notes():
    from pix2pixhdaudiosr_amd.generate import bandwidth_notes
    assert bandwidth_notes(4000.0, None, 4000.0) == [] and bandwidth_notes(3600.0, 20000.0, 4000.0) == []
    narrow = bandwidth_notes(3599.0, None, 4000.0)
    assert len(narrow) == 1 and "the generator was trained on inputs that reach it" in narrow[0] and "3.60 kHz" in narrow[0]
    empty = bandwidth_notes(4000.0, 4200.0, 4000.0)                # at 1.05 times the Nyquist frequency: still nothing above it
    assert len(empty) == 1 and "the original carries nothing above it: LSD-HF compares against an empty band" in empty[0]
    assert bandwidth_notes(4000.0, 4201.0, 4000.0) == [] and len(bandwidth_notes(0.0, 0.0, 4000.0)) == 2


# ------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------
def _stub_resolver(tops):
    """SuperResolver with every device step replaced; the bandwidth measurement 'returns' the k_top of `tops` for (lr, sr, hr)."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver

    class Stub(SuperResolver):
        def __init__(self):
            self.opt = SimpleNamespace(lr_sampling_rate=8000, hr_sampling_rate=48000)
            self.device = torch.device("cpu")
            self.calls = []

        def _read(self, path, slot='in0'):
            from pix2pixhdaudiosr_amd.data import wavio
            self.calls.append(('read', path))
            return torch.zeros(0, dtype=torch.uint8), wavio.info(path), slot

        def _decode(self, host, meta, slot):
            return torch.linspace(-1, 1, meta.num_frames)[None].repeat(meta.num_channels, 1)

        def enhance_lr(self, lr_audio, noise=None):
            return 1.7 * lr_audio

        def _measure_bandwidth(self, bw, lr, sr, hr):
            n = 2 if hr is None else 3
            self.calls.append(('measure', bw, n))
            res = torch.tensor([[k, k // bw['band_bins'], 1.0, 1e-6] for k in tops[:n]], dtype=torch.float64)
            return {'packed': res.reshape(-1).view(torch.uint8), 'clips': n, 'frames': 5}

        def _write(self, path_out, sr, encoding, stage=None, **extra):
            self.calls.append(('write', path_out, encoding, stage, extra))
            return None
    return Stub()


@pytest.fixture
def stub(tmp_path, monkeypatch):
    from pix2pixhdaudiosr_amd.data import audio_dataset, wavio
    from pix2pixhdaudiosr_amd.util import util as U
    monkeypatch.setattr(audio_dataset, "lr_round_trip", lambda raw, *a, **k: raw)
    monkeypatch.setattr(U, "compute_matrics", lambda *args, **kw: (1.0, 2.0, 3.0, 0, 0, 0, 4.0))      # a full-band file's metrics: no device
    src = tmp_path / "in"
    src.mkdir()
    for name, C, rate in (("a.wav", 1, 48000), ("b.wav", 2, 16000)):
        wavio.save(str(src / name), torch.zeros(C, 64), rate)
    return _stub_resolver((146, 989, 170)), src


KEYS = ['hr', 'info', 'lr', 'metrics', 'sr']
REC_KEYS = ['channels', 'error', 'frames', 'metrics', 'out_frames', 'path', 'rate', 'written_channels']


def test_nothing_moves_without_the_option(stub, tmp_path):
    sr, src = stub
    for kw in ({}, dict(bandwidth=False), dict(bandwidth=False, bandwidth_opts=None)):
        res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', **kw)
        assert sorted(res) == KEYS and sr.calls[-1] == ('write', str(tmp_path / "o.wav"), 'pcm16', None, {})
        assert sorted(sr.enhance_file(str(src / "b.wav"), None, is_lr_input=True, **kw)) == KEYS and sr.calls[-1][0] == 'read'
        recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all', **kw)
        assert [sorted(r) for r in recs] == [REC_KEYS] * 2
        assert [c[3:] for c in sr.calls if c[0] == 'write'][-2:] == [(None, {})] * 2
    assert not any(c[0] == 'measure' for c in sr.calls)


def test_the_option_reaches_the_file_path_and_the_result(stub, tmp_path):
    sr, src = stub
    res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', bandwidth=True)
    assert sorted(res) == sorted(KEYS + ['bandwidth'])
    assert sr.calls[-2] == ('measure', BR.DEFAULTS, 2) and sorted(sr.calls[-1][4]) == ['bandwidth']
    b = res['bandwidth']
    assert sorted(b) == ['band_bins', 'frames', 'hop', 'input', 'lr_nyquist', 'n_fft', 'notes', 'original', 'output', 'threshold_db']
    assert b['input'] == 146 * 48000.0 / 2048 and b['output'] == 989 * 48000.0 / 2048 and b['original'] is None
    assert (b['lr_nyquist'], b['threshold_db'], b['n_fft'], b['hop'], b['band_bins'], b['frames']) == (4000.0, 60.0, 2048, 1024, 8, 5)
    assert len(b['notes']) == 1 and "trained on inputs that reach it" in b['notes'][0]
    # a full-band original at the high rate: three clips, the original's note; the options; no file to write: measured all the same
    res = sr.enhance_file(str(src / "a.wav"), None, bandwidth=True, bandwidth_opts={'n_fft': 512, 'threshold_db': 50})
    assert sr.calls[-2] == ('measure', {'n_fft': 512, 'hop': 256, 'band_bins': 8, 'threshold_db': 50.0}, 3) and sr.calls[-1][:2] == ('write', None)
    b = res['bandwidth']
    assert b['original'] == 170 * 48000.0 / 512 and b['input'] == 146 * 48000.0 / 512 and b['n_fft'] == 512 and b['notes'] == []
    # nothing passed reads 0.0
    quiet = _stub_resolver((-1, -1, 40))
    b = quiet.enhance_file(str(src / "a.wav"), None, bandwidth=True)['bandwidth']
    assert (b['input'], b['output'], b['original']) == (0.0, 0.0, 40 * 48000.0 / 2048) and len(b['notes']) == 2
    # a folder: per-file records
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, bandwidth=True)
    assert [sorted(r) for r in recs] == [sorted(REC_KEYS + ['bandwidth'])] * 2 and all(r['bandwidth']['input'] == 146 * 48000.0 / 2048 for r in recs)


def test_refusals_come_before_a_file_is_read(stub, tmp_path):
    sr, src = stub
    n = len(sr.calls)
    for kw, word in ((dict(bandwidth='yes'), "bandwidth must be a bool"), (dict(bandwidth_opts={'n_fft': 512}), "options of bandwidth=True"),
                     (dict(bandwidth=True, bandwidth_opts={'threshold_db': 0}), "threshold_db must lie"),
                     (dict(bandwidth=True, bandwidth_opts={'width': 3}), "unknown bandwidth_opts")):
        with pytest.raises(ValueError, match=word):
            sr.enhance_file(str(src / "a.wav"), str(tmp_path / "x.wav"), is_lr_input=True, **kw)
        with pytest.raises(ValueError, match=word):
            sr.enhance_folder(str(src), str(tmp_path / "out2"), is_lr_input=True, **kw)
    with pytest.raises(ValueError, match="not built for loudness_scope='folder'"):
        sr.enhance_folder(str(src), str(tmp_path / "out2"), is_lr_input=True, loudness='report', loudness_scope='folder', bandwidth=True)
    assert len(sr.calls) == n and not (tmp_path / "x.wav").exists() and not (tmp_path / "out2").exists()


def test_cli_options_and_refusals(capsys):
    from pix2pixhdaudiosr_amd.generate import _parser, main
    a = _parser().parse_args(BASE)
    assert (a.bandwidth, a.bandwidth_threshold_db, a.bandwidth_n_fft, a.bandwidth_band_bins, a.crossover_hz) == (False, None, None, None, None)
    b = _parser().parse_args(BASE + ["--bandwidth", "--bandwidth_threshold_db", "45", "--bandwidth_n_fft", "512", "--bandwidth_band_bins", "4",
                                     "--crossover", "input", "--crossover_hz", "auto"])
    assert (b.bandwidth, b.bandwidth_threshold_db, b.bandwidth_n_fft, b.bandwidth_band_bins, b.crossover_hz) == (True, 45.0, 512, 4, "auto")
    assert _parser().parse_args(BASE + ["--crossover", "input", "--crossover_hz", "3000"]).crossover_hz == 3000.0
    for extra, word in ((["--bandwidth_n_fft", "512"], "--bandwidth_n_fft is an option of --bandwidth"),
                        (["--bandwidth", "--bandwidth_threshold_db", "0"], "threshold_db must lie"),
                        (["--bandwidth", "--bandwidth_n_fft", "1000"], "power of two"),
                        (["--crossover_hz", "sometimes"], "or auto")):
        with pytest.raises(SystemExit) as e:                      # ("ck" does not exist: loading anything would raise another error)
            main(BASE + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_prints_the_report_and_adds_the_columns(stub, tmp_path, capsys):
    """The part of main() behind the model's construction, on the stub: --bandwidth prints one line per file and one per note and adds
    three columns behind all others; without it not a word about it and the table as it was."""
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_BANDWIDTH, _parser, _run
    assert METRICS_COLUMNS_BANDWIDTH == ("bw_in", "bw_out", "bw_orig")
    sr, src = stub
    lines, tables = {}, {}
    for flag in ([], ["--bandwidth"]):
        for folder_mode, inp, out in ((False, src / "a.wav", tmp_path / "o.wav"), (True, src, tmp_path / "outdir")):
            csv_path = tmp_path / "m.csv"
            a = _parser().parse_args(["--input", str(inp), "--output", str(out), "--load_pretrain", "ck", "--metrics_csv", str(csv_path)] + flag)
            stage = dict(clip=a.clip, ceiling_dbfs=a.ceiling_dbfs, dither=a.dither, dither_seed=a.dither_seed, report_peaks=a.report_peaks)
            if flag:
                stage.update(bandwidth=True, bandwidth_opts=None)
            assert _run(a, sr, stage, None, 48000, folder_mode) == 0
            lines[(bool(flag), folder_mode)] = capsys.readouterr().out.splitlines()
            with open(csv_path, newline="") as f:
                tables[(bool(flag), folder_mode)] = list(csv.reader(f))
    for folder_mode, names in ((False, [str(tmp_path / "o.wav")]), (True, ["a.wav", "b.wav"])):
        plain, on = lines[(False, folder_mode)], lines[(True, folder_mode)]
        assert not any("bandwidth" in l or "note" in l for l in plain)
        extra = [l for l in on if l not in plain]
        assert [l for l in on if l in plain] == plain
        # a.wav is a full-band clip at the high rate (an original, 170 * 48000 / 2048 = 3.98 kHz: nothing above the Nyquist frequency);
        # b.wav is not
        want = ["%s: bandwidth input 3.42 kHz, output 23.18 kHz, original 3.98 kHz (-60 dB, low rate's Nyquist 4.00 kHz)" % names[0]]
        if folder_mode:
            want.append("%s: bandwidth input 3.42 kHz, output 23.18 kHz (-60 dB, low rate's Nyquist 4.00 kHz)" % names[1])
        assert [l for l in extra if "bandwidth input" in l] == want
        notes = [l for l in extra if ": note: " in l]
        assert len(extra) == len(want) + len(notes) and len(notes) == (3 if folder_mode else 2)
        assert sum("trained on inputs that reach it" in l for l in notes) == len(names) and sum("LSD-HF compares against an empty band" in l for l in notes) == 1
        off_rows, on_rows = tables[(False, folder_mode)], tables[(True, folder_mode)]
        assert tuple(off_rows[0]) == METRICS_COLUMNS and tuple(on_rows[0]) == METRICS_COLUMNS + METRICS_COLUMNS_BANDWIDTH
        assert [r[:-3] for r in on_rows] == off_rows and len(on_rows) == 3          # header, a.wav's channel, mean
        assert [float(v) for v in on_rows[1][-3:]] == [146 * 48000.0 / 2048, 989 * 48000.0 / 2048, 170 * 48000.0 / 2048] and on_rows[2][-3:] == on_rows[1][-3:]


def test_the_crossover_line():
    from pix2pixhdaudiosr_amd.generate.report import _print_crossover
    import io
    from contextlib import redirect_stdout
    buf = io.StringIO()
    with redirect_stdout(buf):
        _print_crossover({'hz': 3249.0, 'taps': 1031, 'edge_hz': 3420.0})
    assert buf.getvalue() == "crossover: 3.25 kHz, 1031 taps (input band ends at 3.42 kHz)\n"
