"""The stereo image report and the mid/side mode without a GPU: the premises of the measurement on the restatement
(tests/_stereo_ref.py) alone, the plans and their refusals, the figures, the note, the plumbing of the option through enhance_file /
enhance_folder on a stub, the printed line and the columns of --metrics_csv -- and that nothing moves without the options."""
import csv
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _stereo_ref as SR

BASE = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]


# ------------------------------------------------------------------------------------------
# the premises, on the restatement alone
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def premises():
    return {name: SR.image_ref(x, SR.HR, SR.LR, SR.N_FFT, SR.HOP)[0] for name, x in SR.premise_inputs().items()}


@pytest.mark.parametrize("name", ['same', 'inverted', 'half', 'independent', 'partial', 'split'])
def test_premise(premises, name):
    fig = premises[name]
    print(name, fig)
    SR.check_premise(name, fig)
    if name == 'same':
        assert fig['low']['side_db'] == fig['high']['side_db'] == float('-inf') and fig['low']['balance_db'] == 0.0
    if name == 'inverted':
        assert fig['low']['side_db'] == fig['high']['side_db'] == float('inf')
    if name == 'half':
        assert abs(fig['low']['corr'] - 1.0) <= 1e-12


def test_restatement_details():
    assert SR.split_bin_ref(48000, 8000, 2048) == 171 and SR.split_bin_ref(SR.HR, SR.LR, SR.N_FFT) == 22
    assert SR.split_bin_ref(48000, 24000, 2048) == 512             # a Nyquist frequency on a bin: that bin
    x = SR.premise_inputs()['partial']
    assert x.shape == (2, SR.SAMPLES) and np.abs(x).max() < 1.5
    v = SR.frame_values_ref(x, SR.N_FFT, SR.HOP)
    assert v.shape == (4, 63, 129) and (v[0] >= 0).all() and (v[2] ** 2 + v[3] ** 2 <= v[0] * v[1] * (1 + 1e-9)).all()
    assert SR.xspec_ref(x[:, :255], 256, 128).shape == (1, 4, 129) and not SR.xspec_ref(x[:, :255], 256, 128).any()
    # the order of the band sums shows on values 2^60 apart: ascending order would lose every small one
    big = np.zeros(600)
    big[0], big[1:] = 2.0 ** 60, 1.0
    assert SR.band_sum_ref(big) == 2.0 ** 60 + 512.0 != float(np.cumsum(big)[-1])
    # silence: no figure has a denominator
    assert SR.figures_ref(np.zeros(8)) == {b: {'corr': None, 'coherence': None, 'side_db': None, 'balance_db': None} for b in ('low', 'high')}


def test_matrix_restatement_returns_left_and_right_on_the_grid():
    """Operands on the 2^-15 grid (16-bit PCM): the sum and difference, their halves and the decoder's sum and difference are all
    exact in float32, so encode then decode returns L and R."""
    rng = np.random.default_rng(6)
    x = (rng.integers(-32768, 32768, (2, 4099)) / 32768.0).astype(np.float32)
    ms = SR.matrix_ref(x, 0.5)
    assert ms.dtype == np.float32 and np.array_equal(ms[0].astype(np.float64), (x[0].astype(np.float64) + x[1]) / 2)
    back = SR.matrix_ref(ms, 1.0, guard_side=True)
    assert np.array_equal(back.view(np.int32), x.view(np.int32))
    # the guard reads a non-finite side sample as +0 and leaves the mid row's alone
    y = np.array([[1.0, np.nan, 0.5, 0.25], [np.nan, 1.0, np.inf, -np.inf]], dtype=np.float32)
    g = SR.matrix_ref(y, 1.0, guard_side=True)
    assert g[0].tolist()[0] == 1.0 and math.isnan(g[0][1]) and g[:, 2].tolist() == [0.5, 0.5] and g[:, 3].tolist() == [0.25, 0.25]
    assert np.isnan(SR.matrix_ref(y, 1.0)[:, 0]).all()


# ------------------------------------------------------------------------------------------
# plans
# ------------------------------------------------------------------------------------------
def test_split_bin():
    from pix2pixhdaudiosr_amd.generate import stereo_split_bin
    assert stereo_split_bin(48000, 8000, 2048) == 171
    assert stereo_split_bin(48000, 48000, 2048) == 1024 and stereo_split_bin(48000, 1, 64) == 1      # the last bin; the first above bin 0
    for hr, lr, n in ((48000, 8000, 256), (48000, 16000, 2048), (44100, 11025, 1024), (48000, 24000, 2048), (16000, 8000, 64)):
        assert stereo_split_bin(hr, lr, n) == SR.split_bin_ref(hr, lr, n)
    for args, word in (((48000, 48001, 2048), r"must lie in \[1, 1024\]"), ((48000, 96000, 2048), "must lie in"),
                       ((0, 8000, 2048), "hr_rate"), ((48000, True, 2048), "lr_rate"), ((48000, 8000, 2.5), "n_fft")):
        with pytest.raises(ValueError, match=word):
            stereo_split_bin(*args)


def test_checks_and_their_error_texts():
    from pix2pixhdaudiosr_amd.generate import STEREO_DEFAULTS, STEREO_MODES, STEREO_NOTE_DROP, check_stereo, check_stereo_report
    assert STEREO_MODES == ('lr', 'ms') and STEREO_DEFAULTS == {'n_fft': 2048, 'hop': 1024} == SR.DEFAULTS and STEREO_NOTE_DROP == 0.3
    assert check_stereo('lr', "x") == 'lr' and check_stereo('ms', "x") == 'ms'
    for bad in ('LR', None, 'mid', 1):
        with pytest.raises(ValueError, match="x: stereo must be 'lr' or 'ms'"):
            check_stereo(bad, "x")
    assert check_stereo_report() is None and check_stereo_report(False, None, 'folder', "x") is None
    assert check_stereo_report(True) == STEREO_DEFAULTS and check_stereo_report(True, {'n_fft': None}) == STEREO_DEFAULTS
    assert check_stereo_report(True, {'n_fft': 512}) == {'n_fft': 512, 'hop': 256}
    assert check_stereo_report(True, {'n_fft': 64, 'hop': 64}) == {'n_fft': 64, 'hop': 64} and check_stereo_report(True, {'hop': 1})['hop'] == 1
    for args, word in ((('yes',), "stereo_report must be a bool"), ((True, [1]), "stereo_report_opts must be None or a dict"),
                       ((False, {'n_fft': 512}), "options of stereo_report=True"), ((True, None, 'folder'), "not built for loudness_scope='folder'"),
                       ((True, {'band_bins': 8}), "unknown stereo_report_opts"), ((True, {'n_fft': 1000}), "power of two"),
                       ((True, {'n_fft': 32}), "power of two"), ((True, {'n_fft': 4096}), "power of two"), ((True, {'n_fft': 512.0}), "power of two"),
                       ((True, {'hop': 0}), "hop must be an int"), ((True, {'n_fft': 64, 'hop': 65}), "hop must be an int"),
                       ((True, {'hop': True}), "hop must be an int")):
        with pytest.raises(ValueError, match=word):
            check_stereo_report(*args, who="who") if len(args) == 3 else check_stereo_report(*args)


def test_figures_are_the_restatements():
    from pix2pixhdaudiosr_amd.generate import stereo_figures
    rng = np.random.default_rng(8)
    for _ in range(20):
        ll, rr = rng.uniform(0.1, 5.0, 2), rng.uniform(0.1, 5.0, 2)
        c = rng.uniform(-1, 1, 2) * np.sqrt(ll * rr)
        im = rng.uniform(-0.2, 0.2, 2)
        res = [ll[0], rr[0], c[0], im[0], ll[1], rr[1], c[1], im[1]]
        assert stereo_figures(res) == SR.figures_ref(res)
    f = stereo_figures([2.0, 2.0, 2.0, 0.0, 4.0, 1.0, -2.0, 0.0])
    assert f['low'] == {'corr': 1.0, 'coherence': 1.0, 'side_db': float('-inf'), 'balance_db': 0.0}
    assert f['high']['corr'] == -1.0 and f['high']['side_db'] == 10.0 * math.log10(9.0) and f['high']['balance_db'] == 10.0 * math.log10(4.0)
    f = stereo_figures([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])                 # a silent right channel; an empty band
    assert f['low'] == {'corr': None, 'coherence': None, 'side_db': 0.0, 'balance_db': float('inf')}
    assert f['high'] == {'corr': None, 'coherence': None, 'side_db': None, 'balance_db': None}
    assert stereo_figures([0.0, 1.0, 0.0, 0.0, 1.0, 1.0, -1.0, 0.0])['low']['balance_db'] == float('-inf')
    assert stereo_figures([0.0, 1.0, 0.0, 0.0, 1.0, 1.0, -1.0, 0.0])['high']['side_db'] == float('inf')
    assert stereo_figures([1.0, 1.0, 0.0, 1.0] * 2)['low'] == {'corr': 0.0, 'coherence': 1.0, 'side_db': 0.0, 'balance_db': 0.0}
    assert math.isnan(stereo_figures([float('nan'), 1.0, 0.5, 0.0] * 2)['low']['corr'])
    with pytest.raises(ValueError, match="eight"):
        stereo_figures([1.0] * 4)


def _figs(lo, hi):
    return {'low': {'corr': lo, 'coherence': 1.0, 'side_db': -3.0, 'balance_db': 0.0}, 'high': {'corr': hi, 'coherence': 0.5, 'side_db': -1.5, 'balance_db': 0.5}}


def test_notes():
    from pix2pixhdaudiosr_amd.generate import stereo_notes
    assert stereo_notes(_figs(0.82, 0.60), 'lr') == [] and stereo_notes(_figs(0.82, 0.52), 'lr') == []       # a drop of 0.3 exactly: none
    note = stereo_notes(_figs(0.82, 0.04), 'lr')
    assert len(note) == 1 and "stereo='ms'" in note[0] and "+0.04" in note[0] and "+0.82" in note[0]
    assert stereo_notes(_figs(0.82, 0.04), 'ms') == [] and stereo_notes(_figs(None, 0.04), 'lr') == [] and stereo_notes(_figs(0.8, None), 'lr') == []
    assert len(stereo_notes(_figs(0.1, -0.5), 'lr')) == 1


# ------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------
SUMS = ([4.0, 4.0, 3.28, 0.1, 1.0, 1.0, 0.80, 0.0], [4.0, 4.0, 3.28, 0.1, 1.0, 1.0, 0.04, 0.3], [4.0, 4.0, 3.28, 0.1, 1.0, 1.0, 0.71, 0.0])


def _stub_resolver(mode='lr'):
    """SuperResolver with every device step replaced; the stereo measurement 'returns' SUMS for (lr, sr, hr)."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver

    class Stub(SuperResolver):
        def __init__(self):
            self.opt = SimpleNamespace(lr_sampling_rate=8000, hr_sampling_rate=48000)
            self.device = torch.device("cpu")
            self.stereo = mode
            self.calls = []

        def _read(self, path, slot='in0'):
            from pix2pixhdaudiosr_amd.data import wavio
            self.calls.append(('read', path))
            return torch.zeros(0, dtype=torch.uint8), wavio.info(path), slot

        def _decode(self, host, meta, slot):
            return torch.linspace(-1, 1, meta.num_frames)[None].repeat(meta.num_channels, 1)

        def enhance_lr(self, lr_audio, noise=None):
            return 1.7 * lr_audio

        def _measure_stereo(self, st, lr, sr, hr):
            n = 2 if hr is None else 3
            self.calls.append(('measure', st, n, tuple(sr.shape)))
            return {'packed': torch.tensor(SUMS[:n], dtype=torch.float64).reshape(-1).view(torch.uint8), 'clips': n, 'frames': 5}

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
    for name, C, rate in (("a.wav", 2, 48000), ("b.wav", 2, 16000), ("c.wav", 1, 48000), ("d.wav", 3, 48000)):
        wavio.save(str(src / name), torch.zeros(C, 64), rate)
    return _stub_resolver(), src


KEYS = ['hr', 'info', 'lr', 'metrics', 'sr']
REC_KEYS = ['channels', 'error', 'frames', 'metrics', 'out_frames', 'path', 'rate', 'written_channels']
STEREO_KEYS = ['frames', 'hop', 'input', 'mode', 'n_fft', 'notes', 'original', 'output', 'split_hz']


def test_nothing_moves_without_the_option(stub, tmp_path):
    sr, src = stub
    for kw in ({}, dict(stereo_report=False), dict(stereo_report=False, stereo_report_opts=None)):
        res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', **kw)
        assert sorted(res) == KEYS and sr.calls[-1] == ('write', str(tmp_path / "o.wav"), 'pcm16', None, {})
        assert sorted(sr.enhance_file(str(src / "b.wav"), None, is_lr_input=True, **kw)) == KEYS and sr.calls[-1][0] == 'read'
        recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all', **kw)
        assert [sorted(r) for r in recs] == [REC_KEYS] * 4 and all(r['error'] is None for r in recs)
        assert [c[3:] for c in sr.calls if c[0] == 'write'][-4:] == [(None, {})] * 4
    assert not any(c[0] == 'measure' for c in sr.calls)


def test_the_option_reaches_the_file_path_and_the_result(stub, tmp_path):
    sr, src = stub
    res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', stereo_report=True)
    assert sorted(res) == sorted(KEYS + ['stereo'])
    assert sr.calls[-2] == ('measure', SR.DEFAULTS, 2, (2, 64)) and sorted(sr.calls[-1][4]) == ['stereo']
    s = res['stereo']
    assert sorted(s) == STEREO_KEYS
    assert s['input'] == SR.figures_ref(SUMS[0]) and s['output'] == SR.figures_ref(SUMS[1]) and s['original'] is None
    assert (s['split_hz'], s['n_fft'], s['hop'], s['frames'], s['mode']) == (171 * 48000.0 / 2048, 2048, 1024, 5, 'lr')
    assert len(s['notes']) == 1 and "stereo='ms'" in s['notes'][0]
    # a full-band original at the high rate: three clips; the options; no file to write: measured all the same
    res = sr.enhance_file(str(src / "a.wav"), None, channels='all', stereo_report=True, stereo_report_opts={'n_fft': 512})
    assert sr.calls[-2] == ('measure', {'n_fft': 512, 'hop': 256}, 3, (2, 64)) and sr.calls[-1][:2] == ('write', None)
    s = res['stereo']
    assert s['original'] == SR.figures_ref(SUMS[2]) and s['split_hz'] == 43 * 48000.0 / 512 and s['n_fft'] == 512
    # another channel count: the key, None, nothing measured, nothing more fetched
    n = len(sr.calls)
    for name, channels in (("c.wav", 'all'), ("a.wav", 'first'), ("d.wav", 'all')):
        res = sr.enhance_file(str(src / name), str(tmp_path / "o.wav"), channels=channels, stereo_report=True)
        assert sorted(res) == sorted(KEYS + ['stereo']) and res['stereo'] is None and sr.calls[-1][4] == {}
    assert not any(c[0] == 'measure' for c in sr.calls[n:])
    # the mode in the result, and no note with it
    ms = _stub_resolver('ms')
    s = ms.enhance_file(str(src / "b.wav"), None, is_lr_input=True, channels='all', stereo_report=True)['stereo']
    assert s['mode'] == 'ms' and s['notes'] == [] and s['output'] == SR.figures_ref(SUMS[1])
    # a folder: per-file records
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all', stereo_report=True)
    assert [sorted(r) for r in recs] == [sorted(REC_KEYS + ['stereo'])] * 4
    assert [r['stereo'] is None for r in recs] == [False, False, True, True]


def test_ms_skips_a_file_of_more_than_two_channels(stub, tmp_path):
    _, src = stub
    ms = _stub_resolver('ms')
    recs = ms.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all')
    assert [r['error'] is None for r in recs] == [True, True, True, False] and "stereo='ms' takes one or two channels, 3 would be written" in recs[3]['error']
    assert [sorted(r) for r in recs] == [REC_KEYS] * 4 and not (tmp_path / "out" / "d.wav").exists() and len([c for c in ms.calls if c[0] == 'write']) == 3
    assert all(r['error'] is None for r in ms.enhance_folder(str(src), str(tmp_path / "out2"), is_lr_input=True, channels=2))
    with pytest.raises(ValueError, match="takes one or two channels"):
        ms.enhance_file(str(src / "d.wav"), str(tmp_path / "x.wav"), channels='all')
    assert not (tmp_path / "x.wav").exists()


def test_refusals_come_before_a_file_is_read(stub, tmp_path):
    sr, src = stub
    n = len(sr.calls)
    for kw, word in ((dict(stereo_report='yes'), "stereo_report must be a bool"), (dict(stereo_report_opts={'n_fft': 512}), "options of stereo_report=True"),
                     (dict(stereo_report=True, stereo_report_opts={'n_fft': 100}), "power of two"),
                     (dict(stereo_report=True, stereo_report_opts={'width': 3}), "unknown stereo_report_opts")):
        with pytest.raises(ValueError, match=word):
            sr.enhance_file(str(src / "a.wav"), str(tmp_path / "x.wav"), is_lr_input=True, **kw)
        with pytest.raises(ValueError, match=word):
            sr.enhance_folder(str(src), str(tmp_path / "out2"), is_lr_input=True, **kw)
    with pytest.raises(ValueError, match="not built for loudness_scope='folder'"):
        sr.enhance_folder(str(src), str(tmp_path / "out2"), is_lr_input=True, loudness='report', loudness_scope='folder', stereo_report=True)
    assert len(sr.calls) == n and not (tmp_path / "x.wav").exists() and not (tmp_path / "out2").exists()


def test_cli_options_and_refusals(capsys):
    from pix2pixhdaudiosr_amd.generate import _parser, main
    a = _parser().parse_args(BASE)
    assert (a.stereo, a.stereo_report, a.stereo_n_fft, a.stereo_hop) == ('lr', False, None, None)
    b = _parser().parse_args(BASE + ["--stereo", "ms", "--stereo_report", "--stereo_n_fft", "512", "--stereo_hop", "128"])
    assert (b.stereo, b.stereo_report, b.stereo_n_fft, b.stereo_hop) == ('ms', True, 512, 128)
    for extra, word in ((["--stereo_n_fft", "512"], "--stereo_n_fft is an option of --stereo_report"),
                        (["--stereo_hop", "512"], "--stereo_hop is an option of --stereo_report"),
                        (["--stereo_report", "--stereo_n_fft", "1000"], "power of two"),
                        (["--stereo_report", "--stereo_hop", "4096"], "hop must be an int"),
                        (["--stereo", "side"], "invalid choice")):
        with pytest.raises(SystemExit) as e:                      # ("ck" does not exist: loading anything would raise another error)
            main(BASE + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_prints_the_report_and_adds_the_columns(stub, tmp_path, capsys):
    """The part of main() behind the model's construction, on the stub: --stereo_report prints one line per two-channel file and one
    per note and adds four columns behind all others; without it not a word about it and the table as it was."""
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_STEREO, _parser, _run
    assert METRICS_COLUMNS_STEREO == ("corr_lf_out", "corr_hf_out", "corr_hf_orig", "side_hf_out_db")
    sr, src = stub
    lines, tables = {}, {}
    for flag in ([], ["--stereo_report"]):
        for folder_mode, inp, out in ((False, src / "a.wav", tmp_path / "o.wav"), (True, src, tmp_path / "outdir")):
            csv_path = tmp_path / "m.csv"
            a = _parser().parse_args(["--input", str(inp), "--output", str(out), "--load_pretrain", "ck", "--metrics_csv", str(csv_path),
                                      "--channels", "all"] + flag)
            stage = dict(clip=a.clip, ceiling_dbfs=a.ceiling_dbfs, dither=a.dither, dither_seed=a.dither_seed, report_peaks=a.report_peaks)
            if flag:
                stage.update(stereo_report=True, stereo_report_opts=None)
            assert _run(a, sr, stage, None, 48000, folder_mode) == 0
            lines[(bool(flag), folder_mode)] = capsys.readouterr().out.splitlines()
            with open(csv_path, newline="") as f:
                tables[(bool(flag), folder_mode)] = list(csv.reader(f))
    side = SR.figures_ref(SUMS[1])['high']['side_db']
    for folder_mode, names in ((False, [str(tmp_path / "o.wav")]), (True, ["a.wav", "b.wav"])):
        plain, on = lines[(False, folder_mode)], lines[(True, folder_mode)]
        assert not any("stereo" in l or "note" in l for l in plain)
        extra = [l for l in on if l not in plain]
        assert [l for l in on if l in plain] == plain
        # a.wav is a full-band clip at the high rate (an original); b.wav is not; c.wav and d.wav have no stereo image and no line
        want = ["%s: stereo correlation below / above 4.01 kHz: input +0.82 / +0.80, output +0.82 / +0.04, original +0.82 / +0.71" % names[0]]
        if folder_mode:
            want.append("%s: stereo correlation below / above 4.01 kHz: input +0.82 / +0.80, output +0.82 / +0.04" % names[1])
        assert [l for l in extra if "stereo correlation" in l] == want
        notes = [l for l in extra if ": note: " in l]
        assert len(extra) == len(want) + len(notes) and len(notes) == len(names) and all("--stereo ms" in l for l in notes)
        off_rows, on_rows = tables[(False, folder_mode)], tables[(True, folder_mode)]
        assert tuple(off_rows[0]) == METRICS_COLUMNS and tuple(on_rows[0]) == METRICS_COLUMNS + METRICS_COLUMNS_STEREO
        assert [r[:-4] for r in on_rows] == off_rows
        # the rows with metrics: a.wav's two channels (c.wav's one and d.wav's three in a folder), then the mean
        assert len(on_rows) == (1 + 6 + 1 if folder_mode else 1 + 2 + 1)
        for row in on_rows[1:3]:
            assert [float(v) for v in row[-4:]] == [0.82, 0.04, 0.71, side]
        assert [float(v) for v in on_rows[-1][-4:]] == [0.82, 0.04, 0.71, side]                         # the mean skips the rows without a figure
        if folder_mode:
            assert all(math.isnan(float(v)) for row in on_rows[3:-1] for v in row[-4:])


def test_the_line_without_a_figure(capsys):
    from pix2pixhdaudiosr_amd.generate.report import _print_stereo
    s = {'input': SR.figures_ref(np.zeros(8)), 'output': SR.figures_ref(SUMS[1]), 'original': None, 'split_hz': 4007.8125, 'notes': ['one', 'two']}
    _print_stereo("x.wav", s)
    assert capsys.readouterr().out.splitlines() == ["x.wav: stereo correlation below / above 4.01 kHz: input n/a / n/a, output +0.82 / +0.04",
                                                   "x.wav: note: one", "x.wav: note: two"]
