"""enhance_file(bandwidth=True) / enhance_folder / --bandwidth and SuperResolver(crossover_hz='auto') on the GPU: the report against
the restatement of tests/_bandwidth_ref.py on the returned clips; without the option every byte, key, line and launch is the
parent's; the auto crossover is the crossover kernel with the restatement's plan behind the plain pipeline (the criterion of
tests/test_gpu_generate_crossover.py) and, for an input that reaches the low rate's Nyquist frequency, the fixed crossover byte for
byte; folders and the command line.  The tiny model is the one of tests/test_gpu_generate_loudness.py; clips of eight segments."""
import csv
import os
import re

import numpy as np
import pytest
import torch

import _bandwidth_ref as BR
from test_gpu_generate_loudness import RATE, _bytes, _excerpt, _opt, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 8000                                                           # eight segments of 992 samples; six frames of 2048 at hop 1024
FAMILIES = ("gconv", "halo", "cls_skip", "march", "march_w", "wgrad", "splitk", "tile256", "tile128x192", "dfirst", "dlast", "c7",
            "thin_wgrad", "timed_pack", "timed_frames", "stitch", "pcm", "metrics_rows", "xover", "specimg", "loudness", "truepeak",
            "limiter", "bandwidth")
BW_KEYS = ['band_bins', 'frames', 'hop', 'input', 'lr_nyquist', 'n_fft', 'notes', 'original', 'output', 'threshold_db']


def _counts(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    lib = _lib.lib()
    out = {f: lib.p2phd_launch_count(f.encode(), 0) for f in FAMILIES}
    assert min(out.values()) >= 0
    if reset:
        lib.p2phd_launch_count(None, 1)
    return out


def _ref(rows, plan=None):
    """(Hz, k_top, the margin in dB of the nearest level to thr) of the restatement on a returned clip, all channels one programme."""
    x = rows.cpu().numpy()
    p = dict(BR.DEFAULTS, **(plan or {}))
    hz, res = BR.bandwidth_ref(x, RATE, p)
    return hz, int(res[0]), BR.margin_db(BR.ltas_ref(x, p['n_fft'], p['hop']), x.shape[0], p['band_bins'], BR.rel_of(p['threshold_db']))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """narrow.wav: a '48 kHz' file whose content stops at 2.5 kHz (brick-wall noise), for --is_lr_input; full.wav, stereo.wav: speech
    at the high rate, which goes through the round trip and is its own original."""
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("bandwidth_in")
    wavio.save(str(d / "narrow.wav"), torch.from_numpy(BR.brickwall_noise(N, RATE, 2500.0, 3).astype(np.float32)), RATE)
    x = _excerpt()
    # (slices of the stored excerpt on which every level of the restatement's decision stands more than 0.5 dB from thr)
    wavio.save(str(d / "full.wav"), 0.5 * x[4000:4000 + N], RATE)
    wavio.save(str(d / "stereo.wav"), torch.stack([0.5 * x[5000:5000 + N - 500], -0.3 * x[15000:15000 + N - 500]]), RATE)
    return d


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    return SuperResolver(model, opt)


# ------------------------------------------------------------------------------------------
# the report
# ------------------------------------------------------------------------------------------
def test_report_is_the_restatement_on_the_returned_clips(resolver, files, tmp_path):
    resolver.enhance_file(str(files / "narrow.wav"), None, is_lr_input=True)      # capture, tables, packed weights
    torch.manual_seed(5)
    _counts(reset=True)
    res = resolver.enhance_file(str(files / "narrow.wav"), str(tmp_path / "on.wav"), is_lr_input=True, bandwidth=True)
    assert _counts()["bandwidth"] == 4                             # the input and the generated clip, two launches each
    assert sorted(res) == ['bandwidth', 'hr', 'info', 'lr', 'metrics', 'sr'] and res['hr'] is None
    b = res['bandwidth']
    assert sorted(b) == BW_KEYS
    hz, k_top, margin = _ref(res['lr'])
    print(f"input: {b['input']:.2f} Hz; restatement {hz:.2f} Hz (bin {k_top}), nearest level {margin:.2f} dB from thr")
    # the premise: nothing of the restatement's decision stands within 0.1 dB of thr -- the fp32 error at -60 dB is three orders smaller
    assert margin >= 0.1 and 0 <= k_top - 2500.0 * 2048 / RATE <= 8
    assert b['input'] == k_top * float(RATE) / 2048 == hz
    assert b['original'] is None and b['lr_nyquist'] == 4000.0
    assert (b['threshold_db'], b['n_fft'], b['hop'], b['band_bins']) == (60.0, 2048, 1024, 8)
    assert b['frames'] == BR.frames_ref(N, 2048, 1024) == 6 and res['sr'].shape[-1] == N
    assert len(b['notes']) == 1 and "the generator was trained on inputs that reach it" in b['notes'][0]
    hz_out, k_out, margin_out = _ref(res['sr'])
    print(f"output: {b['output']:.2f} Hz; restatement {hz_out:.2f} Hz, nearest level {margin_out:.2f} dB from thr")
    if margin_out >= 0.1:
        assert b['output'] == hz_out
    # twice: the same figures; other options of the plan
    torch.manual_seed(5)
    assert resolver.enhance_file(str(files / "narrow.wav"), None, is_lr_input=True, bandwidth=True)['bandwidth'] == b
    plan = {'n_fft': 512, 'hop': 256, 'band_bins': 4, 'threshold_db': 50.0}
    torch.manual_seed(5)
    other = resolver.enhance_file(str(files / "narrow.wav"), None, is_lr_input=True, bandwidth=True, bandwidth_opts=dict(plan))['bandwidth']
    hz2, k2, margin2 = _ref(res['lr'], plan)
    assert margin2 >= 0.1 and other['input'] == hz2 and other['frames'] == BR.frames_ref(N, 512, 256) and other['n_fft'] == 512


def test_report_with_an_original(resolver, files):
    """A full-band file at the high rate: three clips, six launches; the round trip's band ends above the low rate's Nyquist
    frequency (the resampler's images), the original's far above it: no note."""
    torch.manual_seed(5)
    _counts(reset=True)
    res = resolver.enhance_file(str(files / "full.wav"), None, bandwidth=True)
    assert _counts()["bandwidth"] == 6
    b = res['bandwidth']
    for key, rows in (('input', res['lr']), ('original', res['hr'])):
        hz, k_top, margin = _ref(rows)
        print(f"{key}: {b[key]:.2f} Hz; restatement {hz:.2f} Hz, nearest level {margin:.2f} dB from thr")
        assert margin >= 0.1 and b[key] == hz
    assert 4000.0 < b['input'] < 7000.0 and b['original'] > 15000.0 and b['notes'] == []
    # all channels of a clip are one programme
    torch.manual_seed(5)
    st = resolver.enhance_file(str(files / "stereo.wav"), None, channels='all', bandwidth=True)
    hz, _, margin = _ref(st['hr'])
    assert tuple(st['hr'].shape) == (2, N - 500) and margin >= 0.1 and st['bandwidth']['original'] == hz


def test_option_off_is_the_parent(resolver, files, tmp_path):
    resolver.enhance_file(str(files / "full.wav"), None)           # capture, tables, packed weights
    runs = {}
    for name, kw in (("plain", {}), ("off", dict(bandwidth=False, bandwidth_opts=None)), ("on", dict(bandwidth=True))):
        torch.manual_seed(5)
        _counts(reset=True)
        res = resolver.enhance_file(str(files / "full.wav"), str(tmp_path / (name + ".wav")), **kw)
        runs[name] = (res, _counts(), _bytes(str(tmp_path / (name + ".wav"))))
    assert sorted(runs["plain"][0]) == sorted(runs["off"][0]) == ['hr', 'info', 'lr', 'metrics', 'sr']
    assert runs["off"][1] == runs["plain"][1] and runs["plain"][1]["bandwidth"] == 0 and runs["off"][2] == runs["plain"][2]
    assert runs["plain"][0]['metrics'] == runs["off"][0]['metrics']
    # with it: the same bytes and the same launches of every other family
    assert runs["on"][2] == runs["plain"][2] and runs["on"][0]['metrics'] == runs["plain"][0]['metrics']
    assert {f: n for f, n in runs["on"][1].items() if f != "bandwidth"} == {f: n for f, n in runs["plain"][1].items() if f != "bandwidth"}
    with pytest.raises(ValueError, match="options of bandwidth=True"):
        resolver.enhance_file(str(files / "full.wav"), str(tmp_path / "never.wav"), bandwidth_opts={'n_fft': 512})
    with pytest.raises(ValueError, match="not built for loudness_scope='folder'"):
        resolver.enhance_folder(str(files), str(tmp_path / "never"), loudness='report', loudness_scope='folder', bandwidth=True)
    assert not os.path.exists(str(tmp_path / "never.wav")) and not os.path.exists(str(tmp_path / "never"))


# ------------------------------------------------------------------------------------------
# crossover_hz='auto'
# ------------------------------------------------------------------------------------------
def _noise(sr, rows, seed):
    shape = sr.noise_shape(1)
    return torch.randn((rows,) + shape[1:], generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_auto_crossover_on_a_narrow_band_input(files, tmp_path):
    """The clip is the crossover kernel, with the plan the restatement's band edge gives, behind the plain pipeline -- bit for bit, the
    criterion of tests/test_gpu_generate_crossover.py: below the crossover the input, above the edge the generated clip."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver, crossover, crossover_auto_plan, crossover_coefficients, crossover_plan, segment_plan
    model, opt = _tiny()
    plain = SuperResolver(model, opt)
    auto = SuperResolver(model, opt, crossover='input', crossover_hz='auto')
    assert auto.crossover_auto and auto.crossover_plan == crossover_plan(RATE, 8000) and not getattr(plain, 'crossover_auto')
    x = torch.from_numpy(np.stack([BR.brickwall_noise(N, RATE, 2500.0, 3), BR.brickwall_noise(N, RATE, 2000.0, 4)]).astype(np.float32)).to(DEV)
    hz, k_top, margin = _ref(x)
    assert margin >= 0.1 and hz < 3000.0
    want_plan, edge = crossover_auto_plan(RATE, 8000, hz)
    assert edge == hz and want_plan[0] > auto.crossover_plan[0]
    noise = _noise(plain, 2 * segment_plan(N, opt.segment_length, 0.25)[0], 9)
    base = plain.enhance_lr(x, noise=noise)
    want = crossover(base, x, plain.gain / 2.0, crossover_coefficients(*want_plan).to(DEV))
    _counts(reset=True)
    got = auto.enhance_lr(x, noise=noise)
    torch.cuda.synchronize()
    counts = _counts()
    assert counts["bandwidth"] == 2 and counts["xover"] == 1
    assert auto.last_crossover == {'hz': want_plan[1] * RATE, 'taps': want_plan[0], 'edge_hz': hz}
    assert auto.last_crossover['hz'] == pytest.approx(0.95 * hz, rel=1e-12)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not torch.equal(got, base)
    # again: the cached table; one channel of it alone is another clip with another edge
    assert torch.equal(auto.enhance_lr(x, noise=noise), got) and len(auto._xover_auto) == 1
    auto.enhance_lr(x[1:], noise=noise[:noise.shape[0] // 2])
    assert len(auto._xover_auto) == 2 and auto.last_crossover['edge_hz'] == _ref(x[1:])[0] < hz
    # through the file path: the result's 'crossover'
    torch.manual_seed(5)
    res = auto.enhance_file(str(files / "narrow.wav"), str(tmp_path / "auto.wav"), is_lr_input=True)
    hz_file = _ref(res['lr'])[0]
    plan_file, _ = crossover_auto_plan(RATE, 8000, hz_file)
    assert sorted(res) == ['crossover', 'hr', 'info', 'lr', 'metrics', 'sr']
    assert res['crossover'] == {'hz': plan_file[1] * RATE, 'taps': plan_file[0], 'edge_hz': hz_file}


def test_auto_crossover_on_a_full_band_input_is_the_fixed_one(files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, crossover_plan
    model, opt = _tiny()
    out = {}
    for name, kw in (("fixed", {}), ("auto", dict(crossover_hz='auto'))):
        sr = SuperResolver(model, opt, crossover='input', **kw)
        torch.manual_seed(5)
        res = sr.enhance_file(str(files / "full.wav"), str(tmp_path / (name + ".wav")), encoding='float32')
        out[name] = (res, _bytes(str(tmp_path / (name + ".wav"))))
    assert 'crossover' not in out["fixed"][0]
    taps, cutoff, _ = crossover_plan(RATE, 8000)
    assert out["auto"][0]['crossover'] == {'hz': cutoff * RATE, 'taps': taps, 'edge_hz': 4000.0}
    assert _ref(out["auto"][0]['lr'])[0] > 4000.0                 # the round trip's band ends above the Nyquist frequency
    assert out["auto"][1] == out["fixed"][1] and torch.equal(out["auto"][0]['sr'], out["fixed"][0]['sr'])
    with pytest.raises(ValueError, match=r"options of crossover='input'"):
        SuperResolver(model, opt, crossover_hz='auto')


# ------------------------------------------------------------------------------------------
# folders and the command line
# ------------------------------------------------------------------------------------------
def test_folder_records_and_csv(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_BANDWIDTH, write_metrics_csv
    recs = resolver.enhance_folder(str(files), str(tmp_path / "on"), channels='all', seed=11, bandwidth=True)
    by = {r['path']: r for r in recs}
    assert sorted(by) == ["full.wav", "narrow.wav", "stereo.wav"] and all(sorted(r['bandwidth']) == BW_KEYS for r in recs)
    for name in by:
        torch.manual_seed(11)
        one = resolver.enhance_file(str(files / name), str(tmp_path / ("one_" + name)), channels='all', bandwidth=True)
        assert by[name]['bandwidth'] == one['bandwidth'] and _bytes(str(tmp_path / "on" / name)) == _bytes(str(tmp_path / ("one_" + name)))
    write_metrics_csv(str(tmp_path / "on.csv"), recs, bandwidth=True)
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == METRICS_COLUMNS + METRICS_COLUMNS_BANDWIDTH and len(rows) == 1 + 4 + 1     # every file is its own original here
    for row in rows[1:-1]:
        b = by[row[0]]['bandwidth']
        assert [float(v) for v in row[-3:]] == [b['input'], b['output'], b['original']]


def test_cli_lines_and_csv_columns(files, tmp_path, capsys):
    """Without --bandwidth main() prints the lines and writes the columns of the parent; with it one `bandwidth` line per file, one
    per note, and three columns more, holding what enhance_file returns.  --crossover_hz auto prints the file's crossover."""
    from pix2pixhdaudiosr_amd import generate as G
    from pix2pixhdaudiosr_amd.models.models import create_model
    common = dict(mdct_type="mdct4", checkpoints_dir=str(tmp_path), name="run", seed=1234)
    torch.manual_seed(1234)
    create_model(_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:                       # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    base = ["--input", str(files / "full.wav"), "--load_pretrain", str(folder), "--encoding", "float32"]
    _counts(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "off.wav"), "--metrics_csv", str(tmp_path / "off.csv")]) == 0
    assert _counts()["bandwidth"] == 0
    off = capsys.readouterr().out.splitlines()
    assert not any("bandwidth" in l or "crossover" in l for l in off)
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(G.METRICS_COLUMNS)
    _counts(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--metrics_csv", str(tmp_path / "on.csv"), "--bandwidth"]) == 0
    assert _counts()["bandwidth"] == 6
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if ": bandwidth " in l or ": note: " in l]
    assert len(extra) == 1 and [l.replace("on.wav", "off.wav").replace("on.csv", "off.csv") for l in on if l not in extra] == off
    m = re.fullmatch(re.escape(str(tmp_path / "on.wav")) + r": bandwidth input (\d+\.\d\d) kHz, output (\d+\.\d\d) kHz, original (\d+\.\d\d) kHz "
                     r"\(-60 dB, low rate's Nyquist 4\.00 kHz\)", extra[0])
    assert m, extra[0]
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == G.METRICS_COLUMNS + G.METRICS_COLUMNS_BANDWIDTH and len(rows) == 3
    assert ["%.2f" % (float(v) / 1000.0) for v in rows[1][-3:]] == [m.group(1), m.group(2), m.group(3)] and rows[2][-3:] == rows[1][-3:]
    assert rows[1][:7] == list(csv.reader(open(str(tmp_path / "off.csv"))))[1] and _bytes(str(tmp_path / "on.wav")) == _bytes(str(tmp_path / "off.wav"))
    # folder mode, a narrow-band input, the auto crossover: one bandwidth line and one crossover line per file, and the note
    assert G.main(["--input", str(files), "--output", str(tmp_path / "dir"), "--load_pretrain", str(folder), "--is_lr_input", "--bandwidth",
                   "--bandwidth_threshold_db", "50", "--crossover", "input", "--crossover_hz", "auto"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert sum(": bandwidth input " in l and "(-50 dB" in l for l in lines) == 3
    assert sum(re.fullmatch(r"crossover: \d+\.\d\d kHz, \d+ taps \(input band ends at \d+\.\d\d kHz\)", l) is not None for l in lines) == 3
    assert any(l.startswith("narrow.wav: note: ") and "trained on inputs that reach it" in l for l in lines)
    assert any("(auto)" in l for l in lines)
    # an option of --bandwidth: the parser's error, before anything is loaded
    with pytest.raises(SystemExit):
        G.main(base + ["--output", str(tmp_path / "no.wav"), "--bandwidth_band_bins", "4"])
    assert "--bandwidth_band_bins is an option of --bandwidth" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "no.wav"))


def test_auto_crossover_reaches_the_album_pipeline(files, tmp_path):
    """loudness_scope='folder' generates through enhance_lr too: every record carries the crossover its file got."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    auto = SuperResolver(model, opt, crossover='input', crossover_hz='auto')
    recs = auto.enhance_folder(str(files), str(tmp_path / "album"), is_lr_input=True, seed=11, loudness=-23.0, loudness_scope='folder')
    assert [r['path'] for r in recs] == ["full.wav", "narrow.wav", "stereo.wav"] and all(r['error'] is None for r in recs)
    for r in recs:
        torch.manual_seed(11)
        one = auto.enhance_file(str(files / r['path']), None, is_lr_input=True)
        assert sorted(r['crossover']) == ['edge_hz', 'hz', 'taps'] and r['crossover'] == one['crossover']
    by = {r['path']: r['crossover'] for r in recs}
    assert by["full.wav"]['edge_hz'] == 4000.0 and by["narrow.wav"]['edge_hz'] < 3000.0 and by["narrow.wav"]['taps'] > by["full.wav"]['taps']
    plain = SuperResolver(model, opt, crossover='input').enhance_folder(str(files), str(tmp_path / "plain"), is_lr_input=True, seed=11,
                                                                        loudness=-23.0, loudness_scope='folder')
    assert all('crossover' not in r for r in plain)
