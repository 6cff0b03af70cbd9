"""SuperResolver(stereo='ms') and enhance_file(stereo_report=True) / enhance_folder / --stereo / --stereo_report on the GPU: without
the options every byte, key, line and launch is the parent's; the mode is the matrix kernel around the unchanged pipeline, bit for
bit, with the auto crossover's measurement left on left / right; a dual-mono file comes out dual mono, finite, and as its mono run;
the report against the restatement of tests/_stereo_ref.py on the returned clips; folders, the album pipeline and the command line.
The tiny model is the one of tests/test_gpu_generate_loudness.py; clips of eight segments."""
import csv
import os
import re

import numpy as np
import pytest
import torch

import _stereo_ref as SR
from _bandwidth_ref import brickwall_noise, frames_ref
from test_gpu_generate_bandwidth import FAMILIES as PARENT_FAMILIES
from test_gpu_generate_loudness import RATE, _bytes, _excerpt, _opt, _tiny
from test_gpu_stereo import _xspec_bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 8000                                                           # eight segments of 992 samples; six frames of 2048 at hop 1024
FAMILIES = PARENT_FAMILIES + ("stereo",)
STEREO_KEYS = ['frames', 'hop', 'input', 'mode', 'n_fft', 'notes', 'original', 'output', 'split_hz']
KEYS = ['hr', 'info', 'lr', 'metrics', 'sr']


def _counts(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    lib = _lib.lib()
    out = {f: lib.p2phd_launch_count(f.encode(), 0) for f in FAMILIES}
    assert min(out.values()) >= 0
    if reset:
        lib.p2phd_launch_count(None, 1)
    return out


def _others(counts):
    return {f: n for f, n in counts.items() if f != "stereo"}


def _same(a, b):
    """Bit for bit (a zero's sign aside: M + 0 is +0 where M is -0)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and bool(((a.view(torch.int32) == b.view(torch.int32)) | ((a == 0) & (b == 0))).all())


def _noise(sr, rows, seed):
    shape = sr.noise_shape(1)
    return torch.randn((rows,) + shape[1:], generator=torch.Generator().manual_seed(seed)).to(DEV)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Speech at the high rate, which goes through the round trip and is its own original: mono.wav; stereo.wav, two channels with a
    shared part and a part of their own; dual.wav, R = L; three.wav, three channels."""
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("stereo_in")
    x = _excerpt()
    a, b, c = 0.5 * x[4000:4000 + N], 0.4 * x[9000:9000 + N], 0.4 * x[15000:15000 + N]
    wavio.save(str(d / "mono.wav"), a, RATE)
    wavio.save(str(d / "stereo.wav"), torch.stack([a + 0.3 * b, a - 0.3 * c]), RATE)
    wavio.save(str(d / "three.wav"), torch.stack([a, b, c])[:, :N - 500], RATE)
    return d


@pytest.fixture(scope="module")
def dual(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("stereo_dual")
    a = 0.5 * _excerpt()[4000:4000 + N]
    wavio.save(str(d / "dual.wav"), torch.stack([a, a]), RATE)
    wavio.save(str(d / "left.wav"), a, RATE)
    return d


@pytest.fixture(scope="module")
def resolvers():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    return SuperResolver(model, opt), SuperResolver(model, opt, stereo='ms')


# ------------------------------------------------------------------------------------------
# the options off
# ------------------------------------------------------------------------------------------
def test_option_off_is_the_parent(files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    SuperResolver(model, opt).enhance_file(str(files / "stereo.wav"), None, channels='all')      # capture, tables, packed weights
    runs = {}
    for name, make, kw in (("plain", {}, {}), ("off", dict(stereo='lr'), dict(stereo_report=False, stereo_report_opts=None)),
                           ("on", {}, dict(stereo_report=True))):
        sr = SuperResolver(model, opt, **make)
        assert sr.stereo == 'lr'
        torch.manual_seed(5)
        _counts(reset=True)
        res = sr.enhance_file(str(files / "stereo.wav"), str(tmp_path / (name + ".wav")), channels='all', **kw)
        runs[name] = (res, _counts(), _bytes(str(tmp_path / (name + ".wav"))))
    assert sorted(runs["plain"][0]) == sorted(runs["off"][0]) == KEYS
    assert runs["off"][1] == runs["plain"][1] and runs["plain"][1]["stereo"] == 0 and runs["off"][2] == runs["plain"][2]
    assert runs["plain"][0]['metrics'] == runs["off"][0]['metrics']
    # with the report: the same bytes and the same launches of every other family
    assert runs["on"][2] == runs["plain"][2] and runs["on"][0]['metrics'] == runs["plain"][0]['metrics']
    assert _others(runs["on"][1]) == _others(runs["plain"][1]) and runs["on"][1]["stereo"] == 6
    with pytest.raises(ValueError, match="options of stereo_report=True"):
        sr.enhance_file(str(files / "stereo.wav"), str(tmp_path / "never.wav"), stereo_report_opts={'n_fft': 512})
    with pytest.raises(ValueError, match="not built for loudness_scope='folder'"):
        sr.enhance_folder(str(files), str(tmp_path / "never"), loudness='report', loudness_scope='folder', stereo_report=True)
    with pytest.raises(ValueError, match="stereo must be 'lr' or 'ms'"):
        SuperResolver(model, opt, stereo='mid')
    assert not os.path.exists(str(tmp_path / "never.wav")) and not os.path.exists(str(tmp_path / "never"))


# ------------------------------------------------------------------------------------------
# the mode
# ------------------------------------------------------------------------------------------
def test_the_mode_is_the_composition(resolvers):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan, stereo_matrix
    plain, ms = resolvers
    model, opt = _tiny()
    e = _excerpt()
    x = torch.stack([0.5 * e[4000:4000 + N] + 0.2 * e[9000:9000 + N], 0.5 * e[4000:4000 + N] - 0.3 * e[15000:15000 + N]]).to(DEV)
    S = segment_plan(N, opt.segment_length, 0.25)[0]
    noise = _noise(plain, 2 * S, 9)
    for kw in ({}, dict(crossover='input')):
        a, b = (plain, ms) if not kw else (SuperResolver(model, opt, **kw), SuperResolver(model, opt, stereo='ms', **kw))
        want = stereo_matrix(a.enhance_lr(stereo_matrix(x, 0.5), noise), 1.0, guard_side=True)
        b.enhance_lr(x, noise)                                      # (its own capture: a first use runs the chain once more)
        _counts(reset=True)
        base = a.enhance_lr(x, noise)
        counts_lr = _counts(reset=True)
        got = b.enhance_lr(x, noise)
        torch.cuda.synchronize()
        counts = _counts()
        assert counts["stereo"] == 2 and counts_lr["stereo"] == 0 and _others(counts) == _others(counts_lr)
        assert torch.isfinite(got).all() and torch.equal(got.view(torch.int32), want.view(torch.int32)), kw
        assert not torch.equal(got, base)                           # (mid and side are other clips than left and right)
    # one channel runs as ever, with no launch of the family; more than two are refused
    _counts(reset=True)
    assert torch.equal(ms.enhance_lr(x[:1], noise[:S]), plain.enhance_lr(x[:1], noise[:S])) and _counts()["stereo"] == 0
    with pytest.raises(ValueError, match="one or two channels, got 3"):
        ms.enhance_lr(torch.cat([x, x[:1]]), None)


def test_the_auto_crossover_still_measures_left_and_right():
    """Left carries a band up to 2.5 kHz, right one up to 1.2 kHz at a tenth of the level: of left / right as one programme the band
    ends at left's edge.  The clip is the composition with THAT plan: the measurement is not taken on mid / side."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver, crossover, crossover_auto_plan, crossover_coefficients, segment_plan, stereo_matrix
    model, opt = _tiny()
    plain = SuperResolver(model, opt)
    lr_auto = SuperResolver(model, opt, crossover='input', crossover_hz='auto')
    ms_auto = SuperResolver(model, opt, crossover='input', crossover_hz='auto', stereo='ms')
    x = torch.from_numpy(np.stack([brickwall_noise(N, RATE, 2500.0, 3), 0.1 * brickwall_noise(N, RATE, 1200.0, 4)]).astype(np.float32)).to(DEV)
    noise = _noise(plain, 2 * segment_plan(N, opt.segment_length, 0.25)[0], 9)
    lr_auto.enhance_lr(x, noise)
    ms_auto.enhance_lr(x, noise)                                    # (its own capture)
    _counts(reset=True)
    got = ms_auto.enhance_lr(x, noise)
    counts = _counts()
    assert counts["stereo"] == 2 and counts["bandwidth"] == 2 and counts["xover"] == 1
    assert ms_auto.last_crossover == lr_auto.last_crossover and ms_auto.last_crossover['edge_hz'] < 3000.0
    plan, _ = crossover_auto_plan(RATE, 8000, lr_auto.last_crossover['edge_hz'])
    enc = stereo_matrix(x, 0.5)
    want = stereo_matrix(crossover(plain.enhance_lr(enc, noise), enc, plain.gain / 2.0, crossover_coefficients(*plan).to(DEV)), 1.0, guard_side=True)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_dual_mono(dual, tmp_path):
    """The one test that needs the decoder's guard: the side signal of a dual-mono file is digital silence, whose group leaves the
    chain non-finite.  Written with stereo='ms' both channels are the same bytes, every sample is finite, and the clip is the mono
    run of the left channel under the same seed.  'lr' is run beside it: its channels are printed, not asserted."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    plain, ms = SuperResolver(model, opt), SuperResolver(model, opt, stereo='ms')
    torch.manual_seed(21)
    _counts(reset=True)
    res = ms.enhance_file(str(dual / "dual.wav"), str(tmp_path / "ms.wav"), channels='all', encoding='float32')
    assert _counts()["stereo"] == 2
    sr = res['sr']
    assert tuple(sr.shape) == (2, N) and torch.equal(res['lr'][0], res['lr'][1])
    assert torch.isfinite(sr).all()
    assert _same(sr[0], sr[1])
    words = np.frombuffer(_bytes(str(tmp_path / "ms.wav"))[-N * 8:], dtype="<f4").reshape(N, 2)
    assert np.isfinite(words).all() and np.array_equal(words[:, 0].view(np.int32), words[:, 1].view(np.int32))
    torch.manual_seed(21)
    mono = plain.enhance_file(str(dual / "left.wav"), str(tmp_path / "mono.wav"), encoding='float32')
    assert tuple(mono['sr'].shape) == (1, N) and _same(sr[0], mono['sr'][0]) and _same(sr[1], mono['sr'][0])
    torch.manual_seed(21)
    both = plain.enhance_file(str(dual / "dual.wav"), None, channels='all')['sr']
    d = (both[0] - both[1]).abs()
    print(f"dual mono with 'lr': max |L - R| = {float(d.max()):.4g} at a peak of {float(both.abs().max()):.4g}; with 'ms': {float((sr[0] - sr[1]).abs().max()):.4g}")


# ------------------------------------------------------------------------------------------
# the report
# ------------------------------------------------------------------------------------------
def _check_clip(fig, rows, plan=None):
    """The figures the report gives for a clip against the restatement on the returned clip: inside the interval the cross-spectrum's
    bound (tests/test_gpu_stereo.py), summed over the band, leaves each figure."""
    p = dict(SR.DEFAULTS, **(plan or {}))
    x = rows.cpu().numpy().astype(np.float64)
    want_fig, want = SR.image_ref(x, RATE, 8000, p['n_fft'], p['hop'])
    k = SR.split_bin_ref(RATE, 8000, p['n_fft'])
    _, tol = _xspec_bound(x, p['n_fft'], p['hop'])
    box = SR.figure_intervals(want, np.concatenate([tol[:, :k].sum(axis=1), tol[:, k:].sum(axis=1)]) * (1.0 + 1e-9))
    assert sorted(fig) == ['high', 'low']
    for band in ('low', 'high'):
        assert sorted(fig[band]) == ['balance_db', 'coherence', 'corr', 'side_db']
        for key, (lo, hi) in box[band].items():
            print(f"  {band} {key}: report {fig[band][key]}, restatement {want_fig[band][key]}, interval [{lo}, {hi}]")
            assert fig[band][key] is not None and lo <= fig[band][key] <= hi, (band, key, fig[band][key], lo, hi)


def test_report_is_the_restatement_on_the_returned_clips(resolvers, files, tmp_path):
    plain, ms = resolvers
    plain.enhance_file(str(files / "stereo.wav"), None, channels='all')      # capture, tables, packed weights
    outs = {}
    for name, sr, launches in (("lr", plain, 6), ("ms", ms, 8)):
        torch.manual_seed(5)
        _counts(reset=True)
        res = sr.enhance_file(str(files / "stereo.wav"), str(tmp_path / (name + ".wav")), channels='all', stereo_report=True)
        assert _counts()["stereo"] == launches                     # three clips, two launches each; the mode's two
        assert sorted(res) == sorted(KEYS + ['stereo']) and res['hr'] is not None
        s = res['stereo']
        assert sorted(s) == STEREO_KEYS
        assert s['split_hz'] == 171 * 48000 / 2048 and (s['n_fft'], s['hop'], s['mode']) == (2048, 1024, name)
        assert s['frames'] == frames_ref(N, 2048, 1024) == 6 and isinstance(s['notes'], list) and (name == 'lr' or s['notes'] == [])
        for key, rows in (('input', res['lr']), ('output', res['sr']), ('original', res['hr'])):
            print(f"{name} {key}:")
            _check_clip(s[key], rows)
        if s['notes']:
            assert s['output']['high']['corr'] < s['output']['low']['corr'] - 0.3 and "stereo='ms'" in s['notes'][0]
        print(f"{name}: output corr below / above the split {s['output']['low']['corr']:+.3f} / {s['output']['high']['corr']:+.3f}; "
              f"input {s['input']['low']['corr']:+.3f} / {s['input']['high']['corr']:+.3f}; original {s['original']['low']['corr']:+.3f} / "
              f"{s['original']['high']['corr']:+.3f}; notes {len(s['notes'])}")
        # the same figures on a second run
        torch.manual_seed(5)
        assert sr.enhance_file(str(files / "stereo.wav"), None, channels='all', stereo_report=True)['stereo'] == s
        outs[name] = res
    assert outs["lr"]['stereo']['input'] == outs["ms"]['stereo']['input'] and outs["lr"]['stereo']['original'] == outs["ms"]['stereo']['original']
    # other options of the plan
    torch.manual_seed(5)
    other = plain.enhance_file(str(files / "stereo.wav"), None, channels='all', stereo_report=True, stereo_report_opts={'n_fft': 512})['stereo']
    assert (other['n_fft'], other['hop'], other['frames'], other['split_hz']) == (512, 256, frames_ref(N, 512, 256), 43 * 48000 / 512)
    _check_clip(other['input'], outs["lr"]['lr'], {'n_fft': 512, 'hop': 256})
    # a file written with another channel count: the key, None, no launch
    _counts(reset=True)
    for name, channels in (("mono.wav", 'all'), ("stereo.wav", 'first'), ("three.wav", 'all')):
        res = plain.enhance_file(str(files / name), None, channels=channels, stereo_report=True)
        assert sorted(res) == sorted(KEYS + ['stereo']) and res['stereo'] is None
    assert _counts()["stereo"] == 0


# ------------------------------------------------------------------------------------------
# folders, the album pipeline, the command line
# ------------------------------------------------------------------------------------------
def test_folders(resolvers, files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_STEREO, write_metrics_csv
    plain, ms = resolvers
    recs = plain.enhance_folder(str(files), str(tmp_path / "lr"), channels='all', seed=11, stereo_report=True)
    by = {r['path']: r for r in recs}
    assert sorted(by) == ["mono.wav", "stereo.wav", "three.wav"] and all(r['error'] is None for r in recs)
    assert by["mono.wav"]['stereo'] is None and by["three.wav"]['stereo'] is None and sorted(by["stereo.wav"]['stereo']) == STEREO_KEYS
    torch.manual_seed(11)
    one = plain.enhance_file(str(files / "stereo.wav"), str(tmp_path / "one.wav"), channels='all', stereo_report=True)
    assert by["stereo.wav"]['stereo'] == one['stereo'] and _bytes(str(tmp_path / "lr" / "stereo.wav")) == _bytes(str(tmp_path / "one.wav"))
    write_metrics_csv(str(tmp_path / "on.csv"), recs, stereo=True)
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == METRICS_COLUMNS + METRICS_COLUMNS_STEREO and len(rows) == 1 + 6 + 1
    s = one['stereo']
    want = [s['output']['low']['corr'], s['output']['high']['corr'], s['original']['high']['corr'], s['output']['high']['side_db']]
    assert [[float(v) for v in row[-4:]] for row in rows if row[0] == "stereo.wav"] == [want, want] and [float(v) for v in rows[-1][-4:]] == want
    assert all(np.isnan(float(v)) for row in rows[1:-1] if row[0] != "stereo.wav" for v in row[-4:])
    # 'ms': the three-channel file is skipped with its reason, the others are written; the mono file as with 'lr'
    _counts(reset=True)
    recs = ms.enhance_folder(str(files), str(tmp_path / "ms"), channels='all', seed=11)
    assert _counts()["stereo"] == 2
    by_ms = {r['path']: r for r in recs}
    assert by_ms["three.wav"]['error'] is not None and "stereo='ms' takes one or two channels, 3 would be written" in by_ms["three.wav"]['error']
    assert by_ms["mono.wav"]['error'] is None and by_ms["stereo.wav"]['error'] is None and not os.path.exists(str(tmp_path / "ms" / "three.wav"))
    assert os.path.exists(str(tmp_path / "lr" / "three.wav"))
    assert _bytes(str(tmp_path / "ms" / "mono.wav")) == _bytes(str(tmp_path / "lr" / "mono.wav"))
    assert _bytes(str(tmp_path / "ms" / "stereo.wav")) != _bytes(str(tmp_path / "lr" / "stereo.wav"))
    assert all('stereo' not in r for r in recs)
    # the first two channels of it are fine
    assert all(r['error'] is None for r in ms.enhance_folder(str(files), str(tmp_path / "ms2"), channels=2, seed=11))


def test_the_album_pipeline_inherits_the_mode(resolvers, files, tmp_path):
    plain, ms = resolvers
    _counts(reset=True)
    recs = ms.enhance_folder(str(files), str(tmp_path / "album"), channels='all', seed=11, loudness=-23.0, loudness_scope='folder')
    assert _counts()["stereo"] == 2
    by = {r['path']: r for r in recs}
    assert by["three.wav"]['error'] is not None and "one or two channels" in by["three.wav"]['error'] and by["three.wav"]['album'] is None
    assert by["mono.wav"]['error'] is None and by["stereo.wav"]['error'] is None and by["stereo.wav"]['album']['files'] == 2
    # the written stereo file is the mode's clip times the album's gain: another file than 'lr' writes, the mono file aside
    ref = plain.enhance_folder(str(files), str(tmp_path / "album_lr"), channels=2, seed=11, loudness=-23.0, loudness_scope='folder')
    assert all(r['error'] is None for r in ref)
    assert _bytes(str(tmp_path / "album" / "stereo.wav")) != _bytes(str(tmp_path / "album_lr" / "stereo.wav"))
    with pytest.raises(ValueError, match="not built for loudness_scope='folder'"):
        ms.enhance_folder(str(files), str(tmp_path / "never"), loudness=-23.0, loudness_scope='folder', stereo_report=True)
    assert not os.path.exists(str(tmp_path / "never"))


def test_cli_lines_and_csv_columns(files, tmp_path, capsys):
    """Without the options main() prints the lines and writes the columns of the parent; with --stereo_report one `stereo correlation`
    line per two-channel file, one per note, and four columns more, holding what enhance_file returns; --stereo ms adds the start-up
    line."""
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
    base = ["--input", str(files / "stereo.wav"), "--load_pretrain", str(folder), "--encoding", "float32", "--channels", "all"]
    _counts(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "off.wav"), "--metrics_csv", str(tmp_path / "off.csv")]) == 0
    assert _counts()["stereo"] == 0
    off = capsys.readouterr().out.splitlines()
    assert not any("stereo" in l.replace("stereo.wav", "") or "note" in l for l in off)
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(G.METRICS_COLUMNS)
    _counts(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--metrics_csv", str(tmp_path / "on.csv"), "--stereo_report"]) == 0
    assert _counts()["stereo"] == 6
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if ": stereo correlation " in l or ": note: " in l]
    assert [l.replace("on.wav", "off.wav").replace("on.csv", "off.csv") for l in on if l not in extra] == off
    num = r"([+-]\d\.\d\d)"
    m = re.fullmatch(re.escape(str(tmp_path / "on.wav")) + r": stereo correlation below / above 4\.01 kHz: input %s / %s, output %s / %s, original %s / %s"
                     % ((num,) * 6), extra[0])
    assert m, extra[0]
    assert len(extra) in (1, 2)                                    # (the note depends on the figures: random weights)
    assert all(": note: " in l and "--stereo ms" in l for l in extra[1:])
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == G.METRICS_COLUMNS + G.METRICS_COLUMNS_STEREO and len(rows) == 4
    assert ["%+.2f" % float(v) for v in rows[1][-4:-1]] == [m.group(3), m.group(4), m.group(6)] and rows[2][-4:] == rows[1][-4:] == rows[3][-4:]
    assert [r[:-4] for r in rows] == list(csv.reader(open(str(tmp_path / "off.csv")))) and _bytes(str(tmp_path / "on.wav")) == _bytes(str(tmp_path / "off.wav"))
    # folder mode with --stereo ms: the start-up line, one report line (the two-channel file's), the skipped file with its reason
    _counts(reset=True)
    assert G.main(["--input", str(files), "--output", str(tmp_path / "dir"), "--load_pretrain", str(folder), "--channels", "all", "--stereo", "ms",
                   "--stereo_report", "--stereo_n_fft", "512"]) == 0
    assert _counts()["stereo"] == 8
    lines = capsys.readouterr().out.splitlines()
    assert lines.count("stereo: mid / side") == 1 and sum(": stereo correlation below / above 4.03 kHz: " in l for l in lines) == 1
    assert any(l.startswith("skipped three.wav: ") and "stereo='ms' takes one or two channels" in l for l in lines)
    assert not any(": note: " in l for l in lines) and "2 of 3 files enhanced, 1 skipped" in lines
    # an option of --stereo_report: the parser's error, before anything is loaded
    with pytest.raises(SystemExit):
        G.main(base + ["--output", str(tmp_path / "no.wav"), "--stereo_hop", "64"])
    assert "--stereo_hop is an option of --stereo_report" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "no.wav"))
