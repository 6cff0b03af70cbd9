"""enhance_folder(loudness_scope='folder') / --loudness_scope folder on the GPU: a one-file folder comes out as the per-file run
writes it; a three-file folder gets one gain, its written files -- re-read and measured as one programme by the restatement of
tests/_loudness_album_ref.py -- sit at the target and keep their level differences; one guard gain holds the folder's largest true
peak at the ceiling; clip='error' writes nothing; the cache, graphs, 'report', skipped files, the command line and the table.  The
tiny model and the excerpt clip are those of tests/test_gpu_generate_loudness.py, restated."""
import csv
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _loudness_album_ref as AR
import _loudness_ref as R
import _truepeak_ref as TR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE = 48000
NAMES = ("a_loud.wav", "b_stereo.wav", "c_quiet.wav")              # the plan's order
KEYS = ['gain_db', 'input', 'measured', 'momentary_max', 'output', 'target']
ALBUM_KEYS = ['blocks_in', 'blocks_out', 'files', 'gain_db', 'input', 'kept', 'measured', 'output', 'target']


def _opt(**kw):
    o = dict(gpu_ids=[0], isTrain=True, checkpoints_dir="/tmp/p2phd_test_ckpt", name="t", model="pix2pixHD",
             input_nc=2, output_nc=2, label_nc=0, hr_sampling_rate=RATE, lr_sampling_rate=8000,
             n_fft=64, hop_length=32, win_length=64, center=True, no_instance=True, ngf=8, netG="local",
             n_downsample_global=2, n_blocks_global=2, n_local_enhancers=1, n_blocks_local=1, norm="instance",
             no_lsgan=False, ndf=8, n_layers_D=3, num_D=2, no_ganFeat_loss=False, use_hifigan_D=False, use_time_D=False,
             verbose=False, continue_train=False, load_pretrain="", which_epoch="latest", pool_size=0, lr=0.0002,
             beta1=0.5, no_vgg_loss=True, use_match_loss=False, niter_fix_global=0, explicit_encoding=True, alpha=0.6,
             min_value=1e-7, mask=True, mask_mode="mode2", phase_encoding_mode=None, lambda_feat=10.0, fp16=False, niter_decay=100,
             instance_feat=False, label_feat=False, segment_length=31 * 32, batchSize=2)
    o.update(kw)
    return SimpleNamespace(**o)


_MODELS = {}


def _tiny(mdct_type="mdct4"):
    if mdct_type not in _MODELS:
        from pix2pixhdaudiosr_amd.models.models import create_model
        opt = _opt(mdct_type=mdct_type)
        torch.manual_seed(1234)
        model = create_model(opt)
        model.eval()
        _MODELS[mdct_type] = (model, opt)
    return _MODELS[mdct_type]


def _clip(hops=7):
    """0.1 s hops of the stored excerpt (0.5 s), forwards and then backwards: long enough for a few 400 ms blocks."""
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    x = torch.from_numpy(F["test_wav_excerpt_i16"].astype(np.float32) / 32768.0)
    return torch.cat([x, 0.7 * x.flip(0)])[:hops * (RATE // 10) + 321]


def _count(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(b"loudness", 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _written(path):
    from pix2pixhdaudiosr_amd.data import wavio
    data, rate = wavio.load(str(path))
    assert rate == RATE
    return data.numpy()


def _wavs(folder):
    return sorted(os.path.relpath(os.path.join(d, f), str(folder)) for d, _, fs in os.walk(str(folder)) for f in fs if f.endswith(".wav"))


def _same_files(a, b, names=NAMES):
    return _wavs(a) == _wavs(b) == sorted(names) and all(_bytes(os.path.join(str(a), n)) == _bytes(os.path.join(str(b), n)) for n in names)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Three files: the clip at 0.5, a stereo file that is the loudest and has the largest peak, the clip at 0.05."""
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("album_in")
    x = _clip()
    n = 5 * 4800 + 77
    wavio.save(str(d / NAMES[0]), 0.5 * x, RATE)
    wavio.save(str(d / NAMES[1]), torch.stack([0.8 * x[:n], -0.5 * x.flip(0)[:n]]), RATE)
    wavio.save(str(d / NAMES[2]), 0.05 * x, RATE)
    return d


@pytest.fixture(scope="module")
def one_file(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("album_one")
    x = _clip()
    n = 5 * 4800 + 77
    wavio.save(str(d / "only.wav"), torch.stack([0.8 * x[:n], -0.5 * x.flip(0)[:n]]), RATE)
    return d


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    return SuperResolver(model, opt, crossover='input')


def _run(resolver, src, dst, **kw):
    kw.setdefault('channels', 'all')
    kw.setdefault('seed', 11)
    kw.setdefault('encoding', 'float32')
    return resolver.enhance_folder(str(src), str(dst), **kw)


@pytest.fixture(scope="module")
def plain(resolver, files, tmp_path_factory):
    """The run without the option: the unscaled clips (float32 files hold them bit for bit) and the metrics."""
    out = tmp_path_factory.mktemp("album_plain")
    _count(reset=True)
    recs = _run(resolver, files, out)
    assert _count() == 0 and all('loudness' not in r and 'album' not in r for r in recs)
    return recs, out, [_written(out / n) for n in NAMES]


@pytest.fixture(scope="module")
def album(resolver, files, plain, tmp_path_factory):
    """The three-file folder at -23 LUFS, scope 'folder', with its launch count."""
    out = tmp_path_factory.mktemp("album_on")
    _count(reset=True)
    recs = _run(resolver, files, out, loudness=-23.0, loudness_scope='folder')
    return recs, out, _count()


def _levels(clips):
    """Per file the restatement's gating of its own blocks, and the album's over the union."""
    zs = [R.hop_energies(y, RATE) for y in clips]
    own = [R.gating(z, RATE) for z in zs]
    return own, AR.album_gating(AR.album_blocks(zs, RATE))


@pytest.mark.parametrize("case", ["target", "input", "guard"])
def test_a_one_file_folder_is_the_per_file_run(resolver, one_file, tmp_path, case):
    kw = {'target': dict(loudness=-23.0), 'input': dict(loudness='input'),
          'guard': dict(loudness=-23.0, clip='guard', true_peak=True, ceiling_dbfs=-1.0, encoding='pcm16')}[case]
    a = _run(resolver, one_file, tmp_path / "file", **kw)
    b = _run(resolver, one_file, tmp_path / "folder", loudness_scope='folder', **kw)
    assert _same_files(tmp_path / "file", tmp_path / "folder", ("only.wav",))
    assert b[0]['loudness'] == a[0]['loudness'] and b[0].get('output') == a[0].get('output')
    alb = b[0]['album']
    assert sorted(alb) == ALBUM_KEYS and alb['files'] == 1 and alb['blocks_out'] == 2 and alb['blocks_in'] == 2
    assert (alb['input'], alb['measured'], alb['gain_db'], alb['output']) == tuple(a[0]['loudness'][k] for k in ('input', 'measured', 'gain_db', 'output'))


def test_three_files_get_one_gain_and_the_album_sits_at_the_target(resolver, files, plain, album, tmp_path):
    recs0, _, clips0 = plain
    recs, out, launches = album
    assert launches == 6 * 3 + 2
    assert [r['path'] for r in recs] == list(NAMES) and all(r['error'] is None for r in recs)
    alb = recs[0]['album']
    assert sorted(alb) == ALBUM_KEYS and all(r['album'] is alb for r in recs)
    assert alb['files'] == 3 and alb['target'] == -23.0 and alb['output'] == alb['measured'] + alb['gain_db'] and abs(alb['output'] - (-23.0)) <= 1e-5
    assert all(sorted(r['loudness']) == KEYS and r['loudness']['gain_db'] == alb['gain_db'] and r['loudness']['target'] == -23.0 for r in recs)
    assert all(r['loudness']['output'] == r['loudness']['measured'] + alb['gain_db'] for r in recs)
    assert all('output' not in r for r in recs)                    # no output stage was asked for
    gain_db = alb['gain_db']
    # the test would show nothing if the per-file gains were alike
    per_file = _run(resolver, files, tmp_path / "per_file", loudness=-23.0)
    gains = [r['loudness']['gain_db'] for r in per_file]
    print("per-file gains %s dB, album gain %+.4f dB" % (np.round(gains, 3), gain_db))
    assert min(abs(a - b) for i, a in enumerate(gains) for b in gains[i + 1:]) > 0.5
    assert [r['loudness']['measured'] for r in recs] == [r['loudness']['measured'] for r in per_file]     # the track figures are the file path's
    assert [r['loudness']['input'] for r in recs] == [r['loudness']['input'] for r in per_file]
    # the precondition of the level checks, on the unscaled clips: the gates cannot move when the gain is applied
    own0, whole0 = _levels(clips0)
    print("unscaled: album %.4f LUFS, gamma %.4f, kept %d; files %s" % (whole0['I'], whole0['gamma'], whole0['kept'], [np.round(g['l'], 2) for g in own0]))
    assert abs(gain_db) <= 20.0
    for g in own0[:2]:
        assert len(g['l']) >= 2 and g['l'].min() > -50.0
    quiet = own0[2]['l']
    assert len(quiet) >= 2 and quiet.max() < whole0['gamma'] - 1.0 and quiet.min() > -69.0 and (quiet + gain_db).min() > -69.0
    assert (quiet + gain_db).max() < whole0['gamma'] + gain_db - 1.0
    assert np.abs(whole0['l'] - whole0['gamma']).min() > 0.01 and alb['kept'] == whole0['kept'] >= 2
    assert alb['blocks_out'] == sum(len(g['l']) for g in own0) and alb['blocks_in'] == alb['blocks_out']
    assert abs(alb['measured'] - whole0['I']) <= 0.001
    # the written files as one programme
    clips = [_written(out / n) for n in NAMES]
    own, whole = _levels(clips)
    print("written: album %.6f LUFS; files %s" % (whole['I'], [g['I'] for g in own]))
    assert abs(whole['I'] - (-23.0)) <= 0.001
    g32 = np.float32(10.0 ** (gain_db / 20.0))
    for y, y0 in zip(clips, clips0):
        assert y.shape == y0.shape and np.abs(y - y0 * g32).max() <= 1e-6 * np.abs(y).max()
    # the level differences between the files are those of the unscaled clips
    for i in range(3):
        for j in range(i + 1, 3):
            assert abs((own[i]['I'] - own[j]['I']) - (own0[i]['I'] - own0[j]['I'])) <= 0.002
    # ... which the per-file run gives away
    assert abs(own0[0]['I'] - own0[2]['I']) > 15.0
    # the metrics are the unscaled clips'
    assert [r['metrics'] for r in recs] == [r['metrics'] for r in recs0]
    # the album of the inputs the generator was given
    zs_in = []
    for n in NAMES:
        res = resolver.enhance_file(str(files / n), None, channels='all')
        zs_in.append(R.hop_energies(res['lr'].cpu().numpy(), RATE))
    assert abs(alb['input'] - AR.album_gating(AR.album_blocks(zs_in, RATE))['I']) <= 0.001


def _over_the_limit(plain, album):
    """The target at which the loudest file's largest sample is over 1 and the first file's is under it, half way between in dB."""
    _, _, clips0 = plain
    peaks = [float(np.abs(y).max()) for y in clips0]
    assert peaks[1] > 1.2 * peaks[0] > 6.0 * peaks[2]
    target = album[0][0]['album']['measured'] - 10.0 * math.log10(peaks[0] * peaks[1])
    assert -70.0 <= target <= 0.0 and abs(target - album[0][0]['album']['measured']) <= 40.0
    return target, peaks


def test_one_guard_gain_holds_the_largest_true_peak_at_the_ceiling(resolver, files, plain, album, tmp_path):
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients, truepeak_plan
    plan = truepeak_plan(RATE)
    table = true_peak_coefficients(plan['factor'], plan['taps_per_phase'], plan['beta']).numpy()
    target, _ = _over_the_limit(plain, album)
    ceiling = 10.0 ** (-1.0 / 20.0)
    recs = _run(resolver, files, tmp_path / "g", loudness=target, loudness_scope='folder', clip='guard', true_peak=True, ceiling_dbfs=-1.0,
                encoding='pcm16')
    guard = recs[0]['output']['gain']
    assert guard < 1.0 and all(r['output']['gain'] == guard for r in recs)
    tps = [max(r['output']['true_peak']) for r in recs]
    assert tps[1] == max(tps) > ceiling > tps[0]                   # only the loudest file is over the ceiling: one gain for all the same
    assert guard == float(TR.gain([max(tps)], ceiling))
    clips = [_written(tmp_path / "g" / n) for n in NAMES]
    margin = max(TR.dot_bound(y, table).max() for y in clips) + 0.5 * 2.0 ** -15 * np.abs(table.astype(np.float64)).sum(axis=1).max()
    got = [TR.true_peak(y, table).max() for y in clips]
    print("written true peaks %s, ceiling %.9f, margin %.3e, guard %r" % (got, ceiling, margin, guard))
    assert abs(max(got) - ceiling) <= margin and got[1] == max(got)
    own0, whole0 = _levels(plain[2])
    total_db = recs[0]['album']['gain_db'] + 20.0 * math.log10(guard)
    assert abs(total_db) <= 20.0 and all(g['l'].min() + min(total_db, 0.0) > -69.0 for g in own0)       # no block crosses the absolute gate
    _, whole = _levels(clips)
    print("written album %.6f LUFS, target %.4f, guard %.4f dB" % (whole['I'], target, 20.0 * math.log10(guard)))
    assert abs(whole['I'] - (target + 20.0 * math.log10(guard))) <= 0.001


def test_clip_error_writes_no_file_at_all(resolver, files, plain, album, tmp_path):
    from pix2pixhdaudiosr_amd.generate import ClipError
    target, _ = _over_the_limit(plain, album)
    seen = _run(resolver, files, tmp_path / "seen", loudness=target, loudness_scope='folder', report_peaks=True)
    assert [sum(r['output']['clipped']) > 0 for r in seen] == [False, True, False]      # the precondition: the second file alone
    reported = []
    with pytest.raises(ClipError) as e:
        _run(resolver, files, tmp_path / "e", loudness=target, loudness_scope='folder', clip='error', report=reported.append)
    assert os.path.join(str(tmp_path / "e"), NAMES[1]) in str(e.value) and "would clip" in str(e.value)
    assert _wavs(tmp_path / "e") == [] and reported == []


def test_cache_off_and_eager_runs_write_the_same_bytes(files, album, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    recs, out, _ = album
    model, opt = _tiny()
    for name, graph, kw in (("nocache", True, dict(album_cache_bytes=0)), ("eager", False, {}), ("small", True, dict(album_cache_bytes=200000))):
        sr = SuperResolver(model, opt, graph=graph, crossover='input')
        got = _run(sr, files, tmp_path / name, loudness=-23.0, loudness_scope='folder', **kw)
        assert _same_files(out, tmp_path / name), name
        assert [r['loudness'] for r in got] == [r['loudness'] for r in recs] and got[0]['album'] == recs[0]['album']


def test_report_mode_writes_the_plain_bytes_and_fills_the_album(resolver, files, plain, album, tmp_path):
    _, out0, _ = plain
    recs = _run(resolver, files, tmp_path / "r", loudness='report', loudness_scope='folder')
    assert _same_files(out0, tmp_path / "r")
    alb, ref = recs[0]['album'], album[0][0]['album']
    assert alb['gain_db'] == 0.0 and alb['target'] is None and alb['output'] == alb['measured'] == ref['measured'] and alb['input'] == ref['input']
    assert all(r['loudness']['gain_db'] == 0.0 and r['loudness']['output'] == r['loudness']['measured'] for r in recs)
    # 'input': the album of the written files is as loud as the album of the inputs
    recs = _run(resolver, files, tmp_path / "i", loudness='input', loudness_scope='folder')
    alb = recs[0]['album']
    assert alb['target'] == alb['input'] == ref['input'] and abs(alb['output'] - alb['input']) <= 1e-5 and abs(alb['gain_db']) <= 20.0
    _, whole = _levels([_written(tmp_path / "i" / n) for n in NAMES])
    assert abs(whole['I'] - alb['input']) <= 0.001


def test_skipped_files_and_an_empty_folder(resolver, files, album, tmp_path):
    import shutil
    src = tmp_path / "in"
    shutil.copytree(str(files), str(src))
    (src / "b_broken.wav").write_bytes(b"RIFF not a wav file at all")
    seen = []
    _count(reset=True)
    recs = _run(resolver, src, tmp_path / "out", loudness=-23.0, loudness_scope='folder', report=seen.append)
    assert _count() == 6 * 3 + 2
    assert [r['path'] for r in recs] == ["a_loud.wav", "b_broken.wav", "b_stereo.wav", "c_quiet.wav"] and seen == recs
    bad = recs[1]
    assert bad['error'] is not None and bad['loudness'] is None and bad['album'] is None and bad['written_channels'] == 0
    assert _same_files(album[1], tmp_path / "out") and recs[0]['album'] == album[0][0]['album'] and recs[0]['album']['files'] == 3
    # nothing to enhance: no launch, no file
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "x.wav").write_bytes(b"")
    _count(reset=True)
    recs = _run(resolver, empty, tmp_path / "none", loudness=-23.0, loudness_scope='folder')
    assert _count() == 0 and len(recs) == 1 and recs[0]['error'] is not None and recs[0]['album'] is None and _wavs(tmp_path / "none") == []
    (empty / "x.wav").unlink()
    assert _run(resolver, empty, tmp_path / "none", loudness=-23.0, loudness_scope='folder') == [] and _count() == 0


def _both_scopes(sr, src, dst):
    kw = dict(loudness=-23.0, extended_metrics=True, input_formats=('wav',))
    return _run(sr, src, dst / "file", **kw), _run(sr, src, dst / "folder", loudness_scope='folder', **kw)


def test_both_scopes_leave_the_same_record_of_a_file(one_file, tmp_path):
    """Everything a record carries in either scope -- the metrics, the clip's crossover and normalisation ranges, the written path --
    is the same at scope 'file' and at scope 'folder', key for key and in the same order, for an enhanced file and for a skipped one."""
    import shutil
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    sr = SuperResolver(model, opt, crossover='input', crossover_hz='auto', norm_scope='clip')

    def same(file_rec, folder_rec):
        assert [k for k in folder_rec if k != 'album'] == list(file_rec) and 'album' in folder_rec
        assert {'metrics_ext', 'loudness', 'crossover', 'written', 'norm'} <= set(file_rec)

    a, b = _both_scopes(sr, one_file, tmp_path / "one")
    assert len(a) == len(b) == 1 and a[0]['error'] is None and b[0]['error'] is None
    same(a[0], b[0])
    for key in ('metrics', 'metrics_ext', 'crossover', 'written'):
        assert a[0][key] is not None and b[0][key] == a[0][key], key
    assert a[0]['norm'].shape == (2, 2) and torch.equal(b[0]['norm'], a[0]['norm'])
    assert _same_files(tmp_path / "one" / "file", tmp_path / "one" / "folder", ("only.wav",))
    # beside a file of garbage bytes: the skipped record has the same keys in both scopes, and the enhanced file does not move
    src = tmp_path / "in"
    shutil.copytree(str(one_file), str(src))
    (src / "broken.wav").write_bytes(b"RIFF not a wav file at all")
    c, d = _both_scopes(sr, src, tmp_path / "two")
    assert [r['path'] for r in c] == [r['path'] for r in d] == ["broken.wav", "only.wav"]
    same(c[0], d[0])
    same(c[1], d[1])
    assert c[0]['error'] is not None and d[0]['error'] == c[0]['error'] and d[0]['album'] is None
    assert {k: v for k, v in d[0].items() if k != 'album'} == c[0]
    for key in ('metrics', 'metrics_ext', 'crossover', 'written'):
        assert d[1][key] == c[1][key] == a[0][key], key
    assert torch.equal(d[1]['norm'], c[1]['norm']) and torch.equal(c[1]['norm'], a[0]['norm'])
    assert _same_files(tmp_path / "two" / "file", tmp_path / "two" / "folder", ("only.wav",))
    assert _bytes(str(tmp_path / "two" / "file" / "only.wav")) == _bytes(str(tmp_path / "one" / "file" / "only.wav"))


def test_dither_takes_the_seed_of_the_files_place_in_the_plan(resolver, files, tmp_path):
    """pcm16 with dither: file k is dithered with seed + k, as the per-file scope does it -- a one-file folder holding the plan's
    third file, dithered with seed + 2, is that file of the three-file run when both get the same gains ('report', clamp)."""
    import shutil
    kw = dict(loudness='report', loudness_scope='folder', encoding='pcm16', dither='tpdf')
    _run(resolver, files, tmp_path / "three", dither_seed=40, **kw)
    src = tmp_path / "in"
    src.mkdir()
    shutil.copy(str(files / NAMES[2]), str(src / NAMES[2]))
    _run(resolver, src, tmp_path / "one", dither_seed=42, **kw)
    assert _bytes(str(tmp_path / "one" / NAMES[2])) == _bytes(str(tmp_path / "three" / NAMES[2]))
    _run(resolver, src, tmp_path / "other", dither_seed=40, **kw)
    assert _bytes(str(tmp_path / "other" / NAMES[2])) != _bytes(str(tmp_path / "three" / NAMES[2]))


def test_refused_combinations(resolver, files, tmp_path):
    out = tmp_path / "never"
    for kw, message in ((dict(loudness_scope='folder'), "is an option of loudness"),
                        (dict(loudness=-23.0, loudness_scope='folder', clip='guard', limiter=True), "limiter is not built"),
                        (dict(loudness=-23.0, loudness_scope='folder', loudness_range=True), "loudness_range is not built"),
                        (dict(loudness=-23.0, loudness_scope='folder', spectrogram=str(tmp_path / "png")), "spectrogram is not built"),
                        (dict(loudness=-23.0, album_cache_bytes=0), "album_cache_bytes is an option of")):
        with pytest.raises(ValueError, match=message):
            _run(resolver, files, out, **kw)
    with pytest.raises(ValueError, match="option of folder mode"):
        resolver.enhance_file(str(files / NAMES[0]), str(tmp_path / "never.wav"), loudness=-23.0, loudness_scope='folder')
    assert not out.exists() and not (tmp_path / "never.wav").exists() and not (tmp_path / "png").exists()


def test_cli_line_and_csv_row(files, tmp_path, capsys):
    from pix2pixhdaudiosr_amd import generate as G
    from pix2pixhdaudiosr_amd.models.models import create_model
    common = dict(mdct_type="mdct4", checkpoints_dir=str(tmp_path), name="run", seed=11)
    torch.manual_seed(1234)
    create_model(_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:                       # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    base = ["--input", str(files), "--load_pretrain", str(folder), "--encoding", "float32", "--crossover", "input", "--channels", "all",
            "--loudness", "-23"]
    assert G.main(base + ["--output", str(tmp_path / "file"), "--metrics_csv", str(tmp_path / "file.csv")]) == 0
    off = capsys.readouterr().out.splitlines()
    assert not any(l.startswith("album:") for l in off)
    _count(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "folder"), "--metrics_csv", str(tmp_path / "folder.csv"), "--loudness_scope", "folder"]) == 0
    assert _count() == 6 * 3 + 2
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if l.startswith("album:")]
    assert len(extra) == 1 and len(on) == len(off) + 1 and on.index(extra[0]) == on.index("3 of 3 files enhanced, 0 skipped") - 1
    m = re.fullmatch(r"album: loudness input ([-+]\d+\.\d\d) LUFS, measured ([-+]\d+\.\d\d) LUFS, gain ([-+]\d+\.\d\d) dB -> -23\.00 LUFS "
                     r"\(3 files, (\d+) blocks\)", extra[0])
    rows_off, rows_on = (list(csv.reader(open(str(tmp_path / n)))) for n in ("file.csv", "folder.csv"))
    level_in, level_out, gain_db = (float(v) for v in rows_on[-1][-3:])
    assert m and m.groups() == ("%+.2f" % level_in, "%+.2f" % (level_out - gain_db), "%+.2f" % gain_db, "10")     # 4 + 2 + 4 blocks
    assert abs(level_out - (-23.0)) <= 1e-5
    _, whole = _levels([_written(tmp_path / "folder" / n) for n in NAMES])
    assert abs(whole['I'] - (-23.0)) <= 0.001
    # one line per file, each with the album's gain
    lines = [l for l in on if ": loudness input " in l and not l.startswith("album:")]
    assert len(lines) == 3 and all(l.endswith("gain %+.2f dB" % gain_db) for l in lines)
    assert rows_on[0] == rows_off[0] == list(G.METRICS_COLUMNS + G.METRICS_COLUMNS_LOUDNESS)
    assert [r[0] for r in rows_off] == ["file"] + [NAMES[0], NAMES[1], NAMES[1], NAMES[2], "mean"]
    assert [r[0] for r in rows_on] == [r[0] for r in rows_off] + ["album"]
    assert rows_on[-1][:7] == ["album"] + [""] * 6 and len(rows_on[-1]) == 10
    assert [r[:7] for r in rows_on[1:-2]] == [r[:7] for r in rows_off[1:-1]]       # the metrics are the unscaled clips'
    assert all(float(r[-1]) == gain_db for r in rows_on[1:-2])
    with pytest.raises(SystemExit):
        G.main(["--input", str(files / NAMES[0]), "--output", str(tmp_path / "no.wav"), "--load_pretrain", str(folder), "--loudness", "-23",
                "--loudness_scope", "folder"])
    assert not os.path.exists(str(tmp_path / "no.wav"))
