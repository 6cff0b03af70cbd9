"""enhance_file(limiter=True) / enhance_folder(limiter=True) on the GPU: a clip brought to a loudness target that leaves its true
peak 4 dB over a -1 dBTP ceiling is written with its true peak at the ceiling and nearly all of its loudness, where the guard
alone gives 4 dB away; the written loudness is what the float64 restatement of tests/_limiter_ref.py predicts; a clip that fits is
written byte for byte as the guard writes it; without the option nothing changes and nothing is launched; folders and the CSV
columns.  float32 encoding throughout, so that quantisation stays out of the comparisons.  The tiny model and the crossover='input'
resolver are those of tests/test_gpu_generate_truepeak.py, restated."""
import csv
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _limiter_ref as LR
import _loudness_ref as LOUD
import _truepeak_ref as TP
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE = 48000
CEILING_DB = -1.0
CEILING = 10.0 ** (CEILING_DB / 20.0)
OUTPUT_KEYS = ['clipped', 'gain', 'nonfinite', 'peak', 'peak_dbfs', 'true_peak', 'true_peak_dbtp']
LIMITER_KEYS = ['hold', 'input_true_peak_dbtp', 'limited_samples', 'lookahead', 'max_reduction_db']


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


def _clip():
    """The stored excerpt (0.5 s at 48 kHz), forwards and then backwards."""
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    x = torch.from_numpy(F["test_wav_excerpt_i16"].astype(np.float32) / 32768.0)
    return torch.cat([x, 0.7 * x.flip(0)])[:7 * 4800 + 321]


def _count(family=b"limiter", reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(family, 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _written(path):
    from pix2pixhdaudiosr_amd.data import wavio
    data, rate = wavio.load(path)
    assert rate == RATE
    return data.numpy()


@pytest.fixture(scope="module")
def table():
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients, truepeak_plan
    plan = truepeak_plan(RATE)
    return true_peak_coefficients(plan['factor'], plan['taps_per_phase'], plan['beta']).numpy()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("limiter_in")
    x = _clip()
    wavio.save(str(d / "mono.wav"), 0.5 * x, RATE)
    wavio.save(str(d / "stereo.wav"), torch.stack([0.5 * x[:5 * 4800 + 77], -0.3 * x.flip(0)[:5 * 4800 + 77]]), RATE)
    return d


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    from pix2pixhdaudiosr_amd.models.models import create_model
    opt = _opt(mdct_type="mdct4")
    torch.manual_seed(1234)
    model = create_model(opt)
    model.eval()
    return SuperResolver(model, opt, crossover='input')


@pytest.fixture(scope="module")
def measured(resolver, files):
    """One loudness='report', true_peak=True run -> (the loudness target that leaves the true peak 4 dB over the ceiling behind the
    loudness gain, the one that leaves it 3 dB under)."""
    src = str(files / "mono.wav")
    resolver.enhance_file(src, None)                               # capture, tables, packed weights
    torch.manual_seed(5)
    first = resolver.enhance_file(src, None, encoding='float32', loudness='report', true_peak=True)
    level, top = first['loudness']['measured'], max(first['output']['true_peak_dbtp'])
    over, under = level + (CEILING_DB + 4.0) - top, level + (CEILING_DB - 3.0) - top
    print("measured %.3f LUFS, true peak %+.3f dBTP: targets %.3f and %.3f LUFS" % (level, top, over, under))
    assert -70.0 <= under < over <= 0.0
    return over, under


@pytest.fixture(scope="module")
def runs(resolver, files, measured, tmp_path_factory):
    """The same call with the limiter and with the guard alone -> (result, path) of each."""
    d = tmp_path_factory.mktemp("limiter_runs")
    src, target = str(files / "mono.wav"), measured[0]
    common = dict(encoding='float32', loudness=target, clip='guard', ceiling_dbfs=CEILING_DB)
    torch.manual_seed(5)
    _count(reset=True)
    lim = resolver.enhance_file(src, str(d / "lim.wav"), limiter=True, **common)
    assert _count() == 2                                           # two launches per file
    torch.manual_seed(5)
    guard = resolver.enhance_file(src, str(d / "guard.wav"), true_peak=True, **common)
    assert _count() == 2
    return (lim, str(d / "lim.wav")), (guard, str(d / "guard.wav"))


def test_the_written_true_peak_is_at_or_under_the_ceiling(runs, table):
    (res, out), (guard, _) = runs
    o = res['output']
    assert sorted(res) == ['hr', 'info', 'loudness', 'lr', 'metrics', 'output', 'sr']
    assert sorted(o) == sorted(OUTPUT_KEYS + ['limiter']) and sorted(o['limiter']) == LIMITER_KEYS
    lim = o['limiter']
    assert (lim['lookahead'], lim['hold']) == (240, 960) and 0 < lim['limited_samples'] < res['sr'].shape[-1]
    y = _written(out)
    got, margin = TP.true_peak(y, table), TP.dot_bound(y, table)
    # the residual overshoot: the limited clip's true peak over the ceiling in front of the guard's residual gain -- a measurement
    print("limiter: %+.3f dB at most, %d of %d samples, true peak in %+.3f dBTP; limited clip %+.5f dBTP: overshoot %+.5f dB, residual gain %.7f; "
          "written %.9f, ceiling %.9f, margin %.3e"
          % (lim['max_reduction_db'], lim['limited_samples'], y.shape[-1], lim['input_true_peak_dbtp'], max(o['true_peak_dbtp']),
             max(o['true_peak_dbtp']) - CEILING_DB, o['gain'], got.max(), CEILING, margin.max()))
    assert got.max() <= CEILING + margin.max()
    # the clip came 4 dB over, the curve's lowest point takes those 4 dB, the guard's one gain has next to nothing left to do
    assert abs(lim['input_true_peak_dbtp'] - (CEILING_DB + 4.0)) <= 0.01 and abs(lim['max_reduction_db'] + 4.0) <= 0.01
    assert lim['input_true_peak_dbtp'] == pytest.approx(max(guard['output']['true_peak_dbtp']), abs=1e-9)
    assert 0.98 < o['gain'] <= 1.0 and o['gain'] == float(TP.gain(o['true_peak'], CEILING))
    # 'sr' and the metrics stay the clip in front of the output stage
    assert torch.equal(res['sr'], guard['sr']) and res['metrics'] == guard['metrics'] and res['loudness'] == guard['loudness']


def test_the_written_loudness_is_the_restatements_and_above_the_guards(runs, measured, table):
    (res, out), (guard, out_guard) = runs
    sr = res['sr'].cpu().numpy()
    limited, g, m = LR.limit(sr, CEILING, table, 240, 960)
    rest = float(TP.gain(TP.true_peak(limited, table).astype(np.float32), CEILING))
    want = LOUD.integrated(limited * rest, RATE)
    level, level_guard = LOUD.integrated(_written(out), RATE), LOUD.integrated(_written(out_guard), RATE)
    print("target %.3f LUFS; written with the limiter %.4f (restatement %.4f, its residual gain %.7f), with the guard alone %.4f LUFS"
          % (measured[0], level, want, rest, level_guard))
    assert abs(level - want) <= 0.001
    assert level > level_guard                                     # by construction the guard's file sits 4 dB under the target
    assert res['output']['limiter']['limited_samples'] == pytest.approx(int((g < 1).sum()), abs=0.02 * g.size)


def test_a_clip_that_fits_is_written_as_the_guard_writes_it(resolver, files, measured, tmp_path):
    src, target = str(files / "mono.wav"), measured[1]
    common = dict(encoding='float32', loudness=target, clip='guard', ceiling_dbfs=CEILING_DB)
    torch.manual_seed(5)
    guard = resolver.enhance_file(src, str(tmp_path / "g.wav"), true_peak=True, **common)
    torch.manual_seed(5)
    res = resolver.enhance_file(src, str(tmp_path / "l.wav"), limiter=True, **common)
    assert _bytes(str(tmp_path / "l.wav")) == _bytes(str(tmp_path / "g.wav"))
    lim = res['output'].pop('limiter')
    assert lim['limited_samples'] == 0 and lim['max_reduction_db'] == 0.0 and res['output'] == guard['output'] and res['output']['gain'] == 1.0
    assert lim['input_true_peak_dbtp'] == max(guard['output']['true_peak_dbtp'])


def test_without_the_option_nothing_changes(resolver, files, tmp_path):
    src = str(files / "mono.wav")
    outs = []
    for k, kw in enumerate(({}, dict(limiter=False), dict(clip='guard', ceiling_dbfs=-20.0, true_peak=True),
                            dict(clip='guard', ceiling_dbfs=-20.0, true_peak=True, limiter=False))):
        torch.manual_seed(5)
        _count(reset=True)
        _count(b"truepeak", reset=True)
        res = resolver.enhance_file(src, str(tmp_path / ("%d.wav" % k)), encoding='float32', **kw)
        assert _count() == 0 and _count(b"truepeak") == (1 if 'true_peak' in kw else 0)
        outs.append(res)
    assert sorted(outs[0]) == sorted(outs[1]) == ['hr', 'info', 'lr', 'metrics', 'sr']
    assert sorted(outs[2]['output']) == sorted(outs[3]['output']) == OUTPUT_KEYS and outs[2]['output'] == outs[3]['output']
    assert _bytes(str(tmp_path / "0.wav")) == _bytes(str(tmp_path / "1.wav")) and _bytes(str(tmp_path / "2.wav")) == _bytes(str(tmp_path / "3.wav"))
    with pytest.raises(ValueError, match="clip='guard'"):
        resolver.enhance_file(src, str(tmp_path / "never.wav"), limiter=True)
    assert not os.path.exists(str(tmp_path / "never.wav"))


def test_folder_records_and_csv_columns(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_LIMITER, write_metrics_csv
    common = dict(channels='all', encoding='float32', clip='guard', ceiling_dbfs=-20.0)
    plain = resolver.enhance_folder(str(files), str(tmp_path / "off"), seed=11, **common)
    assert all(sorted(r['output']) == ['clipped', 'gain', 'nonfinite', 'peak', 'peak_dbfs'] for r in plain)
    _count(reset=True)
    recs = resolver.enhance_folder(str(files), str(tmp_path / "on"), seed=11, limiter=True, limiter_lookahead_ms=1.5, limiter_hold_ms=0.0, **common)
    assert _count() == 4                                           # two per file
    by = {r['path']: r for r in recs}
    for name in ("mono.wav", "stereo.wav"):
        o = by[name]['output']
        assert sorted(o) == sorted(OUTPUT_KEYS + ['limiter']) and sorted(o['limiter']) == LIMITER_KEYS
        assert (o['limiter']['lookahead'], o['limiter']['hold']) == (72, 0) and o['limiter']['limited_samples'] > 0
        assert len(o['true_peak']) == (2 if name == "stereo.wav" else 1)
        torch.manual_seed(11)
        one = resolver.enhance_file(str(files / name), str(tmp_path / ("one_" + name)), limiter=True, limiter_lookahead_ms=1.5, limiter_hold_ms=0.0, **common)
        assert by[name]['output'] == one['output'] and _bytes(str(tmp_path / "on" / name)) == _bytes(str(tmp_path / ("one_" + name)))
        # the written file: louder than the guard's, its largest sample under the ceiling
        y, y_off = _written(str(tmp_path / "on" / name)), _written(str(tmp_path / "off" / name))
        assert np.abs(y).max() <= 10.0 ** (-20.0 / 20.0) * (1.0 + 1e-6) and np.square(y).sum() > np.square(y_off).sum()
    write_metrics_csv(str(tmp_path / "off.csv"), plain)
    write_metrics_csv(str(tmp_path / "on.csv"), recs, limiter=True)
    rows_off, rows_on = (list(csv.reader(open(str(tmp_path / n)))) for n in ("off.csv", "on.csv"))
    assert tuple(rows_off[0]) == METRICS_COLUMNS and tuple(rows_on[0]) == METRICS_COLUMNS + METRICS_COLUMNS_LIMITER
    assert len(rows_on) == 1 + 3 + 1                               # three written channels and the mean
    for row in rows_on[1:-1]:
        lim = by[row[0]]['output']['limiter']
        assert float(row[-2]) == lim['max_reduction_db'] and int(row[-1]) == lim['limited_samples']
    assert [r[:-2] for r in rows_on] == rows_off                  # the other columns do not move
    with pytest.raises(ValueError, match="limiter must be a bool"):        # before any file is touched
        resolver.enhance_folder(str(files), str(tmp_path / "never"), clip='guard', limiter=1)
    assert not os.path.exists(str(tmp_path / "never"))
