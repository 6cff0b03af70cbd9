"""enhance_file(speech_level=...) / enhance_folder(speech_level=...) / --speech_level on the GPU: without the option nothing
changes and nothing is launched; 'report' only reports, and what it reports is the restatement of tests/_speechlevel_ref.py on the
clip; with a target the written clip is the report run's clip times one float32 gain, bit for bit, and the file, re-read, has the
level the restatement gives that product; 'input' on an 8 kHz two-channel mu-law SPHERE file; the clip guard with the true peak,
the output rate, FLAC, folders, the CSV columns and the command line's lines around it.  The tiny model is the one of
tests/test_gpu_lowband.py, restated; its weights are untrained, so the resolver runs with crossover='input': the clip that is
measured and written then carries the input's own band.

P.56 is not exactly scale-equivariant (the thresholds are fixed and 6 dB apart), so the level of the written file is checked
against the restatement of the scaled clip, not against the target; the departure from the target is printed."""
import csv
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _containers_ref as CR
import _speechlevel_ref as R
import _wavcodec_ref as W
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE, OUT = 48000, 44100
KEYS = ['activity', 'activity_input', 'channels', 'gain_db', 'input', 'long_term', 'measured', 'output', 'target']
GAIN_DB_TOL = 2.1e-6            # two float32 ulp of the gain, in dB: 2 * 2^-23 * 20 / ln 10


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


def _clip():
    """The stored excerpt (0.5 s), forwards and then backwards, with a pause of 0.4 s of faint noise between (twice the hangover): speech, a
    pause, speech."""
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    x = torch.from_numpy(F["test_wav_excerpt_i16"].astype(np.float32) / 32768.0)
    pause = 2e-4 * torch.randn(19200, generator=torch.Generator().manual_seed(3))      # -74 dBFS: some 50 dB under the speech, not digital silence
    return torch.cat([x, pause, 0.7 * x.flip(0)])[:65000 + 321]


def _count(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(b"speechlevel", 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _written(path, rate=RATE):
    from pix2pixhdaudiosr_amd.data import wavio
    data, r = wavio.load(path)
    assert r == rate
    return data.numpy()


_CONSTS = {}


def _level(clip, rate):
    """The restatement's (rows, file figure, channel) of a clip [C, n], with the constants of the library's entry."""
    from pix2pixhdaudiosr_amd.generate import speech_level_consts
    if rate not in _CONSTS:
        c, I = speech_level_consts(rate)
        _CONSTS[rate] = (tuple(c[:4].tolist()), I)
    return R.chunked(np.atleast_2d(clip), *_CONSTS[rate])


def _f32_gain(gain_db):
    """The float32 gain behind a result's 'gain_db' (20 log10 of it in float64: the float32 comes back exactly)."""
    return np.float32(10.0 ** (gain_db / 20.0))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("speechlevel_in")
    x = _clip()
    wavio.save(str(d / "mono.wav"), 0.5 * x, RATE)
    n = 40000 + 77
    wavio.save(str(d / "stereo.wav"), torch.stack([0.5 * x[:n], -0.2 * x.flip(0)[:n]]), RATE)
    # a telephone file: 8 kHz, two talkers, mu-law, NIST SPHERE
    # (over a floor of line noise at -60 dBFS: the pauses of the fixtures are never digital silence)
    floor = (1e-3 * np.random.default_rng(9).standard_normal((2, 9000))).astype(np.float32)
    tel = floor + np.stack([R.modulated_noise(9000, 8000, 1, depth_hz=1.1, level=0.2), R.modulated_noise(9000, 8000, 2, depth_hz=0.7, level=0.05)])
    ints = np.clip(np.round(tel * 32768.0), -32768, 32767).astype(np.int64)
    sph = tmp_path_factory.mktemp("speechlevel_tel")
    with open(str(sph / "tel.sph"), "wb") as f:
        f.write(CR.sphere(W.g711_encode(ints, W.ULAW), CR.sphere_fields(2, 8000, 1, 9000, "ulaw")))
    return SimpleNamespace(dir=d, tel=str(sph / "tel.sph"))


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    return SuperResolver(model, opt, crossover='input')


@pytest.fixture(scope="module")
def plain(resolver, files, tmp_path_factory):
    """The run without the option that the others are compared with: seed 5, float32."""
    out = str(tmp_path_factory.mktemp("speechlevel_plain") / "plain.wav")
    resolver.enhance_file(str(files.dir / "mono.wav"), None)          # capture, tables, packed weights
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files.dir / "mono.wav"), out, encoding='float32')
    assert _count() == 0
    return res, out


@pytest.fixture(scope="module")
def report(resolver, files, plain, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("speechlevel_report") / "r.wav")
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files.dir / "mono.wav"), out, encoding='float32', speech_level='report')
    assert _count() == 6                                           # envelope, counts, decision: of the input and of the generated clip
    return res, out, _level(res['sr'].cpu().numpy(), RATE)


def test_option_off_changes_nothing(resolver, files, plain, tmp_path):
    res0, out0 = plain
    assert sorted(res0) == ['hr', 'info', 'lr', 'metrics', 'sr']
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files.dir / "mono.wav"), str(tmp_path / "off.wav"), encoding='float32', speech_level=None)
    assert _count() == 0 and sorted(res) == sorted(res0)
    assert _bytes(str(tmp_path / "off.wav")) == _bytes(out0) and torch.equal(res['sr'], res0['sr']) and res['metrics'] == res0['metrics']
    with pytest.raises(ValueError, match="option of speech_level"):
        resolver.enhance_file(str(files.dir / "mono.wav"), None, speech_level_max_gain_db=6.0)
    for loud in (dict(loudness=-23.0), dict(loudness='report', loudness_range=True)):
        with pytest.raises(ValueError, match="two claims on the one gain"):
            resolver.enhance_file(str(files.dir / "missing.wav"), None, speech_level=-26.0, **loud)      # (before the file is opened)
    with pytest.raises(ValueError, match="speech_level must be"):
        resolver.enhance_file(str(files.dir / "missing.wav"), None, speech_level='loud')


def test_report_mode_only_reports(resolver, files, plain, report):
    res0, out0 = plain
    res, out, (rows, fig, ch) = report
    assert _bytes(out) == _bytes(out0) and torch.equal(res['sr'], res0['sr']) and res['metrics'] == res0['metrics']
    assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'speech_level', 'sr']
    info = res['speech_level']
    print("report %r" % info)
    assert sorted(info) == KEYS and info['gain_db'] == 0 and info['target'] is None and info['output'] == info['measured']
    assert math.isfinite(fig['active']) and 0.05 < fig['activity'] < 0.999        # (the clip has speech and a pause: the figure means something)
    assert abs(info['measured'] - fig['active']) <= 1e-9 and abs(info['long_term'] - fig['long_term']) <= 1e-9
    assert abs(info['activity'] - fig['activity']) <= 1e-12
    assert info['channels'] == [{'active': info['measured'], 'long_term': info['long_term'], 'activity': info['activity']}]
    rows_in, fig_in, _ = _level(res['lr'].cpu().numpy(), RATE)
    assert abs(info['input'] - fig_in['active']) <= 1e-9 and abs(info['activity_input'] - fig_in['activity']) <= 1e-12
    # measuring alone: no file asked for, the same figures
    torch.manual_seed(5)
    res2 = resolver.enhance_file(str(files.dir / "mono.wav"), None, speech_level='report')
    assert res2['speech_level'] == info and 'output' not in res2


def test_target_scales_by_one_float32_gain(resolver, files, report, tmp_path):
    res_r, _, (rows, fig, ch) = report
    out = str(tmp_path / "t.wav")
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files.dir / "mono.wav"), out, encoding='float32', speech_level=-26.0)
    assert _count() == 6
    info = res['speech_level']
    assert sorted(info) == KEYS and info['target'] == -26.0 and info['measured'] == res_r['speech_level']['measured']
    assert abs(info['gain_db'] - (-26.0 - info['measured'])) <= GAIN_DB_TOL and abs(info['gain_db']) > 0.5
    assert info['output'] == info['measured'] + info['gain_db']
    g = _f32_gain(info['gain_db'])
    want = res_r['sr'].cpu().numpy() * g
    assert (res['sr'].cpu().numpy() == want).all()
    assert res['metrics'] == res_r['metrics'] and torch.equal(res['lr'], res_r['lr'])
    # the written file, re-read: the restatement's level of it is the restatement's level of report_sr * gain
    y = _written(out)
    _, fig_y, _ = _level(y, RATE)
    _, fig_w, _ = _level(want, RATE)
    print("written %.6f dBov, departure from the target %+.6f dB; result %r" % (fig_y['active'], fig_y['active'] - (-26.0), info))
    assert abs(fig_y['active'] - fig_w['active']) <= 1e-6
    # the clamp: at most 1 dB
    torch.manual_seed(5)
    res1 = resolver.enhance_file(str(files.dir / "mono.wav"), None, speech_level=-26.0, speech_level_max_gain_db=1.0)
    assert abs(abs(res1['speech_level']['gain_db']) - 1.0) <= GAIN_DB_TOL and np.sign(res1['speech_level']['gain_db']) == np.sign(info['gain_db'])


def test_input_mode_on_a_telephone_sphere_file(resolver, files, tmp_path):
    """8 kHz, two talkers, mu-law, NIST SPHERE, is_lr_input: the written clip at the input's active level, one gain for both channels."""
    torch.manual_seed(5)
    rep = resolver.enhance_file(files.tel, None, is_lr_input=True, channels='all', speech_level='report')
    out = str(tmp_path / "tel.wav")
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(files.tel, out, is_lr_input=True, channels='all', encoding='float32', speech_level='input')
    assert _count() == 6 and res['sr'].shape[0] == 2 and res['info'].sample_rate == 8000
    info = res['speech_level']
    rows_in, fig_in, ch_in = _level(res['lr'].cpu().numpy(), RATE)        # the input is measured at the model's rate
    rows_out, fig_out, ch_out = _level(rep['sr'].cpu().numpy(), RATE)
    print("tel: %r; input channel %d, output channel %d" % (info, ch_in, ch_out))
    assert ch_in == 0 and abs(info['input'] - fig_in['active']) <= 1e-9 and info['target'] == info['input']
    assert abs(info['measured'] - fig_out['active']) <= 1e-9
    assert abs(info['gain_db'] - (info['input'] - info['measured'])) <= GAIN_DB_TOL
    g = _f32_gain(info['gain_db'])
    assert (res['sr'].cpu().numpy() == rep['sr'].cpu().numpy() * g).all()            # both talkers by one gain: their balance stays
    assert len(info['channels']) == 2
    for c in range(2):
        assert abs(info['channels'][c]['active'] - (rows_out[c]['active'] + info['gain_db'])) <= 1e-9
        assert abs(info['channels'][c]['activity'] - rows_out[c]['activity']) <= 1e-12
    assert (_written(out) == res['sr'].cpu().numpy()).all()


def test_clip_guard_and_true_peak_act_behind_the_gain(resolver, files, report, tmp_path):
    res_r, _, _ = report
    out = str(tmp_path / "g.wav")
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files.dir / "mono.wav"), out, encoding='float32', speech_level=-26.0, clip='guard', ceiling_dbfs=-30.0,
                                true_peak=True)
    guard = res['output']['gain']
    assert guard < 0.9                                            # the ceiling is under the clip's peak at -26 dBov: the guard scales
    # the peak report and the true-peak measurement saw the clip behind the speech-level gain
    assert res['output']['peak'][0] == pytest.approx(float(res['sr'].abs().max()), rel=1e-6)
    assert res['output']['true_peak'][0] >= res['output']['peak'][0]
    g = _f32_gain(res['speech_level']['gain_db'])
    assert (res['sr'].cpu().numpy() == res_r['sr'].cpu().numpy() * g).all()
    y = _written(out)
    assert 20.0 * np.log10(np.abs(y).max()) <= -30.0 + 1e-4
    _, fig_y, _ = _level(y, RATE)
    _, fig_w, _ = _level(res['sr'].cpu().numpy() * np.float32(guard), RATE)
    print("written %.6f dBov behind a guard gain of %r" % (fig_y['active'], guard))
    assert abs(fig_y['active'] - fig_w['active']) <= 1e-6         # (one float32 multiply by the guard's gain on either side)


def test_output_rate_is_the_measured_rate(resolver, files, tmp_path):
    torch.manual_seed(5)
    rep = resolver.enhance_file(str(files.dir / "mono.wav"), None, output_rate=OUT, speech_level='report')
    assert rep['sr'].shape[-1] != _clip().numel()
    _, fig, _ = _level(rep['sr'].cpu().numpy(), OUT)
    _, fig_in, _ = _level(rep['lr'].cpu().numpy(), RATE)
    info = rep['speech_level']
    assert abs(info['measured'] - fig['active']) <= 1e-9 and abs(info['input'] - fig_in['active']) <= 1e-9
    _, wrong, _ = _level(rep['sr'].cpu().numpy(), RATE)
    assert abs(wrong['active'] - fig['active']) > 1e-9            # (the check tells the two rates apart)
    out = str(tmp_path / "o.wav")
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files.dir / "mono.wav"), out, encoding='float32', output_rate=OUT, speech_level=-26.0)
    g = _f32_gain(res['speech_level']['gain_db'])
    assert (res['sr'].cpu().numpy() == rep['sr'].cpu().numpy() * g).all() and (_written(out, OUT) == res['sr'].cpu().numpy()).all()


def test_flac_container(resolver, files, tmp_path):
    torch.manual_seed(5)
    wav = resolver.enhance_file(str(files.dir / "mono.wav"), str(tmp_path / "f.wav"), encoding='pcm16', speech_level=-26.0)
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files.dir / "mono.wav"), str(tmp_path / "f.flac"), encoding='pcm16', speech_level=-26.0, container='flac')
    assert _count() == 6 and res['flac'] is not None and res['speech_level'] == wav['speech_level']
    assert torch.equal(res['sr'], wav['sr'])
    from pix2pixhdaudiosr_amd.data import flacio
    data, rate = flacio.load(str(tmp_path / "f.flac"))
    assert rate == RATE and (data.numpy() == _written(str(tmp_path / "f.wav"))).all()


def test_folder_records_csv_columns_and_all_channels(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_SPEECH_LEVEL, write_metrics_csv
    plain = resolver.enhance_folder(str(files.dir), str(tmp_path / "off"), channels='all', seed=11)
    assert all('speech_level' not in r for r in plain)
    _count(reset=True)
    recs = resolver.enhance_folder(str(files.dir), str(tmp_path / "on"), channels='all', seed=11, encoding='float32', speech_level=-26.0)
    assert _count() == 12                                          # six per file
    by = {r['path']: r for r in recs}
    for name in ("mono.wav", "stereo.wav"):
        torch.manual_seed(11)
        one = resolver.enhance_file(str(files.dir / name), str(tmp_path / ("one_" + name)), channels='all', encoding='float32', speech_level=-26.0)
        assert by[name]['speech_level'] == one['speech_level'] and sorted(one['speech_level']) == KEYS
        assert _bytes(str(tmp_path / "on" / name)) == _bytes(str(tmp_path / ("one_" + name)))
    # two channels: the file's figure is the louder one's, and one gain moved both
    s = by["stereo.wav"]['speech_level']
    assert len(s['channels']) == 2 and s['output'] == max(c['active'] for c in s['channels'])
    torch.manual_seed(11)
    unscaled = resolver.enhance_file(str(files.dir / "stereo.wav"), None, channels='all')
    assert (_written(str(tmp_path / "on" / "stereo.wav")) == unscaled['sr'].cpu().numpy() * _f32_gain(s['gain_db'])).all()
    # the table: three more columns with the option, none without
    write_metrics_csv(str(tmp_path / "off.csv"), plain)
    write_metrics_csv(str(tmp_path / "on.csv"), recs, speech_level=True)
    rows_off, rows_on = (list(csv.reader(open(str(tmp_path / n)))) for n in ("off.csv", "on.csv"))
    assert tuple(rows_off[0]) == METRICS_COLUMNS and tuple(rows_on[0]) == METRICS_COLUMNS + METRICS_COLUMNS_SPEECH_LEVEL
    assert len(rows_on) == 1 + 3 + 1                               # three written channels and the mean
    for row in rows_on[1:-1]:
        l = by[row[0]]['speech_level']
        assert [float(v) for v in row[-3:]] == [l['input'], l['output'], l['activity']]
    with pytest.raises(ValueError, match="speech_level must be"):  # before any file is touched
        resolver.enhance_folder(str(files.dir), str(tmp_path / "never"), speech_level='loud')
    with pytest.raises(ValueError, match="two claims on the one gain"):
        resolver.enhance_folder(str(files.dir), str(tmp_path / "never"), speech_level=-26.0, loudness=-23.0, loudness_scope='folder')
    assert not os.path.exists(str(tmp_path / "never"))


def test_more_than_eight_written_channels_are_refused(resolver, tmp_path):
    """Nine written channels: a ValueError from enhance_file, a skipped file with the error in its record from enhance_folder, and
    nothing written either way.  Eight are accepted and every one of them is measured; channels='first' of the nine is one channel."""
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path / "wide"
    os.makedirs(str(d))
    x = _clip()[:30000]
    rows = torch.stack([(0.5 - 0.05 * c) * (x if c % 2 == 0 else x.flip(0)) for c in range(9)])
    wavio.save(str(d / "eight.wav"), rows[:8], RATE)
    wavio.save(str(d / "nine.wav"), rows, RATE)
    _count(reset=True)
    with pytest.raises(ValueError, match="measured over at most 8 channels, 9 would be written"):
        resolver.enhance_file(str(d / "nine.wav"), str(tmp_path / "nine_out.wav"), channels='all', speech_level='report')
    assert _count() == 0 and not os.path.exists(str(tmp_path / "nine_out.wav"))
    recs = resolver.enhance_folder(str(d), str(tmp_path / "out"), channels='all', seed=3, encoding='float32', speech_level=-26.0)
    by = {r['path']: r for r in recs}
    assert sorted(by) == ["eight.wav", "nine.wav"] and _count() == 6           # the six launches of the one file that was enhanced
    nine, eight = by["nine.wav"], by["eight.wav"]
    assert "measured over at most 8 channels, 9 would be written" in nine['error'] and nine['speech_level'] is None
    assert nine['written_channels'] == 0 and not os.path.exists(str(tmp_path / "out" / "nine.wav"))
    assert eight['error'] is None and eight['written_channels'] == 8 and os.path.exists(str(tmp_path / "out" / "eight.wav"))
    s8 = eight['speech_level']
    assert sorted(s8) == KEYS and len(s8['channels']) == 8
    y = _written(str(tmp_path / "out" / "eight.wav"))
    rows_y, fig_y, ch_y = _level(y, RATE)
    torch.manual_seed(3)
    unscaled = resolver.enhance_file(str(d / "eight.wav"), None, channels='all')
    rows_u, fig_u, ch_u = _level(unscaled['sr'].cpu().numpy(), RATE)
    assert abs(s8['measured'] - fig_u['active']) <= 1e-9 and s8['measured'] == max(r['active'] for r in rows_u)
    for c in range(8):
        assert abs(s8['channels'][c]['active'] - (rows_u[c]['active'] + s8['gain_db'])) <= 1e-9
        assert abs(s8['channels'][c]['activity'] - rows_u[c]['activity']) <= 1e-12
    assert (y == unscaled['sr'].cpu().numpy() * _f32_gain(s8['gain_db'])).all()
    # one channel of the nine is no refusal
    one = resolver.enhance_file(str(d / "nine.wav"), None, channels='first', speech_level='report')
    assert len(one['speech_level']['channels']) == 1


def test_cli_lines_and_csv_header(files, tmp_path, capsys):
    """Without --speech_level main() prints the lines it printed before the option existed and the table has the columns it had;
    with it, one `speech level` line per file more and three columns more, holding what enhance_file returns."""
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
    base = ["--input", str(files.dir / "mono.wav"), "--load_pretrain", str(folder), "--encoding", "float32", "--crossover", "input"]
    _count(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "off.wav"), "--metrics_csv", str(tmp_path / "off.csv")]) == 0
    assert _count() == 0
    off = capsys.readouterr().out.splitlines()
    assert not any("speech level" in l for l in off)
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(G.METRICS_COLUMNS)
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--metrics_csv", str(tmp_path / "on.csv"), "--speech_level", "-26"]) == 0
    assert _count() == 6
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if ": speech level " in l]
    assert len(extra) == 1 and [l.replace("on.wav", "off.wav").replace("on.csv", "off.csv") for l in on if l not in extra] == off
    m = re.fullmatch(re.escape(str(tmp_path / "on.wav")) + r": speech level input ([-+]\d+\.\d\d) dBov \(activity (\d+\.\d) %\), measured ([-+]\d+\.\d\d) dBov "
                     r"\(activity (\d+\.\d) %\), gain ([-+]\d+\.\d\d) dB -> ([-+]\d+\.\d\d) dBov", extra[0])
    assert m and m.group(6) == "-26.00" and on.index(extra[0]) == len(on) - 2      # behind its file's `wrote` line
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == G.METRICS_COLUMNS + G.METRICS_COLUMNS_SPEECH_LEVEL and len(rows) == 3
    assert abs(float(rows[1][-2]) - (-26.0)) <= 1e-5 and "%+.2f" % float(rows[1][-3]) == m.group(1)
    assert "%.1f" % (100.0 * float(rows[1][-1])) == m.group(4)
    # the metric lines and columns are those of the clip in front of the gain
    assert rows[1][:7] == list(csv.reader(open(str(tmp_path / "off.csv"))))[1][:7]
    # folder mode: one line per file
    assert G.main(["--input", str(files.dir), "--output", str(tmp_path / "dir"), "--load_pretrain", str(folder), "--channels", "all",
                   "--crossover", "input", "--speech_level", "report"]) == 0
    lines = capsys.readouterr().out.splitlines()
    mine = [l for l in lines if ": speech level input " in l]
    assert len(mine) == 2 and all("gain +0.00 dB" in l for l in mine)
    with pytest.raises(SystemExit):
        G.main(base + ["--output", str(tmp_path / "no.wav"), "--speech_level", "5"])
    with pytest.raises(SystemExit):
        G.main(base + ["--output", str(tmp_path / "no.wav"), "--speech_level", "-26", "--loudness", "-23"])
    assert not os.path.exists(str(tmp_path / "no.wav"))
