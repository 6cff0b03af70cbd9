"""enhance_file(loudness=...) / enhance_folder(loudness=...) / --loudness on the GPU: without the option nothing changes and
nothing is launched; with a target the written file, measured by the restatement of tests/_loudness_ref.py, sits at the target;
'input' brings it to the input's level; 'report' only reports; the clip guard acts behind the gain; four launches per file;
folders, the CSV columns and the command line's lines.  The tiny model is the one of tests/test_gpu_lowband.py, restated; its
weights are untrained and what it generates is some 25 dB quieter than its input, so the resolver runs with crossover='input':
the clip that is measured and written then carries the input's own band at the pipeline's level, a few dB from the targets."""
import csv
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _loudness_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE = 48000
KEYS = ['gain_db', 'input', 'measured', 'momentary_max', 'output', 'target']


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


def _excerpt():
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    return torch.from_numpy(F["test_wav_excerpt_i16"].astype(np.float32) / 32768.0)


def _clip(hops=7):
    """0.1 s hops of the stored excerpt (0.5 s), forwards and then backwards: long enough for a few 400 ms blocks."""
    x = _excerpt()
    return torch.cat([x, 0.7 * x.flip(0)])[:hops * (RATE // 10) + 321]


def _count(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(b"loudness", 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _written(path):
    from pix2pixhdaudiosr_amd.data import wavio
    data, rate = wavio.load(path)
    assert rate == RATE
    return data.numpy()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("loudness_in")
    x = _clip()
    wavio.save(str(d / "mono.wav"), 0.5 * x, RATE)
    wavio.save(str(d / "stereo.wav"), torch.stack([0.5 * x[:5 * 4800 + 77], -0.3 * x.flip(0)[:5 * 4800 + 77]]), RATE)
    return d


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    return SuperResolver(model, opt, crossover='input')


@pytest.fixture(scope="module")
def plain(resolver, files, tmp_path_factory):
    """The run without the option that the others are compared with: seed 5, float32."""
    out = str(tmp_path_factory.mktemp("loudness_plain") / "plain.wav")
    resolver.enhance_file(str(files / "mono.wav"), None)          # capture, tables, packed weights
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32')
    assert _count() == 0
    return res, out


def _gates_cannot_move(sr_rows, gain_db):
    """The precondition of the level checks: no block of the measured clip below -50 LUFS and a gain within 20 dB, so no block
    crosses the absolute gate at -70 when the gain is applied (the relative gate moves with the clip)."""
    g = R.gating(R.hop_energies(sr_rows, RATE), RATE)
    print("blocks %s  gain %+.3f dB" % (np.round(g['l'], 2), gain_db))
    assert len(g['l']) >= 2 and g['l'].min() > -50.0 and abs(gain_db) <= 20.0
    return g


def test_option_off_changes_nothing(resolver, files, plain, tmp_path):
    res0, out0 = plain
    assert sorted(res0) == ['hr', 'info', 'lr', 'metrics', 'sr']
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), str(tmp_path / "off.wav"), encoding='float32', loudness=None)
    assert _count() == 0 and sorted(res) == sorted(res0)
    assert _bytes(str(tmp_path / "off.wav")) == _bytes(out0) and torch.equal(res['sr'], res0['sr']) and res['metrics'] == res0['metrics']
    with pytest.raises(ValueError, match="option of loudness"):
        resolver.enhance_file(str(files / "mono.wav"), None, loudness_max_gain_db=6.0)


def test_target_puts_the_written_file_at_the_target(resolver, files, plain, tmp_path):
    res0, _ = plain
    out = str(tmp_path / "t.wav")
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32', loudness=-23.0)
    assert _count() == 4                                           # two hop and two gate launches
    assert sorted(res) == ['hr', 'info', 'loudness', 'lr', 'metrics', 'sr']
    info = res['loudness']
    assert sorted(info) == KEYS and info['target'] == -23.0
    _gates_cannot_move(res0['sr'].cpu().numpy(), info['gain_db'])
    y = _written(out)
    level = R.integrated(y, RATE)
    print("written %.6f LUFS; result %r" % (level, info))
    assert abs(level - (-23.0)) <= 0.001
    # the result's figures: the restatement's, and consistent with each other
    assert abs(info['measured'] - R.integrated(res0['sr'].cpu().numpy(), RATE)) <= 0.001
    assert abs(info['input'] - R.integrated(res['lr'].cpu().numpy(), RATE)) <= 0.001
    assert info['output'] == info['measured'] + info['gain_db'] and abs(info['output'] - (-23.0)) <= 1e-5
    assert abs(info['gain_db']) > 0.5                              # (the test would show nothing on a clip that sits at the target)
    assert info['momentary_max'] >= info['output']
    # 'sr' is the written clip, one multiply of the unscaled one; the metrics are the unscaled clip's, bit for bit
    assert (res['sr'].cpu().numpy() == y).all()
    g = np.float32(10.0 ** (info['gain_db'] / 20.0))
    assert np.abs(res['sr'].cpu().numpy() - res0['sr'].cpu().numpy() * g).max() <= 1e-6 * np.abs(y).max()
    assert res['metrics'] == res0['metrics'] and torch.equal(res['lr'], res0['lr'])
    # the clamp: at most 1 dB
    torch.manual_seed(5)
    res1 = resolver.enhance_file(str(files / "mono.wav"), None, loudness=-23.0, loudness_max_gain_db=1.0)
    assert abs(abs(res1['loudness']['gain_db']) - 1.0) <= 1e-6 and np.sign(res1['loudness']['gain_db']) == np.sign(info['gain_db'])


def test_input_mode_matches_the_level_of_the_input(resolver, files, plain, tmp_path):
    res0, _ = plain
    out = str(tmp_path / "i.wav")
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32', loudness='input')
    assert _count() == 4
    info = res['loudness']
    _gates_cannot_move(res0['sr'].cpu().numpy(), info['gain_db'])
    want = R.integrated(res['lr'].cpu().numpy(), RATE)
    level = R.integrated(_written(out), RATE)
    print("written %.6f LUFS, input %.6f LUFS; result %r" % (level, want, info))
    assert abs(level - want) <= 0.001
    assert info['target'] == info['input'] and abs(info['input'] - want) <= 0.001


def test_report_mode_only_reports(resolver, files, plain, tmp_path):
    res0, out0 = plain
    out = str(tmp_path / "r.wav")
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32', loudness='report')
    assert _count() == 4
    assert _bytes(out) == _bytes(out0) and torch.equal(res['sr'], res0['sr'])
    info = res['loudness']
    assert sorted(info) == KEYS and info['gain_db'] == 0 and info['target'] is None and info['output'] == info['measured']
    assert abs(info['measured'] - R.integrated(res0['sr'].cpu().numpy(), RATE)) <= 0.001
    # measuring alone: no file asked for, the same figures
    torch.manual_seed(5)
    res2 = resolver.enhance_file(str(files / "mono.wav"), None, loudness='report')
    assert res2['loudness'] == info and 'output' not in res2


def test_clip_guard_acts_behind_the_gain(resolver, files, plain, tmp_path):
    res0, _ = plain
    out = str(tmp_path / "g.wav")
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32', loudness=-23.0, clip='guard', ceiling_dbfs=-30.0)
    guard = res['output']['gain']
    _gates_cannot_move(res0['sr'].cpu().numpy(), res['loudness']['gain_db'] + 20.0 * np.log10(guard))
    assert guard < 0.9                                            # the ceiling is under the clip's peak at -23 LUFS: the guard scales
    # the peak report saw the clip behind the loudness gain
    assert res['output']['peak'][0] == pytest.approx(float(res['sr'].abs().max()), rel=1e-6)
    level = R.integrated(_written(out), RATE)
    print("written %.6f LUFS, guard gain %r" % (level, guard))
    assert abs(level - (-23.0 + 20.0 * np.log10(guard))) <= 0.001
    assert 20.0 * np.log10(np.abs(_written(out)).max()) <= -30.0 + 1e-4


def test_folder_records_csv_columns_and_all_channels(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_LOUDNESS, write_metrics_csv
    plain = resolver.enhance_folder(str(files), str(tmp_path / "off"), channels='all', seed=11)
    assert all('loudness' not in r for r in plain)
    _count(reset=True)
    recs = resolver.enhance_folder(str(files), str(tmp_path / "on"), channels='all', seed=11, encoding='float32', loudness=-23.0)
    assert _count() == 8                                           # four per file
    by = {r['path']: r for r in recs}
    for name in ("mono.wav", "stereo.wav"):
        torch.manual_seed(11)
        one = resolver.enhance_file(str(files / name), str(tmp_path / ("one_" + name)), channels='all', encoding='float32', loudness=-23.0)
        assert by[name]['loudness'] == one['loudness'] and sorted(one['loudness']) == KEYS
        assert _bytes(str(tmp_path / "on" / name)) == _bytes(str(tmp_path / ("one_" + name)))
    # both channels as one programme: the written stereo file sits at the target
    torch.manual_seed(11)
    unscaled = resolver.enhance_file(str(files / "stereo.wav"), None, channels='all')
    _gates_cannot_move(unscaled['sr'].cpu().numpy(), by["stereo.wav"]['loudness']['gain_db'])
    level = R.integrated(_written(str(tmp_path / "on" / "stereo.wav")), RATE)
    print("stereo written %.6f LUFS" % level)
    assert abs(level - (-23.0)) <= 0.001
    # the table: three more columns with the option, none without
    write_metrics_csv(str(tmp_path / "off.csv"), plain)
    write_metrics_csv(str(tmp_path / "on.csv"), recs, False, False, True)
    rows_off, rows_on = (list(csv.reader(open(str(tmp_path / n)))) for n in ("off.csv", "on.csv"))
    assert tuple(rows_off[0]) == METRICS_COLUMNS and tuple(rows_on[0]) == METRICS_COLUMNS + METRICS_COLUMNS_LOUDNESS
    assert len(rows_on) == 1 + 3 + 1                               # three written channels and the mean
    for row in rows_on[1:-1]:
        l = by[row[0]]['loudness']
        assert [float(v) for v in row[-3:]] == [l['input'], l['output'], l['gain_db']]
    with pytest.raises(ValueError, match="loudness must be"):      # before any file is touched
        resolver.enhance_folder(str(files), str(tmp_path / "never"), loudness='loud')
    assert not os.path.exists(str(tmp_path / "never"))


def test_graphed_and_eager_runs_write_the_same_bytes(files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    outs = []
    for graph in (True, False):
        sr = SuperResolver(model, opt, graph=graph, crossover='input')
        out = str(tmp_path / ("graph%d.wav" % graph))
        torch.manual_seed(9)
        res = sr.enhance_file(str(files / "stereo.wav"), out, channels='all', loudness='input')
        outs.append((_bytes(out), res['loudness']))
    assert outs[0] == outs[1]


def test_cli_lines_and_csv_header(files, tmp_path, capsys):
    """Without --loudness main() prints the lines it printed before the option existed and the table has the columns it had;
    with it, one `loudness` line per file more and three columns more, holding what enhance_file returns."""
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
    number = r"-?(\d+\.\d{4}|inf|nan)"
    metric_lines = [r"MSE: %s" % number, r"SNR_SR: %s" % number, r"SNR_LR: %s" % number, r"LSD: %s" % number]
    base = ["--input", str(files / "mono.wav"), "--load_pretrain", str(folder), "--encoding", "float32", "--crossover", "input"]
    _count(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "off.wav"), "--metrics_csv", str(tmp_path / "off.csv")]) == 0
    assert _count() == 0
    off = capsys.readouterr().out.splitlines()
    frames = _clip().numel()
    want = [re.escape("amplitude: full; low band: the model's"), r"crossover: the input below [\d.]+ Hz \(\d+ taps\)"] + metric_lines + \
           [re.escape("wrote %s (%d samples at 48000 Hz)" % (str(tmp_path / "off.wav"), frames)), re.escape("metrics: %s" % str(tmp_path / "off.csv"))]
    assert len(off) == len(want) and all(re.fullmatch(w, l) for w, l in zip(want, off)), off
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(G.METRICS_COLUMNS)
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--metrics_csv", str(tmp_path / "on.csv"), "--loudness", "-23"]) == 0
    assert _count() == 4
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if ": loudness " in l]
    assert len(extra) == 1 and [l.replace("on.wav", "off.wav").replace("on.csv", "off.csv") for l in on if l not in extra] == off
    m = re.fullmatch(re.escape(str(tmp_path / "on.wav")) + r": loudness input ([-+]\d+\.\d\d) LUFS, output ([-+]\d+\.\d\d) LUFS, gain ([-+]\d+\.\d\d) dB", extra[0])
    assert m and m.group(2) == "-23.00" and on.index(extra[0]) == len(on) - 2      # behind its file's `wrote` line
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == G.METRICS_COLUMNS + G.METRICS_COLUMNS_LOUDNESS and len(rows) == 3
    assert abs(float(rows[1][-2]) - (-23.0)) <= 1e-5 and "%+.2f" % float(rows[1][-3]) == m.group(1) and "%+.2f" % float(rows[1][-1]) == m.group(3)
    assert abs(R.integrated(_written(str(tmp_path / "on.wav")), RATE) - (-23.0)) <= 0.001
    # the metric lines and columns are those of the clip in front of the gain
    assert rows[1][:7] == list(csv.reader(open(str(tmp_path / "off.csv"))))[1][:7]
    # folder mode: one line per file
    assert G.main(["--input", str(files), "--output", str(tmp_path / "dir"), "--load_pretrain", str(folder), "--channels", "all",
                   "--crossover", "input", "--loudness", "report"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert sum(": loudness input " in l for l in lines) == 2 and all(l.endswith("gain +0.00 dB") for l in lines if ": loudness " in l)
    with pytest.raises(SystemExit):
        G.main(base + ["--output", str(tmp_path / "no.wav"), "--loudness", "5"])
    assert not os.path.exists(str(tmp_path / "no.wav"))
