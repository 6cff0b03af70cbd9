"""enhance_file(true_peak=True) / enhance_folder(true_peak=True) / --true_peak on the GPU: without the option nothing changes and
nothing is launched; with it the result's 'output' carries the true peak, which the restatement of tests/_truepeak_ref.py confirms
on the returned clip; clip='guard' leaves the written file with its true peak at the ceiling, clip='error' refuses a file whose
samples fit but whose crests do not; the guard sees the clip behind the loudness gain; folders, the CSV column and the command
line's line.  The tiny model and the crossover='input' resolver are those of tests/test_gpu_generate_loudness.py, restated."""
import csv
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _truepeak_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE = 48000
OUTPUT_KEYS = ['clipped', 'gain', 'nonfinite', 'peak', 'peak_dbfs', 'true_peak', 'true_peak_dbtp']


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
    """The stored excerpt (0.5 s at 48 kHz), forwards and then backwards."""
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    x = torch.from_numpy(F["test_wav_excerpt_i16"].astype(np.float32) / 32768.0)
    return torch.cat([x, 0.7 * x.flip(0)])[:7 * 4800 + 321]


def _count(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(b"truepeak", 1 if reset else 0)


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
    """The plan's table as the library fills it (tests/test_truepeak_host.py holds it to the restatement's), float32 numpy."""
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients, truepeak_plan
    plan = truepeak_plan(RATE)
    return true_peak_coefficients(plan['factor'], plan['taps_per_phase'], plan['beta']).numpy()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("truepeak_in")
    x = _clip()
    wavio.save(str(d / "mono.wav"), 0.5 * x, RATE)
    wavio.save(str(d / "stereo.wav"), torch.stack([0.5 * x[:5 * 4800 + 77], -0.3 * x.flip(0)[:5 * 4800 + 77]]), RATE)
    return d


@pytest.fixture(scope="module")
def tone(tmp_path_factory):
    """0.6 s of a 1 kHz tone whose samples straddle every crest (48 per period, the nearest ones 3.75 degrees on either side: they
    read cos(3.75 deg), 0.019 dB under the crest), under raised-cosine ramps; inside the band the crossover takes from the input."""
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("truepeak_tone")
    x = 0.4 * R.ramped_tone(1000.0 / RATE, np.radians(3.75), n=6 * 4800, ramp=2400)
    wavio.save(str(d / "tone.wav"), torch.from_numpy(x.astype(np.float32)), RATE, encoding='float32')
    return str(d / "tone.wav")


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    return SuperResolver(model, opt, crossover='input')


@pytest.fixture(scope="module")
def plain(resolver, files, tmp_path_factory):
    """The run without the option that the others are compared with: seed 5, float32."""
    out = str(tmp_path_factory.mktemp("truepeak_plain") / "plain.wav")
    resolver.enhance_file(str(files / "mono.wav"), None)          # capture, tables, packed weights
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32')
    assert _count() == 0
    return res, out


def _check_report(output, rows, table):
    """The result's true-peak figures against the restatement on the clip they were measured on, within the dot-product bound."""
    want, bound = R.true_peak(rows, table), R.dot_bound(rows, table)
    got = np.array(output['true_peak'], dtype=np.float64)
    print("true peak %s, restatement %s, error / bound %s; peak %s" % (got, want, np.abs(got - want) / bound, output['peak']))
    assert got.shape == want.shape and (bound > 0).all() and (np.abs(got - want) <= bound).all()
    assert all(t >= p for t, p in zip(output['true_peak'], output['peak']))
    assert output['true_peak_dbtp'] == [20.0 * math.log10(v) for v in output['true_peak']]


def test_option_off_changes_nothing(resolver, files, plain, tmp_path):
    res0, out0 = plain
    assert sorted(res0) == ['hr', 'info', 'lr', 'metrics', 'sr']
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), str(tmp_path / "off.wav"), encoding='float32')
    assert _count() == 0 and sorted(res) == sorted(res0)
    assert _bytes(str(tmp_path / "off.wav")) == _bytes(out0) and torch.equal(res['sr'], res0['sr']) and res['metrics'] == res0['metrics']


def test_option_off_by_keyword_changes_nothing(resolver, files, plain, tmp_path):
    res0, out0 = plain
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), str(tmp_path / "off.wav"), encoding='float32', true_peak=False)
    assert _count() == 0 and sorted(res) == sorted(res0)
    assert _bytes(str(tmp_path / "off.wav")) == _bytes(out0) and torch.equal(res['sr'], res0['sr']) and res['metrics'] == res0['metrics']
    with pytest.raises(ValueError, match="true_peak must be a bool"):
        resolver.enhance_file(str(files / "mono.wav"), None, true_peak='yes')


def test_report_alone_adds_the_output_and_leaves_the_bytes(resolver, files, plain, table, tmp_path):
    res0, out0 = plain
    out = str(tmp_path / "r.wav")
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32', true_peak=True)
    assert _count() == 1                                           # one launch per file
    assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'output', 'sr'] and sorted(res['output']) == OUTPUT_KEYS
    assert _bytes(out) == _bytes(out0) and torch.equal(res['sr'], res0['sr']) and res['metrics'] == res0['metrics']
    assert res['output']['gain'] == 1.0 and len(res['output']['true_peak']) == 1
    _check_report(res['output'], res['sr'].cpu().numpy(), table)
    # the integer encodings: the same bytes as without the option, the same figures
    for encoding in ('pcm16', 'pcm24'):
        a, b = str(tmp_path / ("a_%s.wav" % encoding)), str(tmp_path / ("b_%s.wav" % encoding))
        torch.manual_seed(5)
        resolver.enhance_file(str(files / "mono.wav"), a, encoding=encoding)
        torch.manual_seed(5)
        other = resolver.enhance_file(str(files / "mono.wav"), b, encoding=encoding, true_peak=True)
        assert _bytes(a) == _bytes(b) and other['output']['true_peak'] == res['output']['true_peak']
    # measuring alone: no file asked for, the same figures; beside report_peaks: the same keys
    torch.manual_seed(5)
    only = resolver.enhance_file(str(files / "mono.wav"), None, encoding='float32', true_peak=True, report_peaks=True)
    assert only['output'] == res['output']


@pytest.mark.parametrize("encoding", ("float32", "pcm24", "pcm16"))
def test_guard_puts_the_true_peak_of_the_written_file_at_the_ceiling(resolver, files, table, tmp_path, encoding):
    """clip='guard', ceiling_dbfs=-20: the written stereo file, re-read and measured by the restatement, has its largest true peak
    at 10^(-20/20) -- within the dot-product bound, plus for the integer encodings the half LSB every sample may move by, through
    the filter: 0.5 LSB max_p sum_k |c[p][k]|."""
    out = str(tmp_path / "g.wav")
    ceiling = 10.0 ** (-20.0 / 20.0)
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "stereo.wav"), out, channels='all', encoding=encoding, clip='guard', ceiling_dbfs=-20.0, true_peak=True)
    assert _count() == 1
    o = res['output']
    _check_report(o, res['sr'].cpu().numpy(), table)
    assert len(o['true_peak']) == 2 and max(o['true_peak']) > ceiling and o['gain'] < 1.0       # the guard has something to do
    assert o['gain'] == float(R.gain(o['true_peak'], ceiling))
    y = _written(out)
    lsb = {'float32': 0.0, 'pcm24': 2.0 ** -23, 'pcm16': 2.0 ** -15}[encoding]
    margin = R.dot_bound(y, table).max() + 0.5 * lsb * np.abs(table.astype(np.float64)).sum(axis=1).max()
    got = R.true_peak(y, table)
    print("%s: written true peaks %s, ceiling %.9f, margin %.3e, gain %r" % (encoding, got, ceiling, margin, o['gain']))
    assert abs(got.max() - ceiling) <= margin
    # one gain for both channels: the quieter one keeps its distance (two margins for either ratio)
    assert abs(got.min() / got.max() - min(o['true_peak']) / max(o['true_peak'])) <= 4.0 * margin / got.max()
    if encoding == 'float32':
        assert np.array_equal(y, res['sr'].cpu().numpy() * np.float32(o['gain']))
    # the sample-peak guard of the same call leaves the crests above the ceiling, or at it where a sample is the crest
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "stereo.wav"), out, channels='all', encoding=encoding, clip='guard', ceiling_dbfs=-20.0)
    assert R.true_peak(_written(out), table).max() >= got.max() - margin


def test_error_refuses_a_file_whose_samples_fit_but_whose_true_peak_does_not(resolver, tone, tmp_path):
    from pix2pixhdaudiosr_amd.generate import ClipError
    src = tone
    torch.manual_seed(5)
    first = resolver.enhance_file(src, None, channels='all', encoding='float32', loudness='report', true_peak=True)
    p, t = max(first['output']['peak']), max(first['output']['true_peak'])
    print("sample peak %.6f, true peak %.6f (%.4f dB apart), %.3f LUFS" % (p, t, 20.0 * np.log10(t / p), first['loudness']['measured']))
    assert t > p * 1.0005                                          # a crest between the samples, far beyond the roundings of the gain (1e-7)
    # the level at which 1.0 lies half way (in dB) between the largest sample and the largest crest
    target = first['loudness']['measured'] - 10.0 * np.log10(p * t)
    assert -70.0 <= target <= 0.0
    torch.manual_seed(5)
    seen = resolver.enhance_file(src, None, channels='all', encoding='float32', loudness=target, true_peak=True)
    assert sum(seen['output']['clipped']) == 0 and max(seen['output']['peak']) < 1.0 < max(seen['output']['true_peak'])     # the precondition
    out = str(tmp_path / "e.wav")
    torch.manual_seed(5)
    with pytest.raises(ClipError) as e:
        resolver.enhance_file(src, out, channels='all', encoding='float32', loudness=target, clip='error', true_peak=True)
    text = str(e.value)
    assert out in text and "dBTP" in text and "%+.2f" % max(seen['output']['true_peak_dbtp']) in text and "(0 samples would clip)" in text
    assert not os.path.exists(out)
    # without the option the same call writes the file: no sample clips
    torch.manual_seed(5)
    resolver.enhance_file(src, out, channels='all', encoding='float32', loudness=target, clip='error')
    assert os.path.exists(out)
    # and 'clamp' with the option only reports
    torch.manual_seed(5)
    res = resolver.enhance_file(src, str(tmp_path / "c.wav"), channels='all', encoding='float32', loudness=target, true_peak=True)
    assert _bytes(str(tmp_path / "c.wav")) == _bytes(out) and res['output']['gain'] == 1.0


def test_guard_sees_the_clip_behind_the_loudness_gain(resolver, files, plain, table, tmp_path):
    res0, _ = plain
    out = str(tmp_path / "l.wav")
    ceiling = 10.0 ** (-30.0 / 20.0)
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32', loudness=-23.0, clip='guard', ceiling_dbfs=-30.0, true_peak=True)
    o = res['output']
    assert abs(res['loudness']['gain_db']) > 0.5 and not torch.equal(res['sr'], res0['sr'])    # 'sr' is the clip behind the loudness gain
    _check_report(o, res['sr'].cpu().numpy(), table)              # ... and the one that was measured
    assert o['gain'] == float(R.gain(o['true_peak'], ceiling)) and o['gain'] < 0.9
    y = _written(out)
    got, margin = R.true_peak(y, table), R.dot_bound(y, table)
    print("written true peak %s, ceiling %.9f, margin %s" % (got, ceiling, margin))
    assert abs(got[0] - ceiling) <= margin[0]


def test_folder_records_and_csv_column(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_TRUE_PEAK, write_metrics_csv
    plain = resolver.enhance_folder(str(files), str(tmp_path / "off"), channels='all', seed=11)
    assert all('output' not in r for r in plain)
    _count(reset=True)
    recs = resolver.enhance_folder(str(files), str(tmp_path / "on"), channels='all', seed=11, true_peak=True)
    assert _count() == 2                                           # one per file
    by = {r['path']: r for r in recs}
    for name in ("mono.wav", "stereo.wav"):
        assert sorted(by[name]['output']) == OUTPUT_KEYS
        torch.manual_seed(11)
        one = resolver.enhance_file(str(files / name), str(tmp_path / ("one_" + name)), channels='all', true_peak=True)
        assert by[name]['output'] == one['output']
        assert _bytes(str(tmp_path / "on" / name)) == _bytes(str(tmp_path / ("one_" + name))) == _bytes(str(tmp_path / "off" / name))
    write_metrics_csv(str(tmp_path / "off.csv"), plain)
    write_metrics_csv(str(tmp_path / "on.csv"), recs, true_peak=True)
    rows_off, rows_on = (list(csv.reader(open(str(tmp_path / n)))) for n in ("off.csv", "on.csv"))
    assert tuple(rows_off[0]) == METRICS_COLUMNS and tuple(rows_on[0]) == METRICS_COLUMNS + METRICS_COLUMNS_TRUE_PEAK
    assert len(rows_on) == 1 + 3 + 1                               # three written channels and the mean
    for row in rows_on[1:-1]:
        assert float(row[-1]) == by[row[0]]['output']['true_peak_dbtp'][int(row[1])]
    assert [r[:-1] for r in rows_on] == rows_off                  # the other columns do not move
    with pytest.raises(ValueError, match="true_peak must be a bool"):      # before any file is touched
        resolver.enhance_folder(str(files), str(tmp_path / "never"), true_peak=1)
    assert not os.path.exists(str(tmp_path / "never"))


def test_cli_line_and_csv_header(files, tmp_path, capsys):
    """Without --true_peak main() prints the lines it printed before the option existed and the table has the columns it had;
    with it, one peak line per file that carries the true peak, and one column more."""
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
    want = [re.escape("amplitude: full; low band: the model's"), r"crossover: the input below [\d.]+ Hz \(\d+ taps\)"] + metric_lines + \
           [re.escape("wrote %s (%d samples at 48000 Hz)" % (str(tmp_path / "off.wav"), _clip().numel())), re.escape("metrics: %s" % str(tmp_path / "off.csv"))]
    assert len(off) == len(want) and all(re.fullmatch(w, l) for w, l in zip(want, off)), off
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(G.METRICS_COLUMNS)
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--metrics_csv", str(tmp_path / "on.csv"), "--true_peak"]) == 0
    assert _count() == 1
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if "true peak" in l]
    assert len(extra) == 1 and [l.replace("on.wav", "off.wav").replace("on.csv", "off.csv") for l in on if l not in extra] == off
    m = re.fullmatch(re.escape(str(tmp_path / "on.wav")) + r": peak ([-+]\d+\.\d\d) dBFS, true peak ([-+]\d+\.\d\d) dBTP, 0 clipped, 0 non-finite, "
                     r"gain 1\.000000", extra[0])
    assert m and float(m.group(2)) >= float(m.group(1)) and on.index(extra[0]) == len(on) - 2      # behind its file's `wrote` line
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == G.METRICS_COLUMNS + G.METRICS_COLUMNS_TRUE_PEAK and len(rows) == 3
    assert "%+.2f" % float(rows[1][-1]) == m.group(2) and rows[1][:7] == list(csv.reader(open(str(tmp_path / "off.csv"))))[1][:7]
    assert _bytes(str(tmp_path / "on.wav")) == _bytes(str(tmp_path / "off.wav"))
    # folder mode: one line per file; with --clip guard the line reports the true-peak gain
    assert G.main(["--input", str(files), "--output", str(tmp_path / "dir"), "--load_pretrain", str(folder), "--channels", "all",
                   "--crossover", "input", "--true_peak", "--clip", "guard", "--ceiling_dbfs", "-20"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if "true peak" in l]
    assert len(lines) == 2 and all(re.search(r"dBTP, \d+ clipped, \d+ non-finite, gain 0\.\d{6}$", l) for l in lines), lines
