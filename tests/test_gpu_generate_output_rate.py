"""enhance_file(output_rate=...) / enhance_folder(output_rate=...) / --output_rate on the GPU: without the option, or with the model's
own rate, nothing changes and nothing is launched; with it the file is written at the new rate, its payload the encoder's bytes of
rate_convert on the plain run's clip; the loudness, true-peak, guard and limiter stages run on the converted clip at the output
rate -- the written file, re-read and measured at 44100 Hz by the restatements, has its true peak at the ceiling and its loudness
where the reported gains put it; folders, the command line's lines and the refusals.  The tiny model and the crossover='input'
resolver are those of tests/test_gpu_generate_truepeak.py, restated."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _loudness_ref as LR
import _truepeak_ref as TR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE, OUT = 48000, 44100
RESULT_KEYS = ['hr', 'info', 'lr', 'metrics', 'sr']
RATE_KEYS = ['atten_db', 'model_rate', 'n', 'o', 'passband_hz', 'rate', 'stopband_hz', 'taps_per_phase']


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


def _count(reset=False, family=b"rateconv"):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(family, 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _written(path, rate):
    from pix2pixhdaudiosr_amd.data import wavio
    data, got = wavio.load(path)
    assert got == rate
    return data.numpy()


def _frames(L):
    return -((-L * 147) // 160)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("output_rate_in")
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
    """The runs without the argument that the others are compared with: seed 5, float32 and pcm16."""
    d = tmp_path_factory.mktemp("output_rate_plain")
    resolver.enhance_file(str(files / "mono.wav"), None)          # capture, tables, packed weights
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), str(d / "f32.wav"), encoding='float32')
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "mono.wav"), str(d / "i16.wav"))
    assert _count() == 0
    return res, str(d / "f32.wav"), str(d / "i16.wav")


@pytest.fixture(scope="module")
def tp_table():
    """The true-peak table of a clip at 44100 Hz as the library fills it, float32 numpy."""
    from pix2pixhdaudiosr_amd.generate import true_peak_coefficients, truepeak_plan
    plan = truepeak_plan(OUT)
    return true_peak_coefficients(plan['factor'], plan['taps_per_phase'], plan['beta']).numpy()


# (a) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", (None, RATE))
def test_option_off_changes_nothing(resolver, files, plain, tmp_path, rate):
    res0, f32, i16 = plain
    assert sorted(res0) == RESULT_KEYS
    _count(reset=True)
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files / "mono.wav"), str(tmp_path / "a.wav"), encoding='float32', output_rate=rate)
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "mono.wav"), str(tmp_path / "b.wav"), output_rate=rate)
    assert _count() == 0 and sorted(res) == RESULT_KEYS
    assert _bytes(str(tmp_path / "a.wav")) == _bytes(f32) and _bytes(str(tmp_path / "b.wav")) == _bytes(i16)
    assert torch.equal(res['sr'], res0['sr']) and res['metrics'] == res0['metrics']


# (b) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", ("float32", "pcm16"))
def test_plain_conversion_writes_the_converted_clip(resolver, files, plain, tmp_path, encoding):
    from pix2pixhdaudiosr_amd import generate as g
    from pix2pixhdaudiosr_amd.data import wavio
    res0 = plain[0]
    out = str(tmp_path / "c.wav")
    _count(reset=True)
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding=encoding, output_rate=OUT)
    assert _count() == 1                                           # one launch per file
    L = _clip().numel()
    info = wavio.info(out)
    assert (info.sample_rate, info.num_frames, info.num_channels) == (OUT, _frames(L), 1)
    want = g.rate_convert(res0['sr'], RATE, OUT)
    assert want.shape == (1, _frames(L)) and torch.equal(res['sr'].view(torch.int32), want.view(torch.int32))
    payload = g.pcm_encode(want, encoding).cpu().numpy().tobytes()
    assert len(payload) == _frames(L) * (4 if encoding == 'float32' else 2) and _bytes(out)[-len(payload):] == payload
    # everything that compares clips at the model's rate stays; the result says what was done
    assert sorted(res) == sorted(RESULT_KEYS + ['output_rate']) and sorted(res['output_rate']) == RATE_KEYS
    assert torch.equal(res['lr'], res0['lr']) and torch.equal(res['hr'], res0['hr']) and res['metrics'] == res0['metrics']
    r = res['output_rate']
    assert (r['rate'], r['model_rate'], r['o'], r['n'], r['taps_per_phase'], r['atten_db']) == (OUT, RATE, 160, 147, 92, 120.0)
    assert r['passband_hz'] == pytest.approx(19999.35) and r['stopband_hz'] == pytest.approx(24100.65)


# (c) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,ceiling_dbfs", (("float32", -1.0), ("pcm16", -1.0), ("float32", -20.0), ("pcm16", -20.0)))
def test_output_stage_holds_what_is_written(resolver, files, tp_table, tmp_path, encoding, ceiling_dbfs):
    """loudness=-23, true_peak=True, clip='guard': the written file, re-read and measured at 44100 Hz by the restatements.  Its true
    peak is at the ceiling where the guard had something to do (at -20 dBTP it must have) and under it otherwise -- within the
    dot-product bound, plus for pcm16 the half LSB every sample may move by, through the filter, as tests/test_gpu_generate_truepeak.py
    asserts it at 48000 --, and its loudness is the reported output level plus the guard's gain, within 0.001 LU."""
    out = str(tmp_path / "s.wav")
    ceiling = 10.0 ** (ceiling_dbfs / 20.0)
    _count(reset=True)
    _count(reset=True, family=b"truepeak")
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files / "stereo.wav"), out, channels='all', encoding=encoding, loudness=-23.0, true_peak=True, clip='guard',
                                ceiling_dbfs=ceiling_dbfs, output_rate=OUT)
    assert _count() == 1 and _count(family=b"truepeak") == 1
    o, loud = res['output'], res['loudness']
    y = _written(out, OUT)
    assert y.shape == (2, _frames(5 * 4800 + 77)) == tuple(res['sr'].shape)
    # the figures are those of the converted clip at the output rate
    rows = res['sr'].cpu().numpy()
    want, bound = TR.true_peak(rows, tp_table), TR.dot_bound(rows, tp_table)
    assert (np.abs(np.array(o['true_peak'], dtype=np.float64) - want) <= bound).all()
    assert o['gain'] == float(TR.gain(o['true_peak'], ceiling))
    lsb = {'float32': 0.0, 'pcm16': 2.0 ** -15}[encoding]
    margin = TR.dot_bound(y, tp_table).max() + 0.5 * lsb * np.abs(tp_table.astype(np.float64)).sum(axis=1).max()
    got = TR.true_peak(y, tp_table).max()
    print("%s, %g dBTP: written true peak %.9f, ceiling %.9f, margin %.3e, gain %r" % (encoding, ceiling_dbfs, got, ceiling, margin, o['gain']))
    if ceiling_dbfs == -20.0:
        assert o['gain'] < 1.0                                     # the guard has something to do
    if o['gain'] < 1.0:
        assert abs(got - ceiling) <= margin
    else:
        assert got <= ceiling + margin
    # loudness: the input at the model's rate, the generated clip at the output rate
    assert abs(loud['input'] - LR.integrated(res['lr'].cpu().numpy(), RATE)) <= 0.001
    assert loud['target'] == -23.0 and abs(loud['output'] - (-23.0)) <= 1e-4
    unscaled = rows.astype(np.float64) / 10.0 ** (loud['gain_db'] / 20.0)
    assert abs(loud['measured'] - LR.integrated(unscaled, OUT)) <= 0.001
    level = LR.integrated(y, OUT)
    print("written %.4f LUFS, reported %.4f %+.4f dB" % (level, loud['output'], 20.0 * np.log10(o['gain'])))
    assert abs(level - (loud['output'] + 20.0 * np.log10(o['gain']))) <= 0.001


# (d) ---------------------------------------------------------------------------------------
def test_limiter_runs_at_the_output_rate(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import limiter_plan
    out = str(tmp_path / "l.wav")
    _count(reset=True)
    _count(reset=True, family=b"limiter")
    torch.manual_seed(5)
    res = resolver.enhance_file(str(files / "mono.wav"), out, encoding='float32', loudness=-23.0, clip='guard', ceiling_dbfs=-20.0, limiter=True,
                                output_rate=OUT)
    assert _count() == 1 and _count(family=b"limiter") == 2
    lim, plan = res['output']['limiter'], limiter_plan(OUT)
    assert (lim['lookahead'], lim['hold']) == (plan['lookahead'], plan['hold']) != tuple(limiter_plan(RATE).values())
    assert 0 < lim['limited_samples'] <= res['sr'].shape[-1] == _frames(_clip().numel()) and lim['max_reduction_db'] < 0.0
    assert _written(out, OUT).shape == (1, _frames(_clip().numel()))


# (e) ---------------------------------------------------------------------------------------
def test_folder_mode(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    plain = resolver.enhance_folder(str(files), str(tmp_path / "off"), channels='all', seed=11)
    same = resolver.enhance_folder(str(files), str(tmp_path / "same"), channels='all', seed=11, output_rate=RATE)
    assert [sorted(r) for r in same] == [sorted(r) for r in plain] and [r['out_frames'] for r in same] == [r['out_frames'] for r in plain]
    assert all('output_rate' not in r for r in plain)
    _count(reset=True)
    recs = resolver.enhance_folder(str(files), str(tmp_path / "on"), channels='all', seed=11, output_rate=OUT)
    assert _count() == 2                                           # one per file
    by = {r['path']: r for r in recs}
    for name, frames in (("mono.wav", _clip().numel()), ("stereo.wav", 5 * 4800 + 77)):
        assert _bytes(str(tmp_path / "same" / name)) == _bytes(str(tmp_path / "off" / name))
        r = by[name]
        assert r['error'] is None and r['frames'] == frames and r['out_frames'] == _frames(frames) and sorted(r['output_rate']) == RATE_KEYS
        info = wavio.info(str(tmp_path / "on" / name))
        assert (info.sample_rate, info.num_frames) == (OUT, _frames(frames))
        torch.manual_seed(11)
        resolver.enhance_file(str(files / name), str(tmp_path / ("one_" + name)), channels='all', output_rate=OUT)
        assert _bytes(str(tmp_path / "on" / name)) == _bytes(str(tmp_path / ("one_" + name)))


def test_cli_lines(files, tmp_path, capsys):
    """Without --output_rate main() prints the lines it printed before the option existed; with it one start-up line more, and the
    `wrote` line states the written length and rate."""
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
    base = ["--input", str(files / "mono.wav"), "--load_pretrain", str(folder), "--crossover", "input"]
    L = _clip().numel()
    _count(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "off.wav")]) == 0
    off = capsys.readouterr().out.splitlines()
    assert G.main(base + ["--output", str(tmp_path / "same.wav"), "--output_rate", str(RATE)]) == 0
    same = capsys.readouterr().out.splitlines()
    assert _count() == 0 and [l.replace("same.wav", "off.wav") for l in same] == off
    assert _bytes(str(tmp_path / "same.wav")) == _bytes(str(tmp_path / "off.wav"))
    assert off[-1] == "wrote %s (%d samples at 48000 Hz)" % (str(tmp_path / "off.wav"), L) and not any("output rate" in l for l in off)
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--output_rate", str(OUT)]) == 0
    assert _count() == 1
    on = capsys.readouterr().out.splitlines()
    line = "output rate: 44100 Hz (92 taps x 147 phases, flat to 20.00 kHz, -120 dB from 24.10 kHz)"
    assert on.count(line) == 1 and on[-1] == "wrote %s (%d samples at 44100 Hz)" % (str(tmp_path / "on.wav"), _frames(L))
    assert [l for l in on if l != line][:-1] == off[:-1] and on.index(line) < len(on) - 1
    assert _written(str(tmp_path / "on.wav"), OUT).shape == (1, _frames(L))
    # folder mode: the rate in every `wrote` line
    assert G.main(["--input", str(files), "--output", str(tmp_path / "dir"), "--load_pretrain", str(folder), "--channels", "all", "--crossover", "input",
                   "--output_rate", str(OUT)]) == 0
    lines = capsys.readouterr().out.splitlines()
    wrote = [l for l in lines if l.startswith("wrote ")]
    assert lines.count(line) == 1 and len(wrote) == 2 and all(re.search(r"\(\d+ samples at 44100 Hz, \d channels?\)$", l) for l in wrote), lines
    assert "(%d samples at 44100 Hz, 1 channel)" % _frames(L) in wrote[0]
    # refused before anything is loaded or written
    for extra in (["--output_rate", "7999"], ["--output_rate", str(OUT), "--spectrogram", str(tmp_path / "p.png")], ["--output_rate", "8000"]):
        with pytest.raises(SystemExit):
            G.main(base + ["--output", str(tmp_path / "never.wav")] + extra)
        assert "output_rate" in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "never.wav"))


# (f) ---------------------------------------------------------------------------------------
def test_refusals(resolver, files, tmp_path):
    src = str(files / "mono.wav")
    with pytest.raises(ValueError, match="spectrogram is not built with output_rate"):
        resolver.enhance_file(src, str(tmp_path / "n.wav"), output_rate=OUT, spectrogram=str(tmp_path / "p.png"))
    with pytest.raises(ValueError, match="output_rate is not built for loudness_scope='folder'"):
        resolver.enhance_folder(str(files), str(tmp_path / "never"), loudness=-23.0, loudness_scope='folder', output_rate=OUT)
    with pytest.raises(ValueError, match="spectrogram is not built with output_rate"):
        resolver.enhance_folder(str(files), str(tmp_path / "never"), spectrogram=str(tmp_path / "pics"), output_rate=OUT)
    for bad in (7999, 44100.0, True, "44100"):
        with pytest.raises(ValueError, match="output_rate must be an int >= 8000"):
            resolver.enhance_file(src, str(tmp_path / "n.wav"), output_rate=bad)
    with pytest.raises(ValueError, match="output_rate 8000: rateconv_plan: 48000 -> 8000 Hz"):
        resolver.enhance_file(src, str(tmp_path / "n.wav"), output_rate=8000)
    with pytest.raises(ValueError, match="multiple of 10"):       # the loudness of the written clip is measured in hops of rate / 10
        resolver.enhance_file(src, str(tmp_path / "n.wav"), output_rate=32005, loudness='report')
    assert not os.path.exists(str(tmp_path / "n.wav")) and not os.path.exists(str(tmp_path / "never")) and not os.path.exists(str(tmp_path / "p.png"))
