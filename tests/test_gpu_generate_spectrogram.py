"""enhance_file(spectrogram=...) / enhance_folder(spectrogram=...) / --spectrogram on the GPU: the written PNG is
spectrogram_image of the clips the call returns, the wav does not change by a byte, two launches with the option and none
without, channels, folders, and the command line's lines.  The tiny model is the one of tests/test_gpu_lowband.py, restated."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SMALL = dict(n_fft=256, hop=64, width=96, height=40, range_db=80.0, gap=3)


def _opt(**kw):
    o = dict(gpu_ids=[0], isTrain=True, checkpoints_dir="/tmp/p2phd_test_ckpt", name="t", model="pix2pixHD",
             input_nc=2, output_nc=2, label_nc=0, hr_sampling_rate=48000, lr_sampling_rate=8000,
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


def _clip(n, start=0):
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    return torch.from_numpy(F["test_wav_excerpt_i16"][start:start + n].astype(np.float32) / 32768.0)


def _count(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(b"specimg", 1 if reset else 0)


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _payload(path):
    from pix2pixhdaudiosr_amd.data import wavio
    data, meta = wavio.read_payload(path)
    return bytes(data), meta


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("spectrogram_in")
    wavio.save(str(d / "mono.wav"), 0.5 * _clip(6000), 48000)
    wavio.save(str(d / "stereo.wav"), torch.stack([0.5 * _clip(4500, 500), -0.2 * _clip(4500, 3000)]), 48000)
    wavio.save(str(d / "low.wav"), 0.5 * _clip(900, 100), 8000)                   # a clip at the low rate
    return d


def _expected(res, channel, top_db=None, **plan):
    from pix2pixhdaudiosr_amd.generate import spectrogram_image
    rows = torch.stack([t[channel] for t in (res['lr'], res['sr'], res['hr']) if t is not None])
    return spectrogram_image(rows, top_db=top_db, **plan).cpu().numpy()


def test_picture_of_a_full_band_clip_is_three_panels_of_the_returned_clips(files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SPECTROGRAM_DEFAULTS, SuperResolver
    model, opt = _tiny()
    sr = SuperResolver(model, opt)
    sr.enhance_file(str(files / "mono.wav"), None)                # capture, tables, packed weights
    # without the option: no launch of the family, no key; the reference for the wav's bytes
    torch.manual_seed(5)
    _count(reset=True)
    plain = sr.enhance_file(str(files / "mono.wav"), str(tmp_path / "plain.wav"))
    assert _count() == 0 and 'spectrogram' not in plain
    assert sorted(plain) == ['hr', 'info', 'lr', 'metrics', 'sr']
    # with it, at the defaults
    png = str(tmp_path / "pictures" / "mono.png")                  # (a folder that does not exist yet)
    torch.manual_seed(5)
    _count(reset=True)
    res = sr.enhance_file(str(files / "mono.wav"), str(tmp_path / "with.wav"), spectrogram=png)
    assert _count() == 2
    assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'spectrogram', 'sr'] and res['hr'] is not None
    assert _payload(str(tmp_path / "with.wav"))[0] == _payload(str(tmp_path / "plain.wav"))[0]
    assert torch.equal(res['sr'], plain['sr']) and res['metrics'] == plain['metrics']
    d = SPECTROGRAM_DEFAULTS
    img = _png(png)
    assert img.shape == (3 * d['height'] + 2 * d['gap'], d['width'], 3) and img.dtype == np.uint8
    assert (img == _expected(res, 0)).all()
    info = res['spectrogram']
    assert sorted(info) == ['bins', 'frames', 'panels', 'path', 'range_db', 'top_db']
    assert (info['path'], info['panels'], info['frames'], info['bins'], info['range_db']) == (png, 3, 1 + 6000 // 256, 513, 90.0)
    from pix2pixhdaudiosr_amd.generate import stft_db
    rows = torch.stack([res['lr'][0], res['sr'][0], res['hr'][0]])
    assert info['top_db'] == float(stft_db(rows, 1024, 256).amax())
    # the panels differ: the input has nothing above its band, the original does
    H = d['height']
    assert not (img[:H] == img[2 * H + 2 * d['gap']:]).all()


def test_low_rate_input_gives_two_panels_and_options_reach_the_renderer(files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    sr = SuperResolver(model, opt, crossover='input')              # the second panel is the clip behind the crossover
    png = str(tmp_path / "low.png")
    torch.manual_seed(6)
    _count(reset=True)
    res = sr.enhance_file(str(files / "low.wav"), str(tmp_path / "low_out.wav"), is_lr_input=True, spectrogram=png,
                          spectrogram_opts=dict(SMALL, top_db=-6.0))
    assert _count() == 2 and res['hr'] is None
    img = _png(png)
    assert img.shape == (2 * SMALL['height'] + SMALL['gap'], SMALL['width'], 3)
    assert (img == _expected(res, 0, top_db=-6.0, **SMALL)).all()
    info = res['spectrogram']
    assert (info['panels'], info['frames'], info['bins'], info['top_db'], info['range_db']) == (2, 1 + res['sr'].shape[-1] // 64, 129, -6.0, 80.0)
    # the picture alone: no wav asked for, still one picture and the same pixels
    png2 = str(tmp_path / "low2.png")
    torch.manual_seed(6)
    res2 = sr.enhance_file(str(files / "low.wav"), None, is_lr_input=True, spectrogram=png2, spectrogram_opts=dict(SMALL, top_db=-6.0))
    assert torch.equal(res2['sr'], res['sr']) and (_png(png2) == img).all() and 'output' not in res2
    # together with the output stage: the figures, the wav and the picture come back behind one synchronisation
    png3 = str(tmp_path / "low3.png")
    torch.manual_seed(6)
    res3 = sr.enhance_file(str(files / "low.wav"), str(tmp_path / "low3.wav"), is_lr_input=True, report_peaks=True, spectrogram=png3,
                           spectrogram_opts=dict(SMALL, top_db=-6.0))
    assert (_png(png3) == img).all() and res3['output']['gain'] == 1.0
    assert _payload(str(tmp_path / "low3.wav"))[0] == _payload(str(tmp_path / "low_out.wav"))[0]


def test_channel_choice_and_its_refusals(files, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    sr = SuperResolver(model, opt)
    pictures = []
    for ch in (0, 1):
        png = str(tmp_path / ("ch%d.png" % ch))
        torch.manual_seed(7)
        res = sr.enhance_file(str(files / "stereo.wav"), None, channels='all', spectrogram=png, spectrogram_channel=ch, spectrogram_opts=SMALL)
        assert res['sr'].shape[0] == 2
        pictures.append(_png(png))
        assert (pictures[-1] == _expected(res, ch, **SMALL)).all()
    assert not (pictures[0] == pictures[1]).all()
    # a channel that is not written: ValueError, nothing written, nothing launched
    _count(reset=True)
    for path, kw in ((files / "mono.wav", dict(channels='all')), (files / "stereo.wav", dict(channels='first'))):
        with pytest.raises(ValueError, match=r"spectrogram_channel 1"):
            sr.enhance_file(str(path), str(tmp_path / "no.wav"), spectrogram=str(tmp_path / "no.png"), spectrogram_channel=1, **kw)
    assert _count() == 0 and not os.path.exists(str(tmp_path / "no.wav")) and not os.path.exists(str(tmp_path / "no.png"))
    with pytest.raises(ValueError, match=r"spectrogram n_fft"):
        sr.enhance_file(str(files / "mono.wav"), None, spectrogram=str(tmp_path / "no.png"), spectrogram_opts=dict(n_fft=100))
    with pytest.raises(ValueError, match=r"options of spectrogram=PATH"):
        sr.enhance_file(str(files / "mono.wav"), None, spectrogram_channel=1)


def test_folder_writes_one_picture_per_enhanced_file(files, tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny()
    src = tmp_path / "src"
    (src / "sub").mkdir(parents=True)
    wavio.save(str(src / "a.wav"), 0.5 * _clip(3000), 48000)
    wavio.save(str(src / "sub" / "b.wav"), torch.stack([0.5 * _clip(2500, 500), -0.2 * _clip(2500, 3000)]), 48000)
    (src / "broken.wav").write_bytes(b"RIFF....WAVEjunk")
    sr = SuperResolver(model, opt)
    plain = sr.enhance_folder(str(src), str(tmp_path / "out_plain"), channels='all', seed=11)
    assert all('spectrogram' not in r for r in plain)
    _count(reset=True)
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), channels='all', seed=11, spectrogram=str(tmp_path / "pics"), spectrogram_opts=SMALL)
    assert _count() == 4                                           # two enhanced files
    by = {r['path']: r for r in recs}
    assert by["broken.wav"]['error'] is not None and by["broken.wav"]['spectrogram'] is None
    found = sorted(os.path.relpath(os.path.join(d, f), str(tmp_path / "pics")) for d, _, fs in os.walk(str(tmp_path / "pics")) for f in fs)
    assert found == ["a.wav.png", os.path.join("sub", "b.wav.png")]
    for rel, panels in (("a.wav", 3), (os.path.join("sub", "b.wav"), 3)):
        r = by[rel]
        assert r['error'] is None and r['spectrogram']['path'] == str(tmp_path / "pics" / (rel + ".png")) and r['spectrogram']['panels'] == panels
        assert _png(r['spectrogram']['path']).shape == (3 * SMALL['height'] + 2 * SMALL['gap'], SMALL['width'], 3)
        assert open(str(tmp_path / "out" / rel), "rb").read() == open(str(tmp_path / "out_plain" / rel), "rb").read()
    # as a run of its own writes it
    torch.manual_seed(11)
    one = sr.enhance_file(str(src / "a.wav"), None, channels='all', spectrogram=str(tmp_path / "one.png"), spectrogram_opts=SMALL)
    assert (_png(str(tmp_path / "one.png")) == _png(by["a.wav"]['spectrogram']['path'])).all() and one['spectrogram']['panels'] == 3
    # channel 1: the mono file is that file's reported error, the stereo file gets its picture
    recs = sr.enhance_folder(str(src), str(tmp_path / "out1"), channels='all', seed=11, spectrogram=str(tmp_path / "pics1"),
                             spectrogram_channel=1, spectrogram_opts=SMALL)
    by = {r['path']: r for r in recs}
    assert "spectrogram_channel 1" in by["a.wav"]['error'] and by["a.wav"]['spectrogram'] is None and by["a.wav"]['written_channels'] == 0
    assert not os.path.exists(str(tmp_path / "pics1" / "a.wav.png")) and not os.path.exists(str(tmp_path / "out1" / "a.wav"))
    b = by[os.path.join("sub", "b.wav")]
    assert b['error'] is None and os.path.exists(b['spectrogram']['path'])
    with pytest.raises(ValueError, match=r"spectrogram width"):   # a bad plan: before any file is touched
        sr.enhance_folder(str(src), str(tmp_path / "out2"), spectrogram=str(tmp_path / "pics2"), spectrogram_opts=dict(width=0))
    assert not os.path.exists(str(tmp_path / "out2"))


def test_cli_lines_without_the_option_are_the_parents(files, tmp_path, capsys):
    """Without --spectrogram main() prints what it printed before the option existed -- the lines below are written out from
    the formats that tests/test_gpu_generate_crossover.py and tests/test_outstage_host.py pin in parts ('N of M files enhanced',
    no line of an option that is off) -- and with it exactly one `spectrogram:` line per picture more."""
    from pix2pixhdaudiosr_amd import generate as G
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.models.models import create_model
    d_in = tmp_path / "in"
    d_in.mkdir()
    wavio.save(str(d_in / "a.wav"), _clip(6000), 48000)
    wavio.save(str(d_in / "b.wav"), torch.stack([_clip(3500, 500), -_clip(3500, 900)]), 48000)
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

    # folder mode
    base = ["--input", str(d_in), "--load_pretrain", str(folder), "--channels", "all"]
    assert G.main(base + ["--output", str(tmp_path / "off")]) == 0
    off = capsys.readouterr().out.splitlines()
    want = [re.escape("amplitude: full; low band: the model's"),
            re.escape("wrote %s (6000 samples at 48000 Hz, 1 channel)" % os.path.join(str(tmp_path / "off"), "a.wav")),
            re.escape("wrote %s (3500 samples at 48000 Hz, 2 channels)" % os.path.join(str(tmp_path / "off"), "b.wav")),
            re.escape("2 of 2 files enhanced, 0 skipped"),
            r"mean over 3 channels: MSE %s  SNR_SR %s  SNR_LR %s  LSD %s" % ((number,) * 4)]
    assert len(off) == len(want) and all(re.fullmatch(w, l) for w, l in zip(want, off)), off
    assert G.main(base + ["--output", str(tmp_path / "on"), "--spectrogram", str(tmp_path / "pics"), "--spectrogram_size", "80x32",
                          "--spectrogram_n_fft", "256", "--spectrogram_hop", "64", "--spectrogram_channel", "0"]) == 0
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if l.startswith("spectrogram: ")]
    assert len(extra) == 2 and [l.replace(str(tmp_path / "on"), str(tmp_path / "off")) for l in on if l not in extra] == off
    assert extra[0].startswith("spectrogram: %s (3 panels, 94 frames x 129 bins, 90.0 dB down from " % str(tmp_path / "pics" / "a.wav.png"))
    assert on.index(extra[0]) == 2 and on.index(extra[1]) == 4      # behind its file's `wrote` line
    for name in ("a.wav", "b.wav"):
        assert _png(str(tmp_path / "pics" / (name + ".png"))).shape == (3 * 32 + 2 * 2, 80, 3)
        assert open(str(tmp_path / "on" / name), "rb").read() == open(str(tmp_path / "off" / name), "rb").read()

    # file mode
    base = ["--input", str(d_in / "a.wav"), "--load_pretrain", str(folder)]
    assert G.main(base + ["--output", str(tmp_path / "off.wav")]) == 0
    off = capsys.readouterr().out.splitlines()
    want = [re.escape("amplitude: full; low band: the model's")] + metric_lines + [re.escape("wrote %s (6000 samples at 48000 Hz)" % str(tmp_path / "off.wav"))]
    assert len(off) == len(want) and all(re.fullmatch(w, l) for w, l in zip(want, off)), off
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--spectrogram", str(tmp_path / "a.png"), "--spectrogram_top_db", "0",
                          "--spectrogram_range_db", "100"]) == 0
    on = capsys.readouterr().out.splitlines()
    assert [l.replace("on.wav", "off.wav") for l in on[:-1]] == off
    assert on[-1] == "spectrogram: %s (3 panels, 24 frames x 513 bins, 100.0 dB down from +0.0 dB)" % str(tmp_path / "a.png")
    assert _png(str(tmp_path / "a.png")).shape == (3 * 512 + 2 * 2, 1600, 3)
    assert open(str(tmp_path / "on.wav"), "rb").read() == open(str(tmp_path / "off.wav"), "rb").read()
