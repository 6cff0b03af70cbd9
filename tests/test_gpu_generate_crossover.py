"""SuperResolver(crossover='input') and --crossover (generate.py, csrc/xover.hip) on the GPU: the option is the crossover
kernel applied to what the pipeline returns without it, at level gain / 2; a pass-through generator pins that level; launch
counts; the command line.  The tiny model is the one of tests/test_gpu_lowband.py, restated."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FAMILIES = ("gconv", "halo", "cls_skip", "march", "march_w", "wgrad", "splitk", "tile256", "tile128x192", "dfirst", "dlast", "c7",
            "thin_wgrad", "timed_pack", "timed_frames", "stitch", "pcm", "metrics_rows")


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


def _tiny(mdct_type):
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


def _rows(C, L):
    x = 0.5 * _clip(L)
    return torch.stack([x, -0.7 * x.flip(-1)][:C]).to(DEV)


def _noise(sr, rows, seed):
    shape = sr.noise_shape(1)
    return torch.randn((rows,) + shape[1:], generator=torch.Generator().manual_seed(seed)).to(DEV)


def _taps_dev(plan):
    from pix2pixhdaudiosr_amd.generate import crossover_coefficients
    return crossover_coefficients(*plan).to(DEV)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class PassThrough:
    """`inference` returns the encoding of its own input, as generator output and as input spectrogram."""

    def __init__(self, real):
        self.real, self.mdct_type, self.device = real, real.mdct_type, real.device

    def inference(self, lr_audio, inst, noise=None):
        spectro, pha, norm = self.real.to_spectro(lr_audio, mask=False)
        return spectro, pha, norm, spectro


# ------------------------------------------------------------------------------------------
# composition
# ------------------------------------------------------------------------------------------
def _composes(model, opt, C, L, noise_seed, crossover_hz=None, crossover_taps=None, **kw):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, crossover, crossover_plan, segment_plan
    x = _rows(C, L)
    plain = SuperResolver(model, opt, **kw)
    crossed = SuperResolver(model, opt, crossover='input', crossover_hz=crossover_hz, crossover_taps=crossover_taps, **kw)
    assert plain.crossover_plan is None
    assert crossed.crossover_plan == crossover_plan(opt.hr_sampling_rate, opt.lr_sampling_rate, crossover_hz, crossover_taps)
    assert crossed.gain == plain.gain and crossed.reference_amplitude == plain.reference_amplitude
    S = segment_plan(L, opt.segment_length, kw.get('overlap', 0.25))[0]
    noise = _noise(plain, C * S, noise_seed)
    base = plain.enhance_lr(x, noise=noise)
    want = crossover(base, x, plain.gain / 2.0, _taps_dev(crossed.crossover_plan))
    got = crossed.enhance_lr(x, noise=noise)
    assert tuple(got.shape) == (C, L) and torch.isfinite(got).all()
    assert _same_bits(got, want)
    assert not torch.equal(got, base)
    assert _same_bits(crossed.enhance_lr(x, noise=noise), want)                  # again: replays, the same table
    return crossed


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("overlap", [0.0, 0.25])
def test_option_is_the_kernel_behind_the_plain_pipeline(graph, overlap):
    model, opt = _tiny("mdct2")
    L = 4 * opt.segment_length + 100                               # two full groups and a partial one at overlap 0
    for C in (1, 2):
        sr = _composes(model, opt, C, L, 31 + C, overlap=overlap, graph=graph)
        if graph:
            assert sr._g is not None and sr._g['graph'] is not None
        assert sr.reference_amplitude == (overlap == 0.0)


@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_option_composes_with_lowband_and_either_amplitude(mdct_type):
    """level follows gain / 2: reference_amplitude halves the gain (mdct2), and the crossover sees the same ratio to its input."""
    model, opt = _tiny(mdct_type)
    L = 2 * opt.segment_length + 50
    gains = set()
    for ra in (True, False):
        sr = _composes(model, opt, 2, L, 41, overlap=0.25, lowband='input', lowband_fade=2, reference_amplitude=ra)
        gains.add(sr.gain)
    assert len(gains) == (2 if mdct_type == "mdct2" else 1)
    sr = _composes(model, opt, 1, L, 42, overlap=0.25, crossover_hz=3000.0, crossover_taps=255)
    assert sr.crossover_plan == (255, 3000.0 / 48000, 8.96) and sr._xover_taps.numel() == 255


# ------------------------------------------------------------------------------------------
# level
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,mdct_type", [(2, "mdct2"), (4, "mdct2"), (4, "mdct4")])
def test_pass_through_generator_pins_the_level(up, mdct_type):
    """A generator that returns its input's spectrogram: the pipeline returns (gain / 2) * x up to the transform round trip, and
    the crossover -- which mixes in (gain / 2) * x -- stays within twice that distance.  Any other level factor would add
    |factor - gain / 2| * |x|, orders of magnitude more."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, base_opt = _tiny(mdct_type)                             # (reference_amplitude changes the gain with mdct2 only)
    opt = SimpleNamespace(**dict(vars(base_opt), lr_sampling_rate=base_opt.hr_sampling_rate // up))
    stub = PassThrough(model)
    L = 4 * opt.segment_length + 100
    x = _rows(2, L)
    for ra in (None, True):
        off = SuperResolver(stub, opt, overlap=0.25, reference_amplitude=ra)
        on = SuperResolver(stub, opt, overlap=0.25, reference_amplitude=ra, crossover='input')
        target = (off.gain / 2.0) * x.double()
        d_off = float((off.enhance_lr(x).double() - target).abs().max())
        d_on = float((on.enhance_lr(x).double() - target).abs().max())
        scale = float(target.abs().max())
        print(f"up {up} {mdct_type} gain {off.gain:.4f}: |sr - (gain/2) x| max {d_off:.3e} without, {d_on:.3e} with the crossover; |(gain/2) x| max {scale:.3e}")
        assert d_off < 1e-3 * scale                                # the premise: the stub passes the input through
        assert d_on <= 2.0 * d_off


# ------------------------------------------------------------------------------------------
# launches
# ------------------------------------------------------------------------------------------
def test_one_launch_per_clip_and_nothing_else_changes():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    model, opt = _tiny("mdct2")
    L = 4 * opt.segment_length + 100
    x = _rows(2, L)
    lib = _lib.lib()
    counts = {}
    for name, kw in (("off", {}), ("on", dict(crossover='input'))):
        sr = SuperResolver(model, opt, overlap=0.25, graph=False, **kw)
        noise = _noise(sr, 2 * segment_plan(L, opt.segment_length, 0.25)[0], 5)
        sr.enhance_lr(x, noise=noise)                              # tables and packed weights exist
        lib.p2phd_launch_count(None, 1)
        sr.enhance_lr(x, noise=noise)
        sr.enhance_lr(x[:1], noise=noise)
        torch.cuda.synchronize()
        counts[name] = {f: lib.p2phd_launch_count(f.encode(), 0) for f in FAMILIES + ("xover",)}
    assert counts["off"]["xover"] == 0 and counts["on"]["xover"] == 2           # one per clip, whatever C is
    assert counts["off"]["stitch"] == 4 and sum(counts["off"][f] for f in FAMILIES) > 4       # (gather + stitch per clip; the conv stack ran)
    for f in FAMILIES:
        assert counts["on"][f] == counts["off"][f], f


def test_equal_rates_are_refused():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, base_opt = _tiny("mdct4")
    opt = SimpleNamespace(**dict(vars(base_opt), lr_sampling_rate=base_opt.hr_sampling_rate))
    SuperResolver(model, opt)                                      # fine without the option
    with pytest.raises(ValueError, match=r"nothing to cross over"):
        SuperResolver(model, opt, crossover='input')
    with pytest.raises(ValueError, match=r"crossover must be None or 'input'"):
        SuperResolver(model, base_opt, crossover='model')
    with pytest.raises(ValueError, match=r"options of crossover='input'"):
        SuperResolver(model, base_opt, crossover_taps=255)


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def test_cli_folder(tmp_path, capsys):
    """--crossover input --crossover_taps 255 on a folder of two files writes the payloads of enhance_file on an equally
    configured object; without the flag, those of SuperResolver() as it was.  (lr_sampling_rate 24000: 255 taps at 48 kHz have a
    1080 Hz transition band, which fits under 12 kHz from the default 11.4 kHz.)"""
    from pix2pixhdaudiosr_amd import generate as G
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.models.models import create_model
    d_in, d_on, d_off = tmp_path / "in", tmp_path / "on", tmp_path / "off"
    d_in.mkdir()
    wavio.save(str(d_in / "a.wav"), _clip(6000), 48000)
    wavio.save(str(d_in / "b.wav"), torch.stack([_clip(3500, 500), -_clip(3500, 900)]), 48000)
    common = dict(mdct_type="mdct4", checkpoints_dir=str(tmp_path), name="run", seed=1234, lr_sampling_rate=24000)
    torch.manual_seed(1234)
    create_model(_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:                       # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    base = ["--input", str(d_in), "--load_pretrain", str(folder), "--channels", "all"]
    assert G.main(base + ["--output", str(d_on), "--crossover", "input", "--crossover_taps", "255"]) == 0
    text_on = capsys.readouterr().out
    assert "crossover: the input below 11400 Hz (255 taps)" in text_on and "2 of 2 files enhanced" in text_on
    assert G.main(base + ["--output", str(d_off)]) == 0
    text_off = capsys.readouterr().out
    assert "crossover" not in text_off and "2 of 2 files enhanced" in text_off
    # the objects main builds
    opt = G.opt_from_file(str(folder / "opt.txt"), checkpoints_dir=str(tmp_path), name="run", load_pretrain='', continue_train=False)
    model = create_model(opt)
    model.eval()
    for d_cli, kw in ((d_on, dict(crossover='input', crossover_taps=255)), (d_off, {})):
        sr = G.SuperResolver(model, opt, overlap=0.25, **kw)
        for name in ("a.wav", "b.wav"):
            torch.manual_seed(1234)                                # every file of a folder starts from the seed
            mine = str(tmp_path / ("mine_" + name))
            sr.enhance_file(str(d_in / name), mine, channels='all')
            got, meta = wavio.read_payload(str(d_cli / name))
            want, meta2 = wavio.read_payload(mine)
            assert (meta.num_frames, meta.num_channels, meta.sample_rate) == (meta2.num_frames, meta2.num_channels, 48000)
            assert bytes(got) == bytes(want), (d_cli.name, name)
    a_on, _ = wavio.read_payload(str(d_on / "a.wav"))
    a_off, _ = wavio.read_payload(str(d_off / "a.wav"))
    assert bytes(a_on) != bytes(a_off)
    # a plan that cannot be met is an argument error, before the model is built
    with pytest.raises(SystemExit):
        G.main(base + ["--output", str(d_on), "--crossover", "input", "--crossover_taps", "31"])
    assert "transition band" in capsys.readouterr().err
