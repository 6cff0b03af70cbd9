"""The low-band splice on the GPU (csrc/spectro.hip: p2phd_spectro_decode_spliced; util.imdct(lr_spectro=...);
SuperResolver(lowband='input'); --lowband): pure rows against the existing decode bit for bit, fade rows against a float64
restatement, identity, canaries and argument checks, util.imdct, the pipeline (default = 'model', graph = eager, a
pass-through generator, the lsd_lf ordering) and the command line."""
import csv
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 2
SHAPES = [(F, M, C) for F in (9, 40) for M in (64, 80) for C in (1, 2)]      # F: a partial tile / a full and a partial one
SCALES = (1.0, 0.5)
MIN_VALUE = 1e-7
GUARD = 1024                                                       # floats on either side of the output
GUARD_BITS = 0x7FC0BEEF                                            # a NaN pattern no kernel writes


def _keeps(M):
    return (0, 21, 32, M)


def _fades(keep):
    return sorted({f for f in (0, 1, 5, keep) if f <= keep})


_OPERANDS = {}


def _operands(F, M, C):
    """(sr, lr, pha, minmax) on the GPU: values in [0, 1] with exact 0 and 1 entries, +-1 signs, (min, max) = (-70, 20)."""
    key = (F, M, C)
    if key not in _OPERANDS:
        rng = np.random.default_rng(1000 * F + 10 * M + C)
        def plane():
            x = rng.random((B, C, M, F)).astype(np.float32)
            r = rng.random(x.shape)
            x[r < 0.05] = 0.0
            x[r > 0.95] = 1.0
            return x
        sr, lr = plane(), plane()
        if C == 2:                                                 # equal channels at and above some keep: sign(a0 - a1) = 0
            sr[:, 1, 40:44] = sr[:, 0, 40:44]
        pha = (2.0 * rng.integers(0, 2, (B, M, F)) - 1.0).astype(np.float32)
        mm = np.array([-70.0, 20.0], dtype=np.float32)
        _OPERANDS[key] = tuple(torch.from_numpy(a).to(DEV) for a in (sr, lr, pha, mm))
    return _OPERANDS[key]


_SIGNED = {}


def _signed(which, F, M, C, keep, scale):
    """p2phd_spectro_decode_signed of operand `which` (0 sr, 1 lr) as a numpy array [B, F, M]; computed once per case."""
    from pix2pixhdaudiosr_amd import _lib
    key = (which, F, M, C, keep, scale)
    if key not in _SIGNED:
        ops = _operands(F, M, C)
        spec = torch.empty((B, F, M), dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().p2phd_spectro_decode_signed(_lib.ptr(ops[which]), _lib.ptr(ops[2]), _lib.ptr(ops[3]), B, F, M, C, keep,
                                                          MIN_VALUE, scale, _lib.ptr(spec), _lib.stream_ptr()), "decode_signed")
        _SIGNED[key] = spec.cpu().numpy()
    return _SIGNED[key]


def _spliced_rc(sr, lr, pha, mm, nb, F, M, C, keep, fade, scale):
    """Runs the entry point on an output that lies between two guard regions -> (return code, output [nb, F, M], guards intact)."""
    from pix2pixhdaudiosr_amd import _lib
    n = nb * F * M
    buf = torch.full((GUARD + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    out = buf[GUARD:GUARD + n]
    rc = _lib.lib().p2phd_spectro_decode_spliced(_lib.ptr(sr), _lib.ptr(lr), _lib.ptr(pha), _lib.ptr(mm), nb, F, M, C, keep, fade,
                                                 MIN_VALUE, scale, _lib.ptr(out), _lib.stream_ptr())
    bits = buf.view(torch.int32).cpu().numpy()
    intact = bool((bits[:GUARD] == GUARD_BITS).all() and (bits[GUARD + n:] == GUARD_BITS).all())
    return rc, bits[GUARD:GUARD + n].view(np.float32).reshape(nb, F, M), intact


def _spliced(F, M, C, keep, fade, scale, same=False):
    sr, lr, pha, mm = _operands(F, M, C)
    rc, out, intact = _spliced_rc(sr, sr if same else lr, pha, mm, B, F, M, C, keep, fade, scale)
    assert rc == 0 and intact, (rc, intact)
    assert not (out.view(np.int32) == GUARD_BITS).any()            # every element was written
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------
# 1. pure regions
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,M,C", SHAPES)
def test_pure_regions_are_bit_identical_to_decode_signed(F, M, C):
    for scale in SCALES:
        for keep in _keeps(M):
            s, l = _signed(0, F, M, C, keep, scale), _signed(1, F, M, C, keep, scale)
            for fade in _fades(keep):
                got = _spliced(F, M, C, keep, fade, scale)
                lo = keep - fade
                assert np.array_equal(_bits(got[..., :lo]), _bits(l[..., :lo])), (keep, fade, scale)
                assert np.array_equal(_bits(got[..., keep:]), _bits(s[..., keep:])), (keep, fade, scale)


# ------------------------------------------------------------------------------------------
# 2. fade rows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,M,C", SHAPES)
def test_fade_rows_match_the_float64_restatement(F, M, C):
    """s + w (l - s) in float64 from the fp32 s and l of the existing kernel and w = cos^2(pi (j + 1/2) / (2 fade)) in float64;
    per element 8 * 2^-24 * max(|s|, |l|): the fp32 weight (a few ulp) and three rounded operations."""
    worst = 0.0
    for scale in SCALES:
        for keep in _keeps(M):
            s, l = _signed(0, F, M, C, keep, scale).astype(np.float64), _signed(1, F, M, C, keep, scale).astype(np.float64)
            for fade in _fades(keep):
                if fade == 0:
                    continue
                got = _spliced(F, M, C, keep, fade, scale).astype(np.float64)
                lo = keep - fade
                w = np.cos(np.pi * (np.arange(fade) + 0.5) / (2 * fade)) ** 2
                assert ((0 < w) & (w < 1)).all() and (np.diff(w) < 0).all()   # the input's weight falls towards keep
                assert abs(w[0] + w[-1] - 1) < 1e-15
                sf, lf = s[..., lo:keep], l[..., lo:keep]
                want = sf + w * (lf - sf)
                tol = 8 * 2.0 ** -24 * np.maximum(np.abs(sf), np.abs(lf))
                err = np.abs(got[..., lo:keep] - want)
                rel = float((err / np.maximum(tol, 1e-300)).max())
                worst = max(worst, rel)
                assert (err <= tol).all(), (keep, fade, scale, rel)
    print(f"fade rows F={F} M={M} C={C}: worst error {worst:.3f} of the tolerance")


# ------------------------------------------------------------------------------------------
# 3. identity
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,M,C", SHAPES)
def test_equal_operands_give_decode_signed(F, M, C):
    for scale in SCALES:
        for keep in _keeps(M):
            s = _signed(0, F, M, C, keep, scale)
            for fade in _fades(keep):
                assert np.array_equal(_bits(_spliced(F, M, C, keep, fade, scale, same=True)), _bits(s)), (keep, fade, scale)


# ------------------------------------------------------------------------------------------
# 4. canaries and argument checks (the guard regions are checked in every call above as well)
# ------------------------------------------------------------------------------------------
def test_empty_batch_and_bad_arguments():
    from pix2pixhdaudiosr_amd import _lib
    F, M, C = 9, 80, 2
    sr, lr, pha, mm = _operands(F, M, C)
    L = _lib.lib()
    rc, out, intact = _spliced_rc(sr, lr, pha, mm, 0, F, M, C, 21, 5, 1.0)
    assert rc == 0 and intact and out.size == 0
    # B = 0 writes nothing: the same call aimed at a guarded buffer of one batch leaves all of it alone
    n = F * M
    buf = torch.full((n,), GUARD_BITS, dtype=torch.int32, device=DEV)
    assert L.p2phd_spectro_decode_spliced(_lib.ptr(sr), _lib.ptr(lr), _lib.ptr(pha), _lib.ptr(mm), 0, F, M, C, 21, 5, MIN_VALUE, 1.0,
                                          _lib.ptr(buf), _lib.stream_ptr()) == 0
    assert bool((buf == GUARD_BITS).all())
    einval = None
    for keep, fade, word in ((21, -1, "fade_rows"), (21, 22, "fade_rows"), (0, 1, "fade_rows"), (M + 1, 0, "keep_rows"), (-1, 0, "keep_rows")):
        rc, out, intact = _spliced_rc(sr, lr, pha, mm, B, F, M, C, keep, fade, 1.0)
        text = L.p2phd_last_error().decode()
        assert rc != 0 and intact and word in text and "spectro_decode_spliced" in text, (keep, fade, rc, text)
        assert (_bits(out) == GUARD_BITS).all()                    # refused before anything ran
        einval = rc if einval is None else einval
        assert rc == einval
    # P2PHD_EINVAL: the code the neighbouring entry point gives for its own bad keep_rows
    spec = torch.empty((B, F, M), dtype=torch.float32, device=DEV)
    assert L.p2phd_spectro_decode_signed(_lib.ptr(sr), _lib.ptr(pha), _lib.ptr(mm), B, F, M, C, M + 1, MIN_VALUE, 1.0, _lib.ptr(spec),
                                         _lib.stream_ptr()) == einval
    rc, _, intact = _spliced_rc(sr, lr, pha, mm, B, F, M, 3, 21, 5, 1.0)
    assert rc == einval and intact and "channels" in L.p2phd_last_error().decode()
    assert L.p2phd_spectro_decode_spliced(_lib.ptr(sr), None, _lib.ptr(pha), _lib.ptr(mm), B, F, M, C, 21, 5, MIN_VALUE, 1.0,
                                          _lib.ptr(spec), _lib.stream_ptr()) == einval
    assert "null pointer" in L.p2phd_last_error().decode()
    with pytest.raises(_lib.P2PHDError, match=r"fade_rows"):
        _lib.check(L.p2phd_spectro_decode_spliced(_lib.ptr(sr), _lib.ptr(lr), _lib.ptr(pha), _lib.ptr(mm), B, F, M, C, 21, 22, MIN_VALUE,
                                                  1.0, _lib.ptr(spec), _lib.stream_ptr()), "spectro_decode_spliced")


# ------------------------------------------------------------------------------------------
# 5. util.imdct
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,up,fade", [(2, 3, 0), (2, 3, 5), (2, 2, 32), (2, 1, 7), (1, 3, 5), (1, 1, 0)])
def test_util_imdct_splices(C, up, fade):
    """_imdct = 2 * s makes util.imdct return the decoded spec itself (2 s / 2 is exact)."""
    from pix2pixhdaudiosr_amd.util import util as U
    F, M = 40, 64
    sr, lr, pha, mm = _operands(F, M, C)
    norm = {'min': mm[0], 'max': mm[1]}
    keep = int(M * (1 / up)) if up > 1 else M
    kw = dict(pha=pha, norm_param=norm, _imdct=lambda s: 2 * s, up_ratio=up, explicit_encoding=C == 2)
    torch.manual_seed(3)                                           # the random signs of the single-channel encoding (rows >= keep)
    plain = U.imdct(spectro=sr, **kw)
    torch.manual_seed(3)
    got = U.imdct(spectro=sr, lr_spectro=lr, lowband_fade=fade, **kw)
    assert tuple(got.shape) == (B, F, M) and got.dtype == torch.float32
    plain, got = plain.cpu().numpy(), got.cpu().numpy()
    if C == 2 or up == 1:
        # without lr_spectro: today's launch -- the existing entry point with keep_rows = keep and scale 1
        assert np.array_equal(_bits(plain), _bits(_signed(0, F, M, C, keep, 1.0)))
        assert np.array_equal(_bits(got), _bits(_spliced(F, M, C, keep, fade, 1.0)))
        low = _signed(1, F, M, C, keep, 1.0)
    else:
        # single channel, up_ratio > 1: rows >= keep carry the drawn signs, the same in both calls; rows < keep carry pha
        assert np.array_equal(_bits(np.abs(plain)), _bits(np.abs(_signed(0, F, M, C, keep, 1.0))))
        assert np.array_equal(_bits(plain[..., :keep]), _bits(_signed(0, F, M, C, keep, 1.0)[..., :keep]))
        assert (plain[..., keep:] < 0).any() and (plain[..., keep:] > 0).any()
        low = _signed(1, F, M, C, keep, 1.0)
    assert np.array_equal(_bits(got[..., :keep - fade]), _bits(low[..., :keep - fade]))       # case 1 again, through util.imdct
    assert np.array_equal(_bits(got[..., keep:]), _bits(plain[..., keep:]))
    if fade < keep:
        assert not np.array_equal(got[..., :keep - fade], plain[..., :keep - fade])


def test_util_imdct_validates():
    from pix2pixhdaudiosr_amd.util import util as U
    F, M, C = 40, 64, 2
    sr, lr, pha, mm = _operands(F, M, C)
    kw = dict(spectro=sr, pha=pha, norm_param={'min': mm[0], 'max': mm[1]}, _imdct=lambda s: 2 * s, up_ratio=3, explicit_encoding=True)
    with pytest.raises(ValueError, match=r"lr_spectro shape"):
        U.imdct(lr_spectro=lr[:, :, :-1], **kw)
    with pytest.raises(ValueError, match=r"lr_spectro shape"):
        U.imdct(lr_spectro=_operands(F, M, 1)[1], **kw)
    for bad in (-1, 22, 1.5):
        with pytest.raises(ValueError, match=r"lowband_fade"):
            U.imdct(lr_spectro=lr, lowband_fade=bad, **kw)
    U.imdct(lr_spectro=lr, lowband_fade=21, **kw)
    U.imdct(lowband_fade=99, **kw)                                 # without lr_spectro the fade is not looked at: today's path


# ------------------------------------------------------------------------------------------
# 6. the pipeline
# ------------------------------------------------------------------------------------------
def _opt(**kw):
    """The tiny model of the generate tests with a LocalEnhancer generator."""
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


def _noise(sr, S, seed):
    shape = sr.noise_shape(1)
    return torch.randn((S,) + shape[1:], generator=torch.Generator().manual_seed(seed)).to(DEV)


class PassThrough:
    """`inference` returns the encoding of its own input, as generator output and as input spectrogram."""

    def __init__(self, real):
        self.real, self.mdct_type, self.device = real, real.mdct_type, real.device

    def inference(self, lr_audio, inst, noise=None):
        spectro, pha, norm = self.real.to_spectro(lr_audio, mask=False)
        return spectro, pha, norm, spectro


@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_pipeline_default_graph_and_pass_through(mdct_type):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    T = opt.segment_length
    L = 4 * T + 100                                               # 5 segments: two full groups and a partial one
    lr = (0.5 * _clip(L)).to(DEV)[None]
    keep = int((opt.n_fft if mdct_type == 'mdct2' else opt.n_fft // 2) / 6)
    assert keep >= 4
    plain = SuperResolver(model, opt, overlap=0, graph=False)
    noise = _noise(plain, 5, 21)
    want = plain.enhance_lr(lr, noise=noise)
    # 'model' is the SuperResolver of today
    named = SuperResolver(model, opt, overlap=0, graph=False, lowband='model', lowband_fade=4)
    assert torch.equal(named.enhance_lr(lr, noise=noise), want)
    # 'input': graph replay = eager, and not what 'model' gives
    for fade in (0, 4):
        eager = SuperResolver(model, opt, overlap=0, graph=False, lowband='input', lowband_fade=fade)
        graphed = SuperResolver(model, opt, overlap=0, graph=True, lowband='input', lowband_fade=fade)
        got = eager.enhance_lr(lr, noise=noise)
        assert tuple(got.shape) == (1, L) and torch.isfinite(got).all() and not torch.equal(got, want)
        assert torch.equal(graphed.enhance_lr(lr, noise=noise), got)
        assert graphed._g is not None and graphed._g['graph'] is not None
        assert torch.equal(graphed.enhance_lr(lr, noise=noise), got)          # replays only
    # a generator that returns the input's encoding: both low bands are the same rows
    stub = PassThrough(model)
    through = SuperResolver(stub, opt, overlap=0.25, lowband='model').enhance_lr(lr)
    assert torch.isfinite(through).all() and through.abs().max() > 0
    for fade in (0, 4):
        assert torch.equal(SuperResolver(stub, opt, overlap=0.25, lowband='input', lowband_fade=fade).enhance_lr(lr), through)
    with pytest.raises(ValueError, match=r"lowband_fade"):
        SuperResolver(model, opt, lowband='input', lowband_fade=keep + 1)
    with pytest.raises(ValueError, match=r"lowband must be"):
        SuperResolver(model, opt, lowband='lr')


@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_input_low_band_lowers_lsd_lf(mdct_type):
    """Random weights, a band-limited input made with lr_round_trip, metrics against the full-band original: the run that keeps
    the input's low band has the smaller low-band log-spectral distance.  An ordering only."""
    from pix2pixhdaudiosr_amd.data.audio_dataset import lr_round_trip
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    from pix2pixhdaudiosr_amd.util import util as U
    model, opt = _tiny(mdct_type)
    L = 4 * opt.segment_length + 100
    hr = _clip(L, 3000).to(DEV)[None]
    lr = lr_round_trip(hr, opt.hr_sampling_rate, opt.lr_sampling_rate, opt.hr_sampling_rate)[..., :L]
    figures = {}
    for lowband in ('model', 'input'):
        sr = SuperResolver(model, opt, overlap=0.25, lowband=lowband)
        S = segment_plan(L, opt.segment_length, 0.25)[0]
        y = sr.enhance_lr(lr, noise=_noise(sr, S, 22))
        figures[lowband] = U.compute_matrics_ext(hr, lr, y, opt)[0]
    print(f"{mdct_type}: lsd_lf model {figures['model']['lsd_lf']:.4f} input {figures['input']['lsd_lf']:.4f}; "
          f"lsd_hf model {figures['model']['lsd_hf']:.4f} input {figures['input']['lsd_hf']:.4f}")
    assert np.isfinite(figures['model']['lsd_lf']) and np.isfinite(figures['input']['lsd_lf'])
    assert figures['input']['lsd_lf'] < figures['model']['lsd_lf']


# ------------------------------------------------------------------------------------------
# 7. the command line
# ------------------------------------------------------------------------------------------
def test_cli_round_trip(tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.models.models import create_model
    clip = str(tmp_path / "clip.wav")
    wavio.save(clip, _clip(6000), 48000)
    common = dict(mdct_type="mdct4", checkpoints_dir=str(tmp_path), name="run", seed=1234)
    torch.manual_seed(1234)
    create_model(_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:                      # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    out, table = str(tmp_path / "sr.wav"), str(tmp_path / "m.csv")
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.generate", "--input", clip, "--output", out, "--load_pretrain",
                        str(folder), "--lowband", "input", "--lowband_fade", "2", "--metrics_csv", table, "--metrics_ext"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    line = [l for l in p.stdout.splitlines() if l.startswith("amplitude:")]
    assert len(line) == 1 and "low band: the input's (fade over 2 rows)" in line[0], p.stdout
    assert "LSD_LF:" in p.stdout
    meta = wavio.info(out)
    assert (meta.sample_rate, meta.num_frames, meta.num_channels) == (48000, 6000, 1)
    with open(table, newline="") as f:
        rows = list(csv.reader(f))
    assert "lsd_lf" in rows[0] and len(rows) == 3 and rows[-1][0] == "mean"
    assert np.isfinite(float(rows[1][rows[0].index("lsd_lf")]))
