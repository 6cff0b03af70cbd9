"""Whole-file generation on the GPU (pix2pixhdaudiosr_amd/generate.py, csrc/stitch.hip): the two kernels against the numpy
restatement (tests/_generate_ref.py), the pipeline against the hand-composed loop of test_gpu_evaltail.py and against the
reference's own chain (tests/golden/generate.npz), graph replay against eager, a pass-through generator that pins offsets,
weights, trimming and gain, launch accounting, and the file / command-line round trip."""
import os
import subprocess
import sys
from math import sqrt

import numpy as np
import pytest
import torch

import _generate_ref as R
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ulp_err(got, want64):
    """max |got - fp32(want)| in units of the spacing of fp32(want)."""
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())


# ------------------------------------------------------------------------------------------
# 1. kernels
# ------------------------------------------------------------------------------------------
# (S, T, V, samples short of the full span)
SHAPES = [(1, 64, 0, 0), (1, 37, 0, 5), (3, 64, 0, 0), (4, 64, 32, 0), (5, 37, 18, 11), (3, 50, 7, 3), (6, 992, 248, 500),
          (2, 4064, 1, 0), (4, 33, 16, 0)]


@pytest.mark.parametrize("S,T,V,short", SHAPES)
def test_gather_and_stitch_match_restatement(S, T, V, short):
    from pix2pixhdaudiosr_amd.generate import segments_gather, segments_stitch
    stride = T - V
    span = (S - 1) * stride + T
    L = span - short
    rng = np.random.default_rng(S * 1000 + T + V)
    x = rng.standard_normal(L).astype(np.float32)
    seg = segments_gather(torch.from_numpy(x).to(DEV), T, stride, S)
    want = R.gather(x, T, stride, S)
    assert seg.dtype == torch.float32 and tuple(seg.shape) == (S, T)
    assert np.array_equal(seg.cpu().numpy().view(np.uint32), want.view(np.uint32))              # bit-equal
    # independent segments (neighbours disagree inside the overlaps) and a gain that is not a power of two
    y = rng.standard_normal((S, T)).astype(np.float32)
    gain = float(np.float32(sqrt(5.0)))
    for L_out in sorted({span, L, max(L - 1, 0)}):
        got = segments_stitch(torch.from_numpy(y).to(DEV), stride, gain, L_out).cpu().numpy()
        assert got.shape == (L_out,)
        if L_out:
            err = _ulp_err(got, R.stitch(y, stride, gain, L_out))
            assert err <= 2.0, (L_out, err)
    # what was gathered from a waveform comes back
    back = segments_stitch(seg, stride, 1.0, L).cpu().numpy()
    err = _ulp_err(back, x.astype(np.float64))
    print(f"stitch(gather(x)) S={S} T={T} V={V}: {err:.2f} ulp")
    assert err <= 2.0, err


def test_gather_views_and_unaligned_source():
    """A source that is not 16-byte aligned takes the element path; the result is the same."""
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import segments_gather
    x = torch.randn(4 * 64 + 1, device=DEV)
    a = x[1:]                                                     # storage offset of one float
    with pytest.raises(_lib.P2PHDError):
        segments_gather(a[::2], 64, 64, 2)                        # strided view: refused, not copied silently
    assert a.data_ptr() % 16 != 0
    got = segments_gather(a.contiguous(), 64, 48, 5)
    assert np.array_equal(got.cpu().numpy(), R.gather(a.cpu().numpy(), 64, 48, 5))


def test_precondition_errors():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import segments_gather, segments_stitch
    seg = torch.zeros(3, 64, device=DEV)
    with pytest.raises(_lib.P2PHDError, match=r"overlap"):
        segments_stitch(seg, 31)                                  # V = 33 > T / 2
    with pytest.raises(_lib.P2PHDError, match=r"overlap"):
        segments_stitch(seg, 65)                                  # V < 0
    with pytest.raises(_lib.P2PHDError, match=r"L_out"):
        segments_stitch(seg, 48, 1.0, 2 * 48 + 64 + 1)            # one sample beyond the span
    with pytest.raises(_lib.P2PHDError, match=r"S >= 1"):
        segments_stitch(torch.zeros(0, 64, device=DEV), 48)
    with pytest.raises(_lib.P2PHDError, match=r"stride"):
        segments_gather(torch.zeros(100, device=DEV), 64, 0, 2)
    with pytest.raises(_lib.P2PHDError, match=r"S >= 1"):
        segments_gather(torch.zeros(100, device=DEV), 64, 64, 0)
    with pytest.raises(_lib.P2PHDError):
        segments_stitch(torch.zeros(3, 64), 48)                   # a host tensor: no CPU path
    assert segments_stitch(seg, 48, 1.0, 0).numel() == 0


# ------------------------------------------------------------------------------------------
# the hand-composed chain (test_gpu_evaltail.py::test_generation_flow_end_to_end) as a function
# ------------------------------------------------------------------------------------------
def _inverse(opt, mdct_type):
    from pix2pixhdaudiosr_amd.dct.dct import IDCT
    from pix2pixhdaudiosr_amd.models.mdct import IMDCT2, IMDCT4
    from pix2pixhdaudiosr_amd.util import util as U
    kw = dict(window=U.kbdwin, win_length=opt.win_length, hop_length=opt.hop_length, n_fft=opt.n_fft, center=opt.center,
              out_length=opt.segment_length, device='cuda')
    return IMDCT2(idct_op=IDCT(), **kw) if mdct_type == 'mdct2' else IMDCT4(**kw)


def hand_loop(model, opt, lr_audio, noise):
    """AudioTestDataset.seg_pad_audio -> model.inference per batch -> util.imdct per batch -> cat -> sqrt(up_ratio - 1)."""
    from pix2pixhdaudiosr_amd.data.audio_dataset import AudioTestDataset
    from pix2pixhdaudiosr_amd.util import util as U
    ds = AudioTestDataset.__new__(AudioTestDataset)
    ds.segment_length = opt.segment_length
    seg = ds.seg_pad_audio(lr_audio)
    _imdct = _inverse(opt, model.mdct_type)
    up_ratio = opt.hr_sampling_rate / opt.lr_sampling_rate
    audio = []
    with torch.no_grad():
        for s0 in range(0, seg.shape[0], opt.batchSize):
            label = seg[s0:s0 + opt.batchSize]
            sr_spectro, lr_pha, norm_param, _ = model.inference(label, None, noise=None if noise is None else noise[s0:s0 + opt.batchSize])
            audio.append(U.imdct(spectro=sr_spectro.abs(), pha=lr_pha.squeeze(1), norm_param=norm_param, _imdct=_imdct,
                                 up_ratio=up_ratio, explicit_encoding=True))
    return sqrt(up_ratio - 1) * torch.cat(audio, dim=0).view(1, -1)


def _clip(n, start=0):
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    return torch.from_numpy(F["test_wav_excerpt_i16"][start:start + n].astype(np.float32) / 32768.0)


def _tiny(mdct_type, seed=1234, **kw):
    from test_gpu_model import make_opt
    from pix2pixhdaudiosr_amd.models.models import create_model
    opt = make_opt(mdct_type=mdct_type, segment_length=31 * 32, batchSize=2, **kw)
    torch.manual_seed(seed)
    model = create_model(opt)
    model.eval()
    return model, opt


def _noise(sr, S, seed):
    shape = sr.noise_shape(1)
    assert sr.noise_shape(2)[1:] == shape[1:]
    return torch.randn((S,) + shape[1:], generator=torch.Generator().manual_seed(seed)).to(DEV)


# ------------------------------------------------------------------------------------------
# 2. overlap = 0 is the existing chain, bit for bit
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_no_overlap_is_bit_identical_to_hand_loop(mdct_type):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    T = opt.segment_length
    L = 4 * T + 100                                               # 5 segments: groups of 2, 2 and a partial one
    lr = (0.5 * _clip(L)).to(DEV)[None]
    sr = SuperResolver(model, opt, overlap=0, graph=False)
    noise = _noise(sr, 5, 11)
    want = hand_loop(model, opt, lr, noise)
    assert want.shape[-1] == 5 * T
    if mdct_type == 'mdct4':
        want = 2 * want                                           # the factor the hand-composed chain leaves with IMDCT4
    got = sr.enhance_lr(lr, noise=noise)
    assert tuple(got.shape) == (1, L) and torch.isfinite(got).all() and got.abs().max() > 0
    assert torch.equal(got, want[:, :L])
    assert torch.equal(sr.enhance_lr(lr[0], noise=noise), got)    # [L] input


# ------------------------------------------------------------------------------------------
# 3. graph replay = eager
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 0.25])
def test_graphed_is_bit_identical_to_eager(overlap):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    model, opt = _tiny("mdct2")
    _, stride, V = segment_plan(1, opt.segment_length, overlap)
    L = 4 * stride + V + 100
    lr = (0.5 * _clip(L, 3000)).to(DEV)[None]
    S = segment_plan(L, opt.segment_length, overlap)[0]
    assert S % 2 == 1 and S >= 5                                  # full groups through the graph and a partial eager one
    eager = SuperResolver(model, opt, overlap=overlap, graph=False)
    graphed = SuperResolver(model, opt, overlap=overlap, graph=True)
    noise = _noise(eager, S, 12)
    want = eager.enhance_lr(lr, noise=noise)
    assert torch.equal(graphed.enhance_lr(lr, noise=noise), want)
    assert graphed._g is not None and graphed._g['graph'] is not None
    assert torch.equal(graphed.enhance_lr(lr, noise=noise), want)            # replays only
    # without injected noise both draw one torch.randn per group: the same seed gives the same clip
    torch.manual_seed(5)
    a = eager.enhance_lr(lr)
    torch.manual_seed(5)
    assert torch.equal(graphed.enhance_lr(lr), a)


# ------------------------------------------------------------------------------------------
# 4. the reference's own chain
# ------------------------------------------------------------------------------------------
# max |hand_loop - reference| / max |reference| of the hand-composed loop (model.inference, util.imdct and seg_pad_audio as
# they were before this pipeline existed) on this fixture, measured on an MI355X with the fp32 model and the fixture's noise
# replayed: 4.09e-6 of the peak (4.80e-8 absolute, peak 1.17e-2; per segment 1.2e-6 .. 4.1e-6; the same on a second run).
# The pipeline is bit-identical to that loop, so it is held to twice the figure: the margin is for another box summing
# the convs in another order.
PARENT_LOOP_ERR = 4.1e-6
REF_TOL = 2 * PARENT_LOOP_ERR


def _fixture_model():
    g = np.load(os.path.join(GOLDEN, "generate.npz"))
    model, opt = _tiny("mdct2", netG="local")
    sd = {k: torch.from_numpy(g[f"G_p_{k}"]) for k in model.netG.state_dict().keys()}
    model.netG.load_state_dict(sd)
    from pix2pixhdaudiosr_amd import _ops
    _ops.bump_weight_epoch()
    n_fft, hop, seg, batch, hr, lr = (int(v) for v in g["meta"])
    assert (opt.n_fft, opt.hop_length, opt.segment_length, opt.batchSize, opt.hr_sampling_rate, opt.lr_sampling_rate) == (n_fft, hop, seg, batch, hr, lr)
    return g, model, opt


def test_reference_fixture():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    g, model, opt = _fixture_model()
    lr = torch.from_numpy(g["lr_audio"]).to(DEV)
    noise = torch.from_numpy(g["noise"]).to(DEV)
    ref = g["audio"]
    L = lr.shape[-1]
    peak = np.abs(ref).max()
    hand = hand_loop(model, opt, lr, noise)
    assert tuple(hand.shape) == ref.shape
    hand_err = np.abs(hand.cpu().numpy() - ref).max() / peak
    for graph in (False, True):
        got = SuperResolver(model, opt, overlap=0, graph=graph).enhance_lr(lr, noise=noise)
        assert torch.equal(got, hand[:, :L])
        err = np.abs(got.cpu().numpy() - ref[:, :L]).max() / peak
        print(f"reference fixture: hand-composed loop {hand_err:.3e}, pipeline (graph={graph}) {err:.3e} of the peak")
        assert hand_err <= 1e-2                                   # more would be a grouping / noise-replay defect
        assert err <= REF_TOL, (err, REF_TOL)


# ------------------------------------------------------------------------------------------
# 5. pass-through generator: offsets, weights, trimming, gain
# ------------------------------------------------------------------------------------------
class PassThrough:
    """`inference` returns the encoding of its own input: what comes back must be the input."""

    def __init__(self, real):
        self.real, self.mdct_type, self.device = real, real.mdct_type, real.device

    def inference(self, lr_audio, inst, noise=None):
        spectro, pha, norm = self.real.to_spectro(lr_audio, mask=False)
        return spectro, pha, norm, spectro


@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
@pytest.mark.parametrize("overlap", [0.1, 0.25, 0.5])
def test_pass_through_returns_the_input(mdct_type, overlap):
    """With overlapping segments the pipeline returns the full amplitude for either transform: the stitch gain undoes the
    halving of util.imdct (reference_amplitude is False by default at overlap > 0)."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    real, opt = _tiny(mdct_type, lr_sampling_rate=24000)          # up_ratio 2: gain sqrt(2 - 1) = 1
    x = _clip(7 * opt.segment_length + 333).to(DEV)[None]
    y = SuperResolver(PassThrough(real), opt, overlap=overlap).enhance_lr(x)
    assert y.shape == x.shape
    err = (y - x).abs().max().item()
    bound = 2e-4 * x.abs().max().item() + 1e-5
    print(f"pass-through {mdct_type} overlap {overlap}: err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, err


def test_reference_amplitude_switch():
    """mdct2 at overlap 0 is the reference-exact mode and keeps the reference's amplitude: its util.imdct halves what
    IMDCT2(MDCT2(x)) = x returns, so the encoding of x comes back as x / 2 (up_ratio 2: sqrt(up_ratio - 1) = 1).  The switch
    overrides the default either way, the results differ by the exact factor 2, and mdct4 has no reference to keep."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    real, opt = _tiny("mdct2", lr_sampling_rate=24000)
    stub = PassThrough(real)
    x = _clip(3 * opt.segment_length + 77).to(DEV)[None]
    bound = 2e-4 * x.abs().max().item() + 1e-5
    ref0 = SuperResolver(stub, opt, overlap=0, graph=False)
    assert ref0.reference_amplitude and not SuperResolver(stub, opt, overlap=0.25).reference_amplitude
    half = ref0.enhance_lr(x)
    assert (2 * half - x).abs().max().item() <= bound
    full = SuperResolver(stub, opt, overlap=0, graph=False, reference_amplitude=False).enhance_lr(x)
    assert torch.equal(full, 2 * half) and (full - x).abs().max().item() <= bound
    kept = SuperResolver(stub, opt, overlap=0.25, graph=False, reference_amplitude=True).enhance_lr(x)
    assert (2 * kept - x).abs().max().item() <= bound
    real4, opt4 = _tiny("mdct4", lr_sampling_rate=24000)
    sr4 = SuperResolver(PassThrough(real4), opt4, overlap=0, graph=False, reference_amplitude=True)
    assert not sr4.reference_amplitude and (sr4.enhance_lr(x) - x).abs().max().item() <= bound


def test_random_draws_inside_the_chain_run_eagerly():
    """mask_mode 'mode1' draws its signs inside to_spectro: such a chain is never captured, so graph=True gives what
    graph=False gives from the same generator state."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct2", mask_mode="mode1")
    lr = (0.5 * _clip(4 * opt.segment_length + 100)).to(DEV)[None]
    a, b = SuperResolver(model, opt, overlap=0, graph=True), SuperResolver(model, opt, overlap=0, graph=False)
    assert not a._graph_ok()
    torch.manual_seed(3)
    ya = a.enhance_lr(lr)
    torch.manual_seed(3)
    assert torch.equal(b.enhance_lr(lr), ya) and a._g is None


# ------------------------------------------------------------------------------------------
# 6. launch accounting
# ------------------------------------------------------------------------------------------
CONV_FAMILIES = (b"gconv", b"c7", b"march", b"dfirst", b"dlast")


def _conv_launches(reset=1):
    from pix2pixhdaudiosr_amd import _lib
    return sum(_lib.lib().p2phd_launch_count(f, reset) for f in CONV_FAMILIES)


def test_launch_accounting():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct2")
    T = opt.segment_length
    lib = _lib.lib()
    eager = SuperResolver(model, opt, overlap=0, graph=False)
    for L in (10, 3 * T + 5, 6 * T):                              # 1, 4 and 6 segments
        lr = torch.randn(1, L, device=DEV) * 0.1
        lib.p2phd_launch_count(b"stitch", 1)
        eager.enhance_lr(lr)
        assert lib.p2phd_launch_count(b"stitch", 1) == 2          # one gather and one stitch, whatever S is
    lr = torch.randn(1, 6 * T, device=DEV) * 0.1                  # three full groups
    eager.enhance_lr(lr)                                          # (packed weights exist from here on)
    _conv_launches()
    eager.enhance_lr(lr)
    per_run = _conv_launches()
    assert per_run > 0 and per_run % 3 == 0
    per_group = per_run // 3
    graphed = SuperResolver(model, opt, overlap=0, graph=True)
    lib.p2phd_launch_count(b"stitch", 1)
    graphed.enhance_lr(lr)
    assert _conv_launches() == 2 * per_group                      # the eager run in front of the capture + the capture itself
    graphed.enhance_lr(lr)
    assert _conv_launches() == 0                                  # replays launch nothing through the library
    assert lib.p2phd_launch_count(b"stitch", 1) == 4              # gather and stitch stay outside the graph


# ------------------------------------------------------------------------------------------
# 7. files and the command line
# ------------------------------------------------------------------------------------------
def test_file_round_trip_and_cli(tmp_path):
    from test_gpu_model import make_opt
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.data.resample import resample
    from pix2pixhdaudiosr_amd.generate import SuperResolver, opt_from_file
    from pix2pixhdaudiosr_amd.models.models import create_model
    pcm = _clip(24000)
    clip = str(tmp_path / "clip.wav")
    wavio.save(clip, pcm, 48000)
    common = dict(mdct_type="mdct4", segment_length=127 * 32, batchSize=2, checkpoints_dir=str(tmp_path), name="run", seed=1234)
    torch.manual_seed(1234)
    create_model(make_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:                      # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(make_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    opt = opt_from_file(str(folder / "opt.txt"))
    assert opt.isTrain is False and opt.segment_length == 127 * 32 and opt.mask_mode == "mode2"
    model = create_model(opt)
    model.eval()
    out = str(tmp_path / "sr.wav")
    torch.manual_seed(opt.seed)
    res = SuperResolver(model, opt).enhance_file(clip, out)
    meta = wavio.info(out)
    assert (meta.sample_rate, meta.num_frames, meta.num_channels) == (48000, 24000, 1)
    assert tuple(res['sr'].shape) == (1, 24000) and tuple(res['lr'].shape) == (1, 24000) and tuple(res['hr'].shape) == (1, 24000)
    assert len(res['metrics']) == 7 and all(np.isfinite(v) for v in res['metrics'])
    assert res['metrics'][2] > 5.0                                # the LR round trip keeps the low band: SNR_LR > 5 dB
    # a low-rate clip: six times the samples, nothing to compare with
    lo = str(tmp_path / "lo.wav")
    wavio.save(lo, resample(pcm.to(DEV)[None], 48000, 8000), 8000)
    n_lo = wavio.info(lo).num_frames
    out_lo = str(tmp_path / "sr_lo.wav")
    res_lo = SuperResolver(model, opt, graph=False).enhance_file(lo, out_lo, is_lr_input=True)
    assert wavio.info(out_lo).num_frames == 6 * n_lo and wavio.info(out_lo).sample_rate == 48000
    assert res_lo['hr'] is None and res_lo['metrics'] is None
    # the command line, in a process of its own, writes the same file
    out_cli = str(tmp_path / "sr_cli.wav")
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.generate", "--input", clip, "--output", out_cli,
                        "--load_pretrain", str(folder)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "SNR_LR:" in p.stdout and "LSD:" in p.stdout
    with open(out, "rb") as a, open(out_cli, "rb") as b:
        assert a.read() == b.read()
