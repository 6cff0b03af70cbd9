"""SuperResolver(norm_scope='clip') / --norm_scope on the GPU: 'group' is today's path with no launch of the family
"normscope"; with 'clip' a pass-through generator writes the same clip at every batch size, the real tiny generator is given the
same encoded segments at every batch size, graph replay is the eager run, digital silence stays finite (and, passed through,
silent) where 'group' writes NaN, a dual-mono pair stays dual mono under stereo='ms', the launches of a clip are counted, and the
file, folder and command-line paths carry the option.  The tiny model and the clip are those of tests/test_gpu_lowband.py:
4 T + 100 samples, five segments at overlap 0."""
import math
import os

import pytest
import torch

from test_gpu_lowband import _clip, _noise, _opt, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = (1, 2, 5)
S = 5


def _count(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(b"normscope", 1 if reset else 0)


def _lr(T, gap=False):
    """The clip [1, 4 T + 100]; with `gap` the samples [T, 3 T) -- segments 1 and 2 -- are digital silence."""
    x = (0.5 * _clip(4 * T + 100)).to(DEV)[None].clone()
    if gap:
        x[:, T:3 * T] = 0.0
    return x


class PassThrough:
    """`inference` returns the encoding of its own input, as generator output and as input spectrogram; `norm` goes on to
    to_spectro, so the output depends on the codec kernels and the transforms only."""

    def __init__(self, real):
        self.real, self.mdct_type, self.device = real, real.mdct_type, real.device

    def inference(self, lr_audio, inst, noise=None, norm=None):
        spectro, pha, nrm = self.real.to_spectro(lr_audio, mask=False, norm=norm)
        return spectro, pha, nrm, spectro

    def clip_norm(self, segments, noise=None, rows=None):
        return self.real.clip_norm(segments, rows=rows)


class Recording:
    """The real model, with every segment's encoded input kept as `inference` hands it to the generator."""

    def __init__(self, real):
        self.real, self.mdct_type, self.device = real, real.mdct_type, real.device
        self.mask_noise_shape, self.clip_norm = real.mask_noise_shape, real.clip_norm
        self.rows = []

    def inference(self, lr_audio, inst, noise=None, **kw):
        out = self.real.inference(lr_audio, inst, noise=noise, **kw)
        _, pha, norm, lr_spectro = out
        for i in range(lr_audio.shape[0]):
            self.rows.append((lr_spectro[i].clone(), pha[i].clone(), norm['_minmax'].clone()))
        return out


# ------------------------------------------------------------------------------------------
# the fact the bit-for-bit claims rest on (it holds without this option as well)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_transform_rows_do_not_depend_on_the_batch(mdct_type):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segments_gather_planar
    model, opt = _tiny(mdct_type)
    T = opt.segment_length
    seg = segments_gather_planar(_lr(T), T, T, S)
    assert tuple(seg.shape) == (S, T)
    spec = model._mdct(seg)
    inv = SuperResolver(model, opt, overlap=0)._imdct
    back = inv(spec)
    for i in range(S):
        assert torch.equal(model._mdct(seg[i:i + 1])[0], spec[i]), i
        assert torch.equal(inv(spec[i:i + 1].contiguous()).reshape(-1), back[i].reshape(-1)), i
    assert torch.equal(model._mdct(seg[1:3]), spec[1:3])


# ------------------------------------------------------------------------------------------
# 'group' is today's path
# ------------------------------------------------------------------------------------------
def test_group_scope_is_todays_path():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    lr = _lr(opt.segment_length)
    plain = SuperResolver(model, opt, overlap=0)
    noise = _noise(plain, S, 31)
    assert plain.norm_scope == 'group'
    _count(reset=True)
    want = plain.enhance_lr(lr, noise=noise)
    named = SuperResolver(model, opt, overlap=0, norm_scope='group')
    assert torch.equal(named.enhance_lr(lr, noise=noise), want)
    assert _count() == 0 and named.last_norm is None
    with pytest.raises(ValueError, match=r"norm_scope must be 'group' or 'clip'"):
        SuperResolver(model, opt, norm_scope='file')


# ------------------------------------------------------------------------------------------
# 'clip' with a pass-through generator: the codec and the transforms alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_clip_scope_passes_through_the_same_at_every_batch(mdct_type):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    stub = PassThrough(model)
    lr = _lr(opt.segment_length)
    outs = {scope: [SuperResolver(stub, opt, overlap=0, batch=b, norm_scope=scope).enhance_lr(lr) for b in BATCHES]
            for scope in ('group', 'clip')}
    for y in outs['clip'] + outs['group']:
        assert tuple(y.shape) == tuple(lr.shape) and torch.isfinite(y).all() and y.abs().max() > 0
    assert torch.equal(outs['clip'][0], outs['clip'][1]) and torch.equal(outs['clip'][0], outs['clip'][2])
    assert not (torch.equal(outs['group'][0], outs['group'][1]) and torch.equal(outs['group'][0], outs['group'][2]))
    # with overlapping segments as well (another segment count, cross-fades)
    a, b = (SuperResolver(stub, opt, overlap=0.25, batch=n, norm_scope='clip').enhance_lr(lr) for n in (1, 4))
    assert torch.equal(a, b)
    # every channel is a clip of its own
    two = torch.cat([lr, 0.01 * lr.flip(1)])
    sr = SuperResolver(stub, opt, overlap=0, batch=2, norm_scope='clip')
    both = sr.enhance_lr(two)
    norms = sr.last_norm.clone()
    for c in range(2):
        assert torch.equal(sr.enhance_lr(two[c:c + 1])[0], both[c])
        assert torch.equal(sr.last_norm[0], norms[c])
    assert tuple(norms.shape) == (2, 2) and bool((norms[:, 0] < norms[:, 1]).all()) and float(norms[1, 1]) < float(norms[0, 1])


# ------------------------------------------------------------------------------------------
# 'clip' with the real tiny generator
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_clip_scope_with_the_generator(mdct_type):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    lr = _lr(opt.segment_length)
    noise = _noise(SuperResolver(model, opt, overlap=0), S, 32)
    recs, outs = {}, {}
    for b in (1, 5):
        rec = Recording(model)
        outs[b] = SuperResolver(rec, opt, overlap=0, batch=b, graph=False, norm_scope='clip').enhance_lr(lr, noise=noise)
        recs[b] = rec.rows
    assert len(recs[1]) == len(recs[5]) == S
    for i in range(S):
        for got, want in zip(recs[1][i], recs[5][i]):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), i
    for i in range(1, S):
        assert torch.equal(recs[1][i][2], recs[1][0][2])           # one range for the clip
    # the generator's own dependence on its batch size (its padding and its normalisation layers see the batch): reported only
    print(f"{mdct_type}: largest difference between the batch-1 and the batch-5 waveform {float((outs[1] - outs[5]).abs().max()):.3e} "
          f"at a peak of {float(outs[5].abs().max()):.3e}")
    group = SuperResolver(model, opt, overlap=0, batch=2, graph=False).enhance_lr(lr, noise=noise)
    eager = SuperResolver(model, opt, overlap=0, batch=2, graph=False, norm_scope='clip')
    got = eager.enhance_lr(lr, noise=noise)
    assert tuple(got.shape) == tuple(lr.shape) and torch.isfinite(got).all() and not torch.equal(got, group)
    # graph replay is the eager run, and the next clip replays the same capture with its own range
    graphed = SuperResolver(model, opt, overlap=0, batch=2, graph=True, norm_scope='clip')
    assert torch.equal(graphed.enhance_lr(lr, noise=noise), got)
    capture = graphed._g['graph']
    assert capture is not None
    quiet = 0.05 * lr.flip(1)
    want = eager.enhance_lr(quiet, noise=noise)
    quiet_norm = eager.last_norm.clone()
    assert torch.equal(graphed.enhance_lr(quiet, noise=noise), want) and graphed._g['graph'] is capture
    assert torch.equal(graphed.last_norm, quiet_norm) and torch.equal(graphed._g['norm'][:2], quiet_norm[0])
    assert torch.equal(graphed.enhance_lr(lr, noise=noise), got) and graphed._g['graph'] is capture
    # without a given noise the channel's noise is one draw
    torch.manual_seed(7)
    drawn = eager.enhance_lr(lr)
    torch.manual_seed(7)
    shape = eager.noise_shape(S)
    assert torch.equal(eager.enhance_lr(lr, noise=torch.randn(shape, device=DEV)), drawn)


# ------------------------------------------------------------------------------------------
# silence
# ------------------------------------------------------------------------------------------
def test_silence_stays_finite_and_passed_through_silent():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    T = opt.segment_length
    lr = _lr(T, gap=True)
    noise = _noise(SuperResolver(model, opt, overlap=0), S, 33)
    group = SuperResolver(model, opt, overlap=0, batch=1).enhance_lr(lr, noise=noise)
    assert not torch.isfinite(group[:, T:3 * T]).any()             # the reason for the option
    assert torch.isfinite(group[:, :T]).all() and torch.isfinite(group[:, 3 * T:]).all()
    clip = SuperResolver(model, opt, overlap=0, batch=1, norm_scope='clip').enhance_lr(lr, noise=noise)
    assert torch.isfinite(clip).all() and clip[:, :T].abs().max() > 0
    stub = PassThrough(model)
    through = SuperResolver(stub, opt, overlap=0, batch=1, norm_scope='clip').enhance_lr(lr)
    assert torch.isfinite(through).all() and bool((through[:, T:3 * T] == 0).all()) and through[:, :T].abs().max() > 0
    assert not torch.isfinite(SuperResolver(stub, opt, overlap=0, batch=1).enhance_lr(lr)[:, T:3 * T]).any()
    # a clip that is silence throughout: a range of zero
    nothing = torch.zeros_like(lr)
    for m, kw in ((stub, {}), (model, dict(noise=noise))):
        sr = SuperResolver(m, opt, overlap=0, batch=2, norm_scope='clip')
        out = sr.enhance_lr(nothing, **kw)
        assert bool((out == 0).all())
        assert float(sr.last_norm[0, 0]) == float(sr.last_norm[0, 1]) and math.isfinite(float(sr.last_norm[0, 0]))


def test_dual_mono_stays_dual_mono_under_mid_side():
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    model, opt = _tiny("mdct4")
    mono = _lr(opt.segment_length)
    sr = SuperResolver(model, opt, overlap=0.25, stereo='ms', norm_scope='clip')
    noise = _noise(sr, 2 * segment_plan(mono.shape[1], opt.segment_length, 0.25)[0], 34)
    out = sr.enhance_lr(torch.cat([mono, mono]), noise=noise)
    assert tuple(out.shape) == (2, mono.shape[1]) and torch.isfinite(out).all() and out.abs().max() > 0
    assert torch.equal(out[0], out[1])
    assert float(sr.last_norm[1, 0]) == float(sr.last_norm[1, 1])  # the side signal: digital silence, a range of zero


# ------------------------------------------------------------------------------------------
# the launches of a clip
# ------------------------------------------------------------------------------------------
def test_launch_count_of_a_clip():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    lr = _lr(opt.segment_length)
    for batch in (2, 5):
        sr = SuperResolver(model, opt, overlap=0, batch=batch, graph=False, norm_scope='clip')
        noise = _noise(sr, 2 * S, 35)
        groups = math.ceil(S / batch)
        _count(reset=True)
        sr.enhance_lr(lr, noise=noise[:S])
        assert _count(reset=True) == groups + 1 + groups           # range calls, the noise fold, one encode per group
        sr.enhance_lr(torch.cat([lr, lr]), noise=noise)
        assert _count(reset=True) == 2 * (groups + 1 + groups)
    # a generator that is given no mask noise: no fold
    SuperResolver(PassThrough(model), opt, overlap=0, batch=2, graph=False, norm_scope='clip').enhance_lr(lr)
    assert _count(reset=True) == 3 + 3


# ------------------------------------------------------------------------------------------
# files, folders, the command line
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("norm_scope_in")
    x = 0.5 * _clip(24000)                                         # 0.5 s: two 400 ms blocks for the folder's loudness
    wavio.save(str(d / "a.wav"), torch.stack([x, 0.3 * x.flip(0)]), 48000)
    wavio.save(str(d / "b.wav"), x[:21000], 48000)
    return d


def test_enhance_file_and_folder_carry_the_ranges(folder, tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    group, clip = SuperResolver(model, opt), SuperResolver(model, opt, norm_scope='clip')
    res = group.enhance_file(str(folder / "a.wav"), str(tmp_path / "g.wav"), channels='all')
    assert 'norm' not in res
    res = clip.enhance_file(str(folder / "a.wav"), str(tmp_path / "c.wav"), channels='all')
    norm = res['norm']
    assert norm.is_cuda and norm.dtype == torch.float32 and tuple(norm.shape) == (2, 2)
    assert bool((norm[:, 0] < norm[:, 1]).all()) and torch.isfinite(res['sr']).all()
    assert wavio.info(str(tmp_path / "c.wav")).num_frames == 24000
    assert tuple(clip.enhance_file(str(folder / "a.wav"), None)['norm'].shape) == (1, 2)
    for kw in ({}, dict(loudness='report', loudness_scope='folder')):
        recs = group.enhance_folder(str(folder), str(tmp_path / ("fg%d" % len(kw))), channels='all', **kw)
        assert [r['error'] for r in recs] == [None, None] and all('norm' not in r for r in recs)
        recs = clip.enhance_folder(str(folder), str(tmp_path / ("fc%d" % len(kw))), channels='all', **kw)
        assert [r['error'] for r in recs] == [None, None]
        assert [tuple(r['norm'].shape) for r in recs] == [(2, 2), (1, 2)] and all(r['norm'].is_cuda for r in recs)
        assert os.path.isfile(str(tmp_path / ("fc%d" % len(kw)) / "b.wav"))
        if kw:
            assert recs[0]['album'] is not None and recs[0]['album']['files'] == 2


def test_command_line(tmp_path, capsys):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import main
    from pix2pixhdaudiosr_amd.models.models import create_model
    clip = str(tmp_path / "clip.wav")
    wavio.save(clip, _clip(6000), 48000)
    common = dict(mdct_type="mdct4", checkpoints_dir=str(tmp_path), name="run", seed=1234)
    torch.manual_seed(1234)
    create_model(_opt(**common)).save('latest')
    run = tmp_path / "run"
    with open(run / "opt.txt", "w") as f:                         # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    base = ["--input", clip, "--load_pretrain", str(run)]
    line = 'normalisation: one range per clip'
    capsys.readouterr()
    assert main(base + ["--output", str(tmp_path / "g.wav")]) == 0
    plain = capsys.readouterr().out
    assert main(base + ["--output", str(tmp_path / "g2.wav"), "--norm_scope", "group"]) == 0
    assert capsys.readouterr().out.replace("g2.wav", "g.wav") == plain and line not in plain
    assert main(base + ["--output", str(tmp_path / "c.wav"), "--norm_scope", "clip"]) == 0
    out = capsys.readouterr().out
    assert out.splitlines().count(line) == 1 and len(out.splitlines()) == len(plain.splitlines()) + 1
    with open(tmp_path / "g.wav", "rb") as a, open(tmp_path / "g2.wav", "rb") as b, open(tmp_path / "c.wav", "rb") as c:
        ga, gb, cc = a.read(), b.read(), c.read()
    assert ga == gb and len(cc) == len(ga) and cc != ga
    with pytest.raises(SystemExit):
        main(base + ["--output", str(tmp_path / "never.wav"), "--norm_scope", "file"])
    assert "--norm_scope" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "never.wav"))
