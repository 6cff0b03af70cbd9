"""SuperResolver(segment_norm=True) / --segment_norm on the GPU: off is today's path with no launch of the family "normrows"; on,
a pass-through generator writes the same clip at every batch size -- at overlap 0 the clip 'group' writes at batch 1 --, channels
share groups and stay clips of their own, the real tiny generator is given the same encoded segments at every batch size, every
group is a full one so that graph replay is the eager run and one capture serves clips of any length and channel count, digital
silence is written as silence where 'group' writes NaN, and the file, folder, album and command-line paths carry the option.
The tiny model and the clip are those of tests/test_gpu_lowband.py (4 T + 100 samples, five segments at overlap 0), the wrapped
models those of tests/test_gpu_generate_norm_scope.py."""
import math
import os

import pytest
import torch

from test_gpu_generate_norm_scope import PassThrough, Recording, _lr
from test_gpu_lowband import _clip, _noise, _opt, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = (1, 2, 5)
S = 5


def _count(family=b"normrows", reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(family, 1 if reset else 0)


class PassThroughRows(PassThrough):
    """PassThrough hands `norm` on to to_spectro as it is: 'rows' too.  It draws no mask noise."""


class RecordingRows(Recording):
    """Recording for either kind of norm dict: a row's range is its own row of the table ('rows') or the batch's two floats."""

    def inference(self, lr_audio, inst, noise=None, **kw):
        out = self.real.inference(lr_audio, inst, noise=noise, **kw)
        _, pha, norm, lr_spectro = out
        for i in range(lr_audio.shape[0]):
            rng = norm['rows'][i, :2] if norm.get('rows') is not None else norm['_minmax']
            self.rows.append((lr_spectro[i].clone(), pha[i].clone(), rng.clone()))
        return out


def _real_rows(rows, n, batch):
    """What a RecordingRows kept for n rows walked in full groups of `batch` -> the n rows without the fillers."""
    from pix2pixhdaudiosr_amd.generate import group_rows_plan
    plan = group_rows_plan(n, batch)
    assert len(rows) == batch * len(plan)
    return [rows[g * batch + i] for g, (_, k) in enumerate(plan) for i in range(k)]


# ------------------------------------------------------------------------------------------
# off is today's path
# ------------------------------------------------------------------------------------------
def test_off_is_todays_path():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    lr = _lr(opt.segment_length)
    plain = SuperResolver(model, opt, overlap=0)
    noise = _noise(plain, S, 51)
    assert plain.segment_norm is False
    _count(reset=True)
    want = plain.enhance_lr(lr, noise=noise)
    named = SuperResolver(model, opt, overlap=0, segment_norm=False)
    assert torch.equal(named.enhance_lr(lr, noise=noise), want)
    clip = SuperResolver(model, opt, overlap=0, norm_scope='clip')
    clip.enhance_lr(lr, noise=noise)
    assert _count() == 0 and named.last_norm is None and tuple(clip.last_norm.shape) == (1, 2)
    on = SuperResolver(model, opt, overlap=0, segment_norm=True)
    _count(b"normscope", reset=True)
    got = on.enhance_lr(lr, noise=noise)
    assert _count() > 0 and _count(b"normscope") == 0 and not torch.equal(got, want)


def test_refused_with_clip_scope_before_a_file_is_opened(tmp_path, capsys):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, main
    model, opt = _tiny("mdct4")
    with pytest.raises(ValueError, match=r"segment_norm gives every segment its own range and norm_scope 'clip'"):
        SuperResolver(model, opt, norm_scope='clip', segment_norm=True)
    with pytest.raises(SystemExit):
        main(["--input", str(tmp_path / "none.wav"), "--output", str(tmp_path / "never.wav"), "--load_pretrain", str(tmp_path / "none"),
              "--segment_norm", "--norm_scope", "clip"])
    assert "segment_norm" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "never.wav"))


# ------------------------------------------------------------------------------------------
# a pass-through generator: the codec and the transforms alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 0.25])
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_passes_through_the_same_at_every_batch(mdct_type, overlap):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    model, opt = _tiny(mdct_type)
    stub = PassThroughRows(model)
    lr = _lr(opt.segment_length)
    segs = segment_plan(lr.shape[1], opt.segment_length, overlap)[0]
    _count(reset=True)
    outs, norms = [], []
    for b in BATCHES:
        sr = SuperResolver(stub, opt, overlap=overlap, batch=b, graph=False, segment_norm=True)
        outs.append(sr.enhance_lr(lr))
        norms.append(sr.last_norm.clone())
        assert _count(reset=True) == 2 * math.ceil(segs / b)       # an encode and a decode per group, every group a full one
        graphed = SuperResolver(stub, opt, overlap=overlap, batch=b, segment_norm=True)
        assert torch.equal(graphed.enhance_lr(lr), outs[-1]) and torch.equal(graphed.last_norm, norms[-1])
        assert _count(reset=True) == 4                             # the warm-up and the capture; a replay calls no entry
    for y, n in zip(outs, norms):
        assert tuple(y.shape) == tuple(lr.shape) and torch.isfinite(y).all() and y.abs().max() > 0
        assert torch.equal(y, outs[0]) and torch.equal(n, norms[0])
        assert tuple(n.shape) == (1, segs, 2) and bool((n[..., 0] < n[..., 1]).all())
    if overlap == 0:                                               # what 'group' means at batch 1
        assert torch.equal(outs[0], SuperResolver(stub, opt, overlap=0, batch=1).enhance_lr(lr))
        assert not torch.equal(outs[0], SuperResolver(stub, opt, overlap=0, batch=5).enhance_lr(lr))


def _each_channel_is_its_own_clip(stub, opt, two, batch, **kw):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver(stub, opt, batch=batch, segment_norm=True, **kw)
    both = sr.enhance_lr(two)
    norms = sr.last_norm.clone()
    assert tuple(both.shape) == tuple(two.shape) and torch.isfinite(both).all() and tuple(norms.shape)[::2] == (2, 2)
    for c in range(2):
        assert torch.equal(sr.enhance_lr(two[c:c + 1])[0], both[c]), (c, kw)
        assert torch.equal(sr.last_norm[0], norms[c]), (c, kw)
    return both, norms


@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_channels_share_groups_and_stay_clips_of_their_own(mdct_type):
    """Two channels a factor of 100 apart, five segments each: at batch 2 and 4 the third and the second group hold rows of both.
    lowband_fade 8 needs the 10 kept rows of mdct2; mdct4 keeps 5 and runs fade 0 and 5."""
    from pix2pixhdaudiosr_amd.generate import spectro_bins
    model, opt = _tiny(mdct_type)
    stub = PassThroughRows(model)
    lr = _lr(opt.segment_length)
    two = torch.cat([lr, 0.01 * lr.flip(1)])
    keep = int(spectro_bins(opt.n_fft, mdct_type) / (opt.hr_sampling_rate / opt.lr_sampling_rate))
    for batch in (2, 4):
        both, norms = _each_channel_is_its_own_clip(stub, opt, two, batch, overlap=0)
        assert float(norms[1, :, 1].max()) < float(norms[0, :, 1].max()) - 30.0      # (40 dB apart, flipped)
    for fade in (0, min(8, keep)):
        assert mdct_type != "mdct2" or fade in (0, 8)
        _each_channel_is_its_own_clip(stub, opt, two, 2, overlap=0.25, lowband='input', lowband_fade=fade)
    _each_channel_is_its_own_clip(stub, opt, two, 2, overlap=0.25, crossover='input')
    # the auto crossover measures all channels as one programme: channels of one content, so that each alone measures the same edge
    same = torch.cat([lr, 0.01 * lr])
    _each_channel_is_its_own_clip(stub, opt, same, 4, overlap=0.25, crossover='input', crossover_hz='auto')


# ------------------------------------------------------------------------------------------
# the real tiny generator
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_with_the_generator(mdct_type):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    lr = _lr(opt.segment_length)
    noise = _noise(SuperResolver(model, opt, overlap=0), S, 52)
    recs, outs = {}, {}
    for b in (1, 5):
        rec = RecordingRows(model)
        outs[b] = SuperResolver(rec, opt, overlap=0, batch=b, graph=False, segment_norm=True).enhance_lr(lr, noise=noise)
        recs[b] = _real_rows(rec.rows, S, b)
    rec = RecordingRows(model)
    group1 = SuperResolver(rec, opt, overlap=0, batch=1, graph=False).enhance_lr(lr, noise=noise)
    recs['group'] = rec.rows
    assert len(recs[1]) == len(recs[5]) == len(recs['group']) == S
    for i in range(S):
        for k in (5, 'group'):
            for got, want in zip(recs[k][i], recs[1][i]):
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (i, k)
    assert len({tuple(r[2].tolist()) for r in recs[1]}) == S       # a range per segment
    assert torch.equal(outs[1], group1)                            # what 'group' writes at batch 1
    # the generator's own dependence on its batch size (its padding and its normalisation layers see the batch): reported only
    print(f"{mdct_type}: largest difference between the batch-1 and the batch-5 waveform {float((outs[1] - outs[5]).abs().max()):.3e} "
          f"at a peak of {float(outs[5].abs().max()):.3e}")
    # graph replay is the eager run: S = 5 at batch 2, the last group one row and a filler
    eager = SuperResolver(model, opt, overlap=0, batch=2, graph=False, segment_norm=True)
    got = eager.enhance_lr(lr, noise=noise)
    want_norm = eager.last_norm.clone()
    assert tuple(got.shape) == tuple(lr.shape) and torch.isfinite(got).all()
    graphed = SuperResolver(model, opt, overlap=0, batch=2, graph=True, segment_norm=True)
    assert torch.equal(graphed.enhance_lr(lr, noise=noise), got) and torch.equal(graphed.last_norm, want_norm)
    assert graphed._g['graph'] is not None
    # without a given noise a group's noise is one draw of the full group's shape
    torch.manual_seed(7)
    drawn = eager.enhance_lr(lr)
    torch.manual_seed(7)
    shape = eager.noise_shape(2)
    given = torch.cat([torch.randn(shape, device=DEV) for _ in range(3)])[:S]
    assert torch.equal(eager.enhance_lr(lr, noise=given)[:, :4 * opt.segment_length], drawn[:, :4 * opt.segment_length])


def test_one_capture_serves_clips_of_any_length_and_channel_count():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    T = opt.segment_length
    one = _lr(T)                                                   # 1 channel, 5 segments: 5 rows
    two = torch.cat([one[:, :2 * T + 50], 0.3 * one[:, T:3 * T + 50]])               # 2 channels, 3 segments each: 6 rows
    graphed = SuperResolver(model, opt, overlap=0, batch=4, graph=True, segment_norm=True)
    eager = SuperResolver(model, opt, overlap=0, batch=4, graph=False, segment_norm=True)
    noise = _noise(graphed, 6, 53)
    calls = []
    inner = graphed._group
    graphed._group = lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1]
    first = graphed.enhance_lr(one, noise=noise[:5])
    capture = graphed._g['graph']
    assert capture is not None and len(calls) == 2                 # the warm-up and the capture
    second = graphed.enhance_lr(two, noise=noise)
    assert len(calls) == 2 and graphed._g['graph'] is capture
    assert tuple(graphed.last_norm.shape) == (2, 3, 2)
    assert torch.equal(second, eager.enhance_lr(two, noise=noise)) and torch.equal(graphed.last_norm, eager.last_norm)
    assert torch.equal(first, eager.enhance_lr(one, noise=noise[:5]))
    assert torch.equal(graphed.enhance_lr(one, noise=noise[:5]), first) and len(calls) == 2 and graphed._g['graph'] is capture


# ------------------------------------------------------------------------------------------
# silence
# ------------------------------------------------------------------------------------------
def test_silence_is_written_as_silence():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    T = opt.segment_length
    lr = _lr(T, gap=True)                                          # segments 1 and 2 are digital silence
    noise = _noise(SuperResolver(model, opt, overlap=0), S, 54)
    group = SuperResolver(model, opt, overlap=0, batch=1).enhance_lr(lr, noise=noise)
    assert not torch.isfinite(group[:, T:3 * T]).any()             # the existing behaviour: what the option changes
    stub = PassThroughRows(model)
    for batch in (1, 2):
        sr = SuperResolver(model, opt, overlap=0, batch=batch, segment_norm=True)
        out = sr.enhance_lr(lr, noise=noise)
        assert torch.isfinite(out).all() and out[:, :T].abs().max() > 0 and out[:, 3 * T:].abs().max() > 0
        n = sr.last_norm[0]
        assert n[1, 0] == n[1, 1] and n[2, 0] == n[2, 1] and bool((n[[0, 3, 4], 0] < n[[0, 3, 4], 1]).all())
        through = SuperResolver(stub, opt, overlap=0, batch=batch, segment_norm=True).enhance_lr(lr)
        assert torch.isfinite(through).all() and bool((through[:, T:3 * T] == 0).all())
        assert through[:, :T].abs().max() > 0 and through[:, 3 * T:].abs().max() > 0
    # a clip that is silence throughout
    nothing = torch.zeros_like(lr)
    for m, kw in ((stub, {}), (model, dict(noise=noise))):
        sr = SuperResolver(m, opt, overlap=0, batch=2, segment_norm=True)
        out = sr.enhance_lr(nothing, **kw)
        assert bool((out == 0).all())
        assert bool((sr.last_norm[..., 0] == sr.last_norm[..., 1]).all()) and torch.isfinite(sr.last_norm).all()
        assert not torch.isfinite(SuperResolver(m, opt, overlap=0, batch=2).enhance_lr(nothing, **kw)).any()


def test_dual_mono_stays_dual_mono_under_mid_side():
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    model, opt = _tiny("mdct4")
    mono = _lr(opt.segment_length)
    sr = SuperResolver(model, opt, overlap=0.25, stereo='ms', segment_norm=True)
    noise = _noise(sr, 2 * segment_plan(mono.shape[1], opt.segment_length, 0.25)[0], 55)
    out = sr.enhance_lr(torch.cat([mono, mono]), noise=noise)
    assert tuple(out.shape) == (2, mono.shape[1]) and torch.isfinite(out).all() and out.abs().max() > 0
    assert torch.equal(out[0], out[1])
    assert bool((sr.last_norm[1, :, 0] == sr.last_norm[1, :, 1]).all())              # the side signal: digital silence throughout
    assert bool((sr.last_norm[0, :, 0] < sr.last_norm[0, :, 1]).all())


# ------------------------------------------------------------------------------------------
# files, folders, the album, the command line
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("segment_norm_in")
    x = 0.5 * _clip(24000)                                         # 0.5 s: two 400 ms blocks for the folder's loudness
    wavio.save(str(d / "a.wav"), torch.stack([x, 0.3 * x.flip(0)]), 48000)
    wavio.save(str(d / "b.wav"), x[:21000], 48000)
    return d


def test_enhance_file_folder_and_album_carry_the_ranges(folder, tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    model, opt = _tiny("mdct4")
    off, on = SuperResolver(model, opt), SuperResolver(model, opt, segment_norm=True)
    sa, sb = (segment_plan(n, opt.segment_length, on.overlap)[0] for n in (24000, 21000))
    assert 'norm' not in off.enhance_file(str(folder / "a.wav"), str(tmp_path / "g.wav"), channels='all')
    res = on.enhance_file(str(folder / "a.wav"), str(tmp_path / "s.wav"), channels='all')
    norm = res['norm']
    assert norm.is_cuda and norm.dtype == torch.float32 and tuple(norm.shape) == (2, sa, 2)
    assert bool((norm[..., 0] < norm[..., 1]).all()) and torch.isfinite(res['sr']).all()
    assert wavio.info(str(tmp_path / "s.wav")).num_frames == 24000
    assert tuple(on.enhance_file(str(folder / "a.wav"), None)['norm'].shape) == (1, sa, 2)
    for kw in ({}, dict(loudness='report', loudness_scope='folder')):
        recs = off.enhance_folder(str(folder), str(tmp_path / ("fg%d" % len(kw))), channels='all', **kw)
        assert [r['error'] for r in recs] == [None, None] and all('norm' not in r for r in recs)
        recs = on.enhance_folder(str(folder), str(tmp_path / ("fs%d" % len(kw))), channels='all', **kw)
        assert [r['error'] for r in recs] == [None, None]
        assert [tuple(r['norm'].shape) for r in recs] == [(2, sa, 2), (1, sb, 2)] and all(r['norm'].is_cuda for r in recs)
        assert os.path.isfile(str(tmp_path / ("fs%d" % len(kw)) / "b.wav"))
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
    line = 'normalisation: one range per segment'
    capsys.readouterr()
    assert main(base + ["--output", str(tmp_path / "g.wav")]) == 0
    plain = capsys.readouterr().out
    assert line not in plain
    _count(reset=True)
    assert main(base + ["--output", str(tmp_path / "s.wav"), "--segment_norm"]) == 0
    out = capsys.readouterr().out
    assert out.splitlines().count(line) == 1 and len(out.splitlines()) == len(plain.splitlines()) + 1 and _count() > 0
    assert main(base + ["--output", str(tmp_path / "s1.wav"), "--segment_norm", "--batchSize", "1"]) == 0
    capsys.readouterr()
    with open(tmp_path / "g.wav", "rb") as a, open(tmp_path / "s.wav", "rb") as b, open(tmp_path / "s1.wav", "rb") as c:
        ga, sa, s1 = a.read(), b.read(), c.read()
    assert len(sa) == len(ga) == len(s1) and sa != ga
    with pytest.raises(SystemExit):
        main(base + ["--output", str(tmp_path / "never.wav"), "--segment_norm", "--norm_scope", "clip"])
    assert "segment_norm" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "never.wav"))
