"""enhance_file / enhance_folder with stream_seconds (--stream_seconds) on the GPU: a file that goes through the pipeline in windows
(generate/stream.py) is written byte for byte as without the option -- with the pass-through generator, which draws no noise and
whose rows see themselves alone --, the real tiny generator is given the same ranges, the groups and the "stitch" launches are the
planned ones on one capture, device and pinned memory do not grow with the file, a failing window leaves nothing behind, and the
folder and command-line paths carry the option.  The tiny model and the clip are those of tests/test_gpu_lowband.py, the wrapped
model that of tests/test_gpu_generate_segment_norm.py."""
import os

import numpy as np
import pytest
import torch

import _containers_ref as CR
import _wavcodec_ref as WC
from test_gpu_generate_segment_norm import PassThroughRows
from test_gpu_lowband import _clip, _noise, _opt, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, BATCH = 31 * 32, 2


def _count(family=b"stitch", reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(family, 1 if reset else 0)


def _ints(frames):
    """int16 [2, frames]: the excerpt and, quieter, the excerpt backwards."""
    x = (_clip(frames) * 32768.0).round().numpy().astype(np.int64)
    return np.stack([x // 2, (3 * x[::-1]) // 10])


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """name -> (path, is_lr_input): two channels each."""
    d = tmp_path_factory.mktemp("stream_in")
    WC.write_pcm16_wav(str(d / "wav48.wav"), _ints(6000), 48000)
    WC.write_pcm16_wav(str(d / "wav44.wav"), _ints(5513), 44100)
    WC.write_coded_wav(str(d / "ulaw8.wav"), 7, WC.g711_encode(_ints(1003), 'ulaw'), 8000, 2)
    (d / "aiff48.aif").write_bytes(CR.aiff(CR.int_bytes(_ints(5001), 2), 2, 5001, 16, rate=48000))
    return {"wav48": (str(d / "wav48.wav"), False), "wav44": (str(d / "wav44.wav"), False), "ulaw8": (str(d / "ulaw8.wav"), True),
            "aiff48": (str(d / "aiff48.aif"), False)}


def _windows(sr, C):
    """stream_seconds for: one window per filler-free unit of segments (one segment with two channels), two groups, one window."""
    stride = sr.T - int(sr.overlap * sr.T)
    return (1e-6, (2 * BATCH // C) * stride / 48000.0, 100.0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _same_file(sr, path, is_lr, channels, tmp_path, windows, **kw):
    plain = sr.enhance_file(path, str(tmp_path / "plain.wav"), is_lr, channels, **kw)
    want = _bytes(tmp_path / "plain.wav")
    assert 'stream' not in plain and len(want) > 44
    C, S = plain['norm'].shape[:2]
    seen = []
    for W in windows:
        res = sr.enhance_file(path, str(tmp_path / "streamed.wav"), is_lr, channels, stream_seconds=W, **kw)
        assert _bytes(tmp_path / "streamed.wav") == want, (path, channels, W, kw)
        assert torch.equal(res['norm'].view(torch.int32), plain['norm'].view(torch.int32))
        st = res['stream']
        assert res['sr'] is None and res['lr'] is None and res['hr'] is None and res['metrics'] is None
        assert st['out_frames'] == plain['sr'].shape[-1] and st['frames'] == plain['info'].num_frames and res['info'] == plain['info']
        assert st['windows'] == -(-S // st['segments_per_window']) and (C * st['segments_per_window']) % sr.batch == 0
        seen.append(st['windows'])
        os.remove(tmp_path / "streamed.wav")
    os.remove(tmp_path / "plain.wav")
    return seen


# ------------------------------------------------------------------------------------------
# byte for byte the file written without the option
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 0.25])
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_streamed_is_the_unstreamed_file(inputs, tmp_path, mdct_type, overlap):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    sr = SuperResolver(PassThroughRows(model), opt, overlap=overlap, batch=BATCH, segment_norm=True)
    for name, (path, is_lr) in inputs.items():
        for channels, C in (('first', 1), ('all', 2)):
            seen = _same_file(sr, path, is_lr, channels, tmp_path, _windows(sr, C), encoding='pcm16', dither='tpdf', dither_seed=3)
            assert seen[0] > seen[1] > seen[2] == 1, (name, channels, seen)
    path, is_lr = inputs["wav48"]
    for encoding in ('pcm24', 'float32'):
        _same_file(sr, path, is_lr, 'all', tmp_path, _windows(sr, 2)[:2], encoding=encoding)
    _same_file(sr, path, is_lr, 'all', tmp_path, _windows(sr, 2)[:1], encoding='pcm16')          # no dither: the encoder alone


@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_streamed_is_the_unstreamed_file_with_the_row_options(inputs, tmp_path, mdct_type):
    """lowband 'input' with a hard switch and a fade (8 rows need the 10 kept rows of mdct2; mdct4 keeps 5), and mid / side."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    stub = PassThroughRows(model)
    for kw in (dict(lowband='input', lowband_fade=0), dict(lowband='input', lowband_fade=8 if mdct_type == 'mdct2' else 5), dict(stereo='ms')):
        sr = SuperResolver(stub, opt, overlap=0.25, batch=BATCH, segment_norm=True, **kw)
        for name in ("wav48", "wav44"):
            path, is_lr = inputs[name]
            _same_file(sr, path, is_lr, 'all', tmp_path, _windows(sr, 2)[:2], encoding='pcm16', dither='tpdf', dither_seed=1)


# ------------------------------------------------------------------------------------------
# the real generator
# ------------------------------------------------------------------------------------------
def test_real_generator_is_given_the_same_ranges(inputs, tmp_path):
    """With a given noise the ranges are the same bits streamed and not.  The waveforms are printed, not compared: what a generator
    does with a row's neighbours in the batch is its own business, and a window's groups hold other neighbours."""
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    from pix2pixhdaudiosr_amd.generate.resolver import _Options
    model, opt = _tiny("mdct4")
    sr = SuperResolver(model, opt, overlap=0.25, batch=BATCH, segment_norm=True)
    path, is_lr = inputs["wav48"]
    lr = sr.enhance_file(path, None, is_lr, 'all')['lr']
    S = sr.last_norm.shape[1]
    noise = _noise(sr, 2 * S, 7)
    want = sr.enhance_lr(lr, noise=noise)
    norm = sr.last_norm.clone()
    off = _Options(None, None, None, None, None, None, None, None, None, None)
    for W in _windows(sr, 2):
        res = sr._enhance_stream(path, str(tmp_path / "s.wav"), is_lr, 'all', 'float32', off, W, noise=noise)
        assert torch.equal(res['norm'].view(torch.int32), norm.view(torch.int32)), W
        got = wavio.load(str(tmp_path / "s.wav"))[0]
        assert tuple(got.shape) == tuple(want.shape) and torch.isfinite(got).all()
        print("stream_seconds %g: %d windows, largest waveform difference %.3e (peak %.3e)"
              % (W, res['stream']['windows'], float((got - want.cpu()).abs().max()), float(want.abs().max())))
    with pytest.raises(ValueError, match=r"noise holds"):
        sr._enhance_stream(path, None, is_lr, 'all', 'float32', off, 1.0, noise=noise[:-1])
    # one written channel: the windows' groups are the clip's groups, so the drawn noise is the unstreamed run's too
    torch.manual_seed(11)
    sr.enhance_file(path, str(tmp_path / "p1.wav"), is_lr, 'first', 'float32')
    torch.manual_seed(11)
    sr.enhance_file(path, str(tmp_path / "s1.wav"), is_lr, 'first', 'float32', stream_seconds=1e-6)
    assert _bytes(tmp_path / "p1.wav") == _bytes(tmp_path / "s1.wav")


# ------------------------------------------------------------------------------------------
# launches, the option off, memory
# ------------------------------------------------------------------------------------------
def test_groups_and_stitch_launches_are_the_planned_ones_on_one_capture(inputs, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, stream_plan
    model, opt = _tiny("mdct4")
    sr = SuperResolver(PassThroughRows(model), opt, overlap=0.25, batch=BATCH, segment_norm=True)
    calls = []
    inner = sr._group_rows
    sr._group_rows = lambda seg, noise: (calls.append(seg.shape[0]), inner(seg, noise))[1]
    sr.enhance_file(inputs["wav48"][0], None, False, 'all')                   # the capture
    capture = sr._g['graph']
    W = _windows(sr, 2)[1]
    for name, frames, rate in (("wav48", 6000, 48000), ("wav44", 5513, 44100)):
        path, is_lr = inputs[name]
        plan = stream_plan(frames, rate, 8000, 48000, is_lr, sr.T, sr.overlap, 2, BATCH, W)
        del calls[:]
        _count(reset=True)
        res = sr.enhance_file(path, str(tmp_path / (name + ".wav")), is_lr, 'all', stream_seconds=W)
        planned = sum(-(-2 * (w['s1'] - w['s0']) // BATCH) for w in plan['windows'])
        assert calls == [BATCH] * planned and res['stream']['groups'] == planned and res['stream']['windows'] == len(plan['windows']) > 1
        assert _count() == 2 * len(plan['windows'])                         # a gather and a stitch per window
        assert sr._g['graph'] is capture
    # the option off: the file's two launches, no key more, the same bytes as without the keyword
    _count(reset=True)
    off = sr.enhance_file(inputs["wav48"][0], str(tmp_path / "off.wav"), False, 'all', stream_seconds=None)
    assert _count() == 2 and 'stream' not in off and off['sr'] is not None
    sr.enhance_file(inputs["wav48"][0], str(tmp_path / "plain.wav"), False, 'all')
    assert _bytes(tmp_path / "off.wav") == _bytes(tmp_path / "plain.wav") == _bytes(tmp_path / "wav48.wav")


def test_memory_is_the_windows_not_the_files(tmp_path):
    """The same window over a clip of 4 windows and one of 16: the peak of allocated device memory over the long run is no larger
    than over the short one, and the pinned buffers of the object are the same size after both."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    sr = SuperResolver(PassThroughRows(model), opt, overlap=0.25, batch=BATCH, segment_norm=True)
    stride = sr.T - int(0.25 * sr.T)
    K = 2
    W = K * stride / 48000.0
    x = np.tile(_ints(12000)[:1], (1, 3))
    paths = {}
    for windows in (4, 16):
        frames = (windows * K - 1) * stride + sr.T - 7                      # the last window is a full one too, but for 7 samples
        paths[windows] = str(tmp_path / ("in%d.wav" % windows))
        WC.write_pcm16_wav(paths[windows], x[:, :frames], 48000)
    peaks, pinned = {}, {}
    sr.enhance_file(paths[4], str(tmp_path / "warm.wav"), stream_seconds=W)
    for windows in (4, 16):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        res = sr.enhance_file(paths[windows], str(tmp_path / ("out%d.wav" % windows)), stream_seconds=W)
        torch.cuda.synchronize()
        assert res['stream']['windows'] == windows and res['stream']['segments_per_window'] == K
        del res
        peaks[windows] = torch.cuda.max_memory_allocated()
        pinned[windows] = sum(t.numel() for t, _ in sr._pins.values())
    print("peak allocated: %d bytes over 4 windows, %d over 16; pinned %d and %d" % (peaks[4], peaks[16], pinned[4], pinned[16]))
    assert peaks[16] <= peaks[4]
    assert pinned[16] == pinned[4]


# ------------------------------------------------------------------------------------------
# file handling, the folder, the command line
# ------------------------------------------------------------------------------------------
def test_a_failing_window_leaves_no_file(inputs, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    sr = SuperResolver(PassThroughRows(model), opt, overlap=0.25, batch=BATCH, segment_norm=True)
    calls = []
    inner = sr._group_rows

    def group(seg, noise):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("window 2")
        return inner(seg, noise)

    sr._group_rows = group
    out = tmp_path / "out"
    with pytest.raises(RuntimeError, match="window 2"):
        sr.enhance_file(inputs["wav48"][0], str(out / "never.wav"), channels='all', stream_seconds=1e-6)
    torch.cuda.synchronize()
    assert os.listdir(out) == []
    sr._group_rows = inner
    sr.enhance_file(inputs["wav48"][0], str(out / "now.wav"), channels='all', stream_seconds=1e-6)
    assert os.listdir(out) == ["now.wav"]


def test_a_folder_streams_file_by_file_and_skips_a_flac(inputs, tmp_path):
    import shutil
    from pix2pixhdaudiosr_amd.data import flacio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    sr = SuperResolver(PassThroughRows(model), opt, overlap=0.25, batch=BATCH, segment_norm=True)
    d = tmp_path / "in"
    d.mkdir()
    shutil.copy(inputs["wav48"][0], d / "a.wav")
    flacio.save(str(d / "b.flac"), torch.from_numpy(_ints(3000).astype(np.float32) / 32768.0), 48000)
    WC.write_pcm16_wav(str(d / "c.wav"), _ints(4100)[:1], 48000)
    kw = dict(channels='all', input_formats=('wav', 'flac'), dither='tpdf', dither_seed=5)
    plain = sr.enhance_folder(str(d), str(tmp_path / "plain"), **kw)
    seen = []
    recs = sr.enhance_folder(str(d), str(tmp_path / "streamed"), stream_seconds=_windows(sr, 2)[1], report=seen.append, **kw)
    assert [r['path'] for r in recs] == ["a.wav", "b.flac", "c.wav"] and seen == recs
    assert recs[1]['error'] is not None and "FLAC input is not streamed" in recs[1]['error'] and recs[1]['stream'] is None
    assert not os.path.exists(tmp_path / "streamed" / "b.wav") and plain[1]['error'] is None
    for i, name in ((0, "a.wav"), (2, "c.wav")):
        r, p = recs[i], plain[i]
        assert r['error'] is None and _bytes(tmp_path / "streamed" / name) == _bytes(tmp_path / "plain" / name)
        assert set(r) == set(p) | {'stream'}
        assert (r['rate'], r['channels'], r['frames'], r['written_channels'], r['out_frames']) == (p['rate'], p['channels'], p['frames'],
                                                                                                  p['written_channels'], p['out_frames'])
        assert torch.equal(r['norm'], p['norm']) and r['stream']['windows'] > 1 and r['metrics'] is None


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
    base = ["--input", clip, "--load_pretrain", str(run), "--segment_norm"]
    capsys.readouterr()
    assert main(base + ["--output", str(tmp_path / "p.wav")]) == 0
    plain = capsys.readouterr().out
    assert 'streaming' not in plain
    _count(reset=True)
    assert main(base + ["--output", str(tmp_path / "s.wav"), "--stream_seconds", "0.03"]) == 0
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith('streaming: windows of ')]
    figures = ('MSE:', 'SNR_SR:', 'SNR_LR:', 'LSD:')                  # (a streamed file is compared with nothing: no metrics lines)
    assert lines == ['streaming: windows of 2 segments (0.031 s)'] and any(ln.startswith(figures) for ln in plain.splitlines())
    assert len(out.splitlines()) == len([ln for ln in plain.splitlines() if not ln.startswith(figures)]) + 1
    # one written channel, one seed: the windows' groups are the clip's, drawn in the same order
    assert _bytes(tmp_path / "s.wav") == _bytes(tmp_path / "p.wav") and _count() == 2 * 4
    with pytest.raises(SystemExit):
        main(["--input", clip, "--load_pretrain", str(run), "--output", str(tmp_path / "never.wav"), "--stream_seconds", "1"])
    assert "needs segment_norm" in capsys.readouterr().err and not os.path.exists(tmp_path / "never.wav")
