"""stream_seconds without a GPU: the plan (plans.stream_plan), the windowed resampler and the stitch with a carry against their
restatements (tests/_stream_ref.py, tests/_generate_ref.py), the flow of generate/stream.py on a SuperResolver built without a
device, its launches replaced by the restatements, and every refusal of plans.check_stream, of the two entry points and of the
command line before a file is opened."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _generate_ref as G
import _stream_ref as SR

CHAINS = [(48000, 8000, 48000, False), (44100, 8000, 48000, False), (8000, 8000, 48000, True)]


# ------------------------------------------------------------------------------------------
# the plan
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_rate,lr,hr,is_lr", CHAINS)
@pytest.mark.parametrize("C,batch", [(1, 1), (1, 4), (2, 4), (3, 4), (2, 5)])
@pytest.mark.parametrize("W", [1e-6, 0.004, 0.011, 1e6])
def test_stream_plan(in_rate, lr, hr, is_lr, C, batch, W):
    from pix2pixhdaudiosr_amd.generate import segment_plan, stream_plan
    T, overlap = 64, 0.25
    for frames in (0, 1, 63, 64, 1000, 1237):
        p = stream_plan(frames, in_rate, lr, hr, is_lr, T, overlap, C, batch, W)
        want_L = len(SR.round_trip(np.zeros(frames, dtype=np.int64), in_rate, lr, hr, is_lr))
        S, stride, V = segment_plan(want_L, T, overlap)
        assert (p['L'], p['S'], p['stride'], p['V']) == (want_L, S, stride, V)
        K, wins = p['K'], p['windows']
        unit = batch // math.gcd(batch, C)
        assert K >= 1 and (C * K) % batch == 0 and K == -(-max(1, math.floor(W * hr / stride + 0.5)) // unit) * unit
        assert [w['s0'] for w in wins] == list(range(0, S, K)) and [w['s1'] for w in wins] == [min(S, s + K) for s in range(0, S, K)]
        assert all((C * (w['s1'] - w['s0'])) % batch == 0 for w in wins[:-1])            # only the last window has filler rows
        at = 0
        for w in wins:                                                                  # the emitted ranges partition [0, L) in order
            assert w['emit'][0] == at and w['emit'][1] >= at
            at = w['emit'][1]
            assert w['need'] == (min(w['s0'] * stride, want_L), min((w['s1'] - 1) * stride + T, want_L))
            assert w['need'][0] <= w['emit'][0] and w['emit'][1] <= max(w['need'][1], w['emit'][0])
            assert 0 <= w['read'][0] <= w['read'][1] <= frames
        assert at == want_L
        if W == 1e-6:
            assert K == batch // math.gcd(batch, C)
        if W == 1e6:
            assert len(wins) == 1 and wins[0]['read'] == (0, frames)


def test_resample_geometry_is_the_librarys():
    import ctypes
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import resample_geometry, resample_out_len
    L = _lib.lib()
    for a, b in ((48000, 8000), (8000, 48000), (44100, 8000), (44100, 48000), (16000, 48000), (22050, 16000), (48000, 44100)):
        got = [ctypes.c_int() for _ in range(4)]
        assert L.p2phd_resample_geometry(a, b, 6, 0.99, *[ctypes.byref(g) for g in got]) == 0
        assert tuple(g.value for g in got) == resample_geometry(a, b) == SR.geometry(a, b)
        for T in (0, 1, 5, 441, 48001):
            assert L.p2phd_resample_out_len(T, a, b) == resample_out_len(T, a, b) == SR.out_len(T, a, b)


# ------------------------------------------------------------------------------------------
# the windowed resampler: integer samples, an integer table, exact
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_rate,lr,hr,is_lr", CHAINS)
@pytest.mark.parametrize("W", [1e-6, 0.003, 0.02])
def test_windows_with_their_halo_are_the_whole_round_trip(in_rate, lr, hr, is_lr, W):
    """Lengths that end inside a polyphase block and on one; windows of one segment -- the halo of the first and the last reaches
    the ends of the file, and with a clip this short those of the inner ones do too -- and of several."""
    from pix2pixhdaudiosr_amd.generate import stream_plan
    T, overlap = 32, 0.25
    o = SR.geometry(in_rate, lr if not is_lr else hr)[0]
    for frames in (1, o, 2 * o + 1, 997, 1200 if in_rate != 44100 else 4 * 441 + 17):
        x = np.random.default_rng(frames).integers(-2000, 2000, size=frames).astype(np.int64)
        whole = SR.round_trip(x, in_rate, lr, hr, is_lr)
        p = stream_plan(frames, in_rate, lr, hr, is_lr, T, overlap, 1, 1, W)
        assert p['L'] == len(whole)
        for w in p['windows']:
            got = SR.round_trip_window(x, p, w)
            a, b = w['need']
            assert np.array_equal(got, whole[a:b]), (frames, w)
        if W == 0.02 and frames > 900:
            assert 1 < len(p['windows']) < p['S']


# ------------------------------------------------------------------------------------------
# the stitch with a carry
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,stride", [(8, 8), (8, 6), (8, 4), (10, 7), (64, 48)])
def test_stitch_with_a_carry_is_the_whole_stitch(T, stride):
    S = 7
    seg = np.random.default_rng(T + stride).standard_normal((S, T))
    for L in ((S - 1) * stride + 1, (S - 1) * stride + T):
        want = G.stitch(seg, stride, 0.75, L)
        for K in (1, 2, S):
            parts, carry = [], None
            for s0 in range(0, S, K):
                Kw = min(K, S - s0)
                last = s0 + Kw == S
                out, carry = SR.stitch_stream(seg[s0:s0 + Kw], stride, 0.75, carry, (L - s0 * stride) if last else Kw * stride, last)
                parts.append(out)
            assert np.array_equal(np.concatenate(parts), want), (T, stride, L, K)


# ------------------------------------------------------------------------------------------
# the flow, on an object built without a device
# ------------------------------------------------------------------------------------------
def _encode(w, first_index):
    """The stand-in encoder: the value and its index in the file, so that a wrong first_index shows."""
    C, n = w.shape
    flat = np.ascontiguousarray(w.T).reshape(-1)
    return (flat + np.arange(first_index, first_index + C * n, dtype=np.float64)).astype('<f4').tobytes()


def _bare(monkeypatch, batch=4, T=32, overlap=0.25, segment_norm=True):
    from pix2pixhdaudiosr_amd.data import audio_dataset
    from pix2pixhdaudiosr_amd.generate import SuperResolver, stream
    sr = SuperResolver.__new__(SuperResolver)
    sr.device, sr.batch, sr.T, sr.graph, sr.segment_norm, sr.overlap = torch.device('cpu'), batch, T, False, segment_norm, overlap
    sr.crossover_plan, sr.gain, sr._pins = None, 1.5, {}
    sr.opt = SimpleNamespace(hr_sampling_rate=48000, lr_sampling_rate=8000)
    sr.model = SimpleNamespace(mask_noise_shape=None)
    sr.calls, sr.reads = [], []

    def group(seg, noise):
        sr.calls.append(seg.clone())
        ranges = torch.zeros((seg.shape[0], 8), dtype=torch.float64)
        ranges[:, 0], ranges[:, 1] = seg[:, 0], seg.sum(dim=1)
        return 2 * seg, ranges

    def pinned(slot, n):
        t = sr._pins.get(slot, (None, None))[0]
        if t is None or t.numel() < n:
            t = torch.empty((max(int(n), 1),), dtype=torch.uint8)
        sr._pins[slot] = (t, None)
        return t

    def decode(host, meta, slot):
        sr.reads.append((slot, meta.num_frames))
        a = np.frombuffer(host.numpy().tobytes(), dtype='<i2').astype(np.float64).reshape(-1, meta.num_channels).T
        return torch.from_numpy(np.ascontiguousarray(a))

    sr._group_rows, sr._pinned, sr._decode = group, pinned, decode
    sr._stream_event = lambda: SimpleNamespace(synchronize=lambda: None)
    monkeypatch.setattr(audio_dataset, "resample", lambda x, a, b: torch.from_numpy(np.stack(
        [SR.resample(r.astype(np.int64), int(a), int(b), SR.table(int(a), int(b))) for r in x.numpy()]).astype(np.float64)))
    monkeypatch.setattr(stream, "segments_gather_planar", lambda x, T, stride, S: torch.from_numpy(
        np.concatenate([G.gather(row, T, stride, S) for row in x.numpy()])))

    def stitch(seg, C, stride, gain, carry_in=None, carry_out=None, first=False, out_length=None):
        K = seg.shape[0] // C
        rows = []
        for c in range(C):
            out, carry = SR.stitch_stream(seg.numpy()[c * K:(c + 1) * K], stride, gain, None if first else carry_in[c].numpy(), out_length, True)
            rows.append(out)
            if carry_out is not None:
                carry_out[c].copy_(torch.from_numpy(carry))
        return torch.from_numpy(np.stack(rows))

    monkeypatch.setattr(stream, "segments_stitch_stream", stitch)
    monkeypatch.setattr(stream, "pcm_encode", lambda w, encoding, first_index=0: torch.from_numpy(
        np.frombuffer(_encode(w.numpy(), first_index), dtype=np.uint8).copy()))
    return sr


@pytest.mark.parametrize("C,batch,W", [(1, 4, 1e-6), (2, 4, 0.002), (2, 3, 0.004), (1, 1, 1e6)])
@pytest.mark.parametrize("in_rate,is_lr", [(48000, False), (44100, False), (8000, True)])
def test_the_flow_writes_the_whole_file_payload(monkeypatch, tmp_path, C, batch, W, in_rate, is_lr):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import stream_plan
    from pix2pixhdaudiosr_amd.generate.resolver import _Options
    sr = _bare(monkeypatch, batch)
    frames = 700 if in_rate != 8000 else 130
    x = np.random.default_rng(C + frames).integers(-3000, 3000, size=(2, frames)).astype(np.int64)
    wavio.save(str(tmp_path / "in.wav"), torch.from_numpy(x.astype(np.float32) / 32768.0), in_rate)
    res = sr._enhance_stream(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), is_lr, 'all' if C == 2 else 'first', 'float32',
                             _Options(None, None, None, None, None, None, None, None, None, None), W)
    plan = stream_plan(frames, in_rate, 8000, 48000, is_lr, sr.T, sr.overlap, C, batch, W)
    # the whole file, in one piece
    lr = np.stack([SR.round_trip(x[c], in_rate, 8000, 48000, is_lr) for c in range(C)]).astype(np.float64)
    S, stride, V = G.plan(lr.shape[1], sr.T, sr.overlap)
    assert (S, stride, lr.shape[1]) == (plan['S'], plan['stride'], plan['L'])
    whole = np.stack([G.stitch(2.0 * G.gather(lr[c], sr.T, stride, S), stride, sr.gain, lr.shape[1]) for c in range(C)])
    want = _encode(whole, 0)
    with open(tmp_path / "out.wav", "rb") as f:
        got = f.read()
    wavio.write_payload(str(tmp_path / "whole.wav"), want, 48000, C, 'float32')
    with open(tmp_path / "whole.wav", "rb") as f:
        assert got == f.read() and got[44:] == want
    os.remove(tmp_path / "whole.wav")
    # the group function ran the planned number of times, on full groups
    groups = sum(math.ceil(C * (w['s1'] - w['s0']) / batch) for w in plan['windows'])
    assert len(sr.calls) == groups == res['stream']['groups'] and all(tuple(g.shape) == (batch, sr.T) for g in sr.calls)
    assert res['stream'] == {'windows': len(plan['windows']), 'segments_per_window': plan['K'], 'groups': groups, 'frames': frames,
                             'out_frames': lr.shape[1], 'window_seconds': plan['K'] * stride / 48000.0}
    assert [n for _, n in sr.reads] == [w['read'][1] - w['read'][0] for w in plan['windows']]
    assert [s for s, _ in sr.reads] == ['stream%d' % (i % 2) for i in range(len(plan['windows']))]
    assert res['sr'] is None and res['lr'] is None and res['hr'] is None and res['metrics'] is None and res['info'].num_frames == frames
    first = torch.stack([torch.from_numpy(G.gather(lr[c], sr.T, stride, S)) for c in range(C)])
    assert tuple(res['norm'].shape) == (C, S, 2) and torch.equal(res['norm'][..., 0], first[..., 0].float()) and res['norm'] is sr.last_norm
    assert sorted(os.listdir(tmp_path)) == ["in.wav", "out.wav"]
    if W == 1e6:
        assert len(plan['windows']) == 1
    else:
        assert len(plan['windows']) > 2


def test_a_failing_window_leaves_no_file(monkeypatch, tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate.resolver import _Options
    sr = _bare(monkeypatch, 1)
    wavio.save(str(tmp_path / "in.wav"), torch.zeros(1, 700), 48000)
    inner = sr._group_rows

    def group(seg, noise):
        if len(sr.calls) == 2:
            raise RuntimeError("window 2")
        return inner(seg, noise)

    sr._group_rows = group
    with pytest.raises(RuntimeError, match="window 2"):
        sr._enhance_stream(str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), False, 'first', 'float32',
                           _Options(None, None, None, None, None, None, None, None, None, None), 1e-6)
    assert os.listdir(tmp_path) == ["in.wav"]


# ------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------
REFUSED = [(dict(loudness='report'), "loudness"), (dict(speech_level='report'), "speech_level"), (dict(clip='guard'), "clip='guard'"),
           (dict(clip='error'), "clip='error'"), (dict(true_peak=True), "true_peak"), (dict(clip='guard', limiter=True), "clip='guard'"),
           (dict(report_peaks=True), "report_peaks"), (dict(spectrogram="p.png"), "spectrogram"), (dict(bandwidth=True), "bandwidth"),
           (dict(stereo_report=True), "stereo_report"), (dict(output_rate=44100), "output_rate"), (dict(extended_metrics=True), "extended_metrics"),
           (dict(container='flac'), "container='flac'"), (dict(dither='shaped'), "dither='shaped'")]


def test_check_stream():
    from pix2pixhdaudiosr_amd.generate import check_stream
    assert check_stream(None) is None and check_stream(None, "x", False, 'input', loudness=-23.0, pack_files=4) is None     # off: nothing is looked at
    assert check_stream(2, "enhance_file", True) == 2.0 and check_stream(0.5, "enhance_file", True, dither='tpdf', output_rate=48000, hr_rate=48000) == 0.5
    for bad in (0, -1.0, float('inf'), float('nan'), True, '5', [1]):
        with pytest.raises(ValueError, match=r"^enhance_file: stream_seconds must be a finite number above 0"):
            check_stream(bad, "enhance_file", True)
    with pytest.raises(ValueError, match=r"^generate: stream_seconds .* needs segment_norm"):
        check_stream(1.0, "generate", False)
    with pytest.raises(ValueError, match=r"^enhance_file: stream_seconds is not built with the crossover"):
        check_stream(1.0, "enhance_file", True, 'input')
    for kw, word in REFUSED + [(dict(limiter=True), "limiter"), (dict(pack_files=2), "pack_files > 1"), (dict(loudness_scope='folder'), "loudness_scope='folder'")]:
        with pytest.raises(ValueError, match=r"^enhance_folder: stream_seconds is not built with " + word.replace("(", r"\(")):
            check_stream(1.0, "enhance_folder", True, **kw)


def test_both_entry_points_refuse_before_a_file_is_opened(monkeypatch, tmp_path):
    opened = []
    cases = [(kw, True, None, "stream_seconds is not built with " + word) for kw, word in REFUSED]
    cases += [({}, False, None, "needs segment_norm"), ({}, True, 'input', "not built with the crossover"), (dict(stream_seconds=0), True, None, "finite number above 0")]
    for kw, segment_norm, crossover, word in cases:
        for entry, target in (("enhance_file", "no_such.wav"), ("enhance_folder", "no_such_folder")):
            sr = _bare(monkeypatch, segment_norm=segment_norm)
            sr.crossover, sr.stereo = crossover, 'lr'
            sr._read = sr._stream_info = lambda *a, **k: opened.append(a)
            with pytest.raises(ValueError, match=word.replace("(", r"\(")):
                getattr(sr, entry)(str(tmp_path / target), str(tmp_path / "out"), **dict(dict(stream_seconds=1.0), **kw))
    sr = _bare(monkeypatch)
    sr.crossover = None
    sr._read = sr._stream_info = lambda *a, **k: opened.append(a)
    with pytest.raises(ValueError, match=r"enhance_folder: stream_seconds is not built with pack_files > 1"):
        sr.enhance_folder(str(tmp_path / "no_such_folder"), str(tmp_path / "out"), stream_seconds=1.0, pack_files=2)
    assert not opened and not (tmp_path / "out").exists()


def test_a_coding_that_does_not_stream_names_file_and_coding(monkeypatch, tmp_path):
    sr = _bare(monkeypatch)
    flac = tmp_path / "a.flac"
    flac.write_bytes(b"fLaC" + bytes(64))
    with pytest.raises(ValueError, match=r"a\.flac: a FLAC input is not streamed"):
        sr._stream_info(str(flac))
    import struct
    ima = tmp_path / "b.wav"                                        # one block of 505 samples, mono
    fmt = struct.pack("<HHIIHHHH", 0x11, 1, 8000, 4055, 256, 4, 2, 505)
    ima.write_bytes(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + 256) + b"WAVEfmt " + struct.pack("<I", len(fmt)) + fmt
                    + b"data" + struct.pack("<I", 256) + bytes(256))
    with pytest.raises(ValueError, match=r"b\.wav: an IMA ADPCM input is not streamed"):
        sr._stream_info(str(ima))


def test_command_line(capsys, tmp_path):
    from pix2pixhdaudiosr_amd.generate import _parser, main
    (tmp_path / "in").mkdir()
    folder = ["--input", str(tmp_path / "in"), "--output", str(tmp_path / "out"), "--load_pretrain", str(tmp_path / "no_such_checkpoint")]
    single = ["--input", str(tmp_path / "a.wav"), "--output", str(tmp_path / "b.wav"), "--load_pretrain", str(tmp_path / "no_such_checkpoint")]
    assert _parser().parse_args(single).stream_seconds is None
    assert _parser().parse_args(single + ["--stream_seconds", "2.5"]).stream_seconds == 2.5
    assert "--stream_seconds" in _parser().format_help()
    on = ["--stream_seconds", "5", "--segment_norm"]
    for argv, word in ((single + ["--stream_seconds", "5"], "needs segment_norm"),
                       (single + ["--stream_seconds", "0", "--segment_norm"], "finite number above 0"),
                       (single + on + ["--crossover", "input"], "the crossover"),
                       (single + on + ["--loudness", "-23"], "loudness"),
                       (single + on + ["--speech_level", "report"], "speech_level"),
                       (single + on + ["--clip", "guard"], "clip='guard'"),
                       (single + on + ["--true_peak"], "true_peak"),
                       (single + on + ["--report_peaks"], "report_peaks"),
                       (single + on + ["--spectrogram", str(tmp_path / "p.png")], "spectrogram"),
                       (single + on + ["--bandwidth"], "bandwidth"),
                       (single + on + ["--stereo_report"], "stereo_report"),
                       (single + on + ["--output_rate", "44100"], "output_rate"),
                       (single + on + ["--metrics_ext"], "extended_metrics"),
                       (single + on + ["--container", "flac"], "container='flac'"),
                       (single + on + ["--dither", "shaped"], "dither='shaped'"),
                       (folder + on + ["--pack_files", "4"], "pack_files > 1")):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and "stream_seconds" in err and word in err, (argv, err)
    assert not (tmp_path / "out").exists() and not (tmp_path / "b.wav").exists()
