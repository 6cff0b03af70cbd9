"""Whole-file generation over channels, encodings and folders (pix2pixhdaudiosr_amd/generate.py): a channel is a clip of its
own, bit for bit; a multi-channel file is the mono files of its channels side by side, byte for byte; a folder run is the
single-file runs of its files, from one captured graph."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_generate import CONV_FAMILIES, _clip, _noise, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _data(path):
    """The data chunk of a wav written by this package (44-byte header)."""
    from pix2pixhdaudiosr_amd.data import wavio
    meta = wavio.info(path)
    with open(path, "rb") as f:
        f.seek(meta.data_offset)
        return f.read(meta.num_frames * meta.block_align), meta


# ------------------------------------------------------------------------------------------
# 7. a channel is a clip of its own
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
@pytest.mark.parametrize("overlap", [0, 0.25])
@pytest.mark.parametrize("graph", [False, True])
def test_channel_invariant(mdct_type, overlap, graph):
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    model, opt = _tiny(mdct_type)
    _, stride, V = segment_plan(1, opt.segment_length, overlap)
    L = 4 * stride + V + 100                                      # 5 segments: groups of 2, 2 and a partial one, per channel
    C = 3
    S = segment_plan(L, opt.segment_length, overlap)[0]
    assert S == 5
    x = torch.stack([0.5 * _clip(L, 1000 * c) for c in range(C)]).to(DEV)
    x[1] = -0.25 * x[1]                                           # channels of different ranges: a shared min / max would show
    sr = SuperResolver(model, opt, overlap=overlap, graph=graph)
    noise = _noise(sr, C * S, 21)
    got = sr.enhance_lr(x, noise=noise)
    assert tuple(got.shape) == (C, L) and torch.isfinite(got).all()
    for c in range(C):
        alone = sr.enhance_lr(x[c:c + 1], noise=noise[c * S:(c + 1) * S])
        assert tuple(alone.shape) == (1, L) and alone.abs().max() > 0
        assert torch.equal(got[c], alone[0]), (c,)
    assert not torch.equal(got[0], got[2])
    if graph:
        assert sr._g is not None and sr._g['graph'] is not None
    # equal channels in, equal channels out (the same noise rows for each)
    same = x[:1].repeat(C, 1)
    out = sr.enhance_lr(same, noise=noise[:S].repeat(C, 1, 1, 1))
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2]) and torch.equal(out[0], got[0])


def test_stitch_count_does_not_depend_on_channels():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct2")
    sr = SuperResolver(model, opt, overlap=0.25, graph=False)
    lib = _lib.lib()
    for C in (1, 3):
        x = torch.randn(C, 3 * opt.segment_length + 5, device=DEV) * 0.1
        lib.p2phd_launch_count(b"stitch", 1)
        sr.enhance_lr(x)
        assert lib.p2phd_launch_count(b"stitch", 1) == 2
    with pytest.raises(ValueError):
        sr.enhance_lr(torch.zeros(1, 2, 100, device=DEV))


# ------------------------------------------------------------------------------------------
# 8. files
# ------------------------------------------------------------------------------------------
def test_multichannel_files(tmp_path):
    """No random draw inside the chain (mask off): a channel's result does not depend on what ran before it."""
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4", mask=False)
    sr = SuperResolver(model, opt)
    assert sr.noise_shape(2) is None
    lib = _lib.lib()
    n = 5 * opt.segment_length // 2 + 17
    chans = torch.stack([_clip(n, 0), -0.5 * _clip(n, 5000), 0.25 * _clip(n, 9000)])
    for name, C, enc_in in (("stereo", 2, "pcm16"), ("three", 3, "pcm24")):
        src = str(tmp_path / f"{name}.wav")
        wavio.save(src, chans[:C], 48000, encoding=enc_in)
        assert wavio.info(src).num_channels == C and wavio.info(src).bits_per_sample == (16 if enc_in == "pcm16" else 24)
        out = str(tmp_path / f"{name}_sr.wav")
        lib.p2phd_launch_count(b"pcm", 1)
        res = sr.enhance_file(src, out, channels='all')
        assert lib.p2phd_launch_count(b"pcm", 1) == 2             # one decode, one encode
        data, meta = _data(out)
        assert (meta.num_channels, meta.num_frames, meta.sample_rate, meta.bits_per_sample) == (C, n, 48000, 16)
        assert tuple(res['sr'].shape) == (C, n) == tuple(res['lr'].shape) == tuple(res['hr'].shape)
        assert isinstance(res['metrics'], list) and len(res['metrics']) == C
        frames = np.frombuffer(data, dtype="<i2").reshape(n, C)
        for c in range(C):
            mono = str(tmp_path / f"{name}_{c}.wav")
            wavio.save(mono, wavio.load(src)[0][c:c + 1], 48000, encoding=enc_in)       # the file that holds channel c
            mono_out = str(tmp_path / f"{name}_{c}_sr.wav")
            one = sr.enhance_file(mono, mono_out)
            assert frames[:, c].tobytes() == _data(mono_out)[0], (name, c)
            assert len(one['metrics']) == 7 and tuple(res['metrics'][c]) == tuple(one['metrics'])
        assert len({frames[:, c].tobytes() for c in range(C)}) == C
    # 'first' (the default) on the stereo file: the mono file of channel 0, and the old return structure
    src = str(tmp_path / "stereo.wav")
    first = sr.enhance_file(src, str(tmp_path / "first.wav"))
    assert _data(str(tmp_path / "first.wav"))[0] == _data(str(tmp_path / "stereo_0_sr.wav"))[0]
    assert open(str(tmp_path / "first.wav"), "rb").read() == open(str(tmp_path / "stereo_0_sr.wav"), "rb").read()
    assert tuple(first['sr'].shape) == (1, n) and isinstance(first['metrics'], tuple) and len(first['metrics']) == 7
    # ... which is what the host codec gives: wavio.load -> enhance_lr -> wavio.save, the path before the device codec
    from pix2pixhdaudiosr_amd.data.audio_dataset import lr_round_trip
    raw = wavio.load(src)[0][:1].to(DEV)
    lr = lr_round_trip(raw, 48000, opt.lr_sampling_rate, opt.hr_sampling_rate)[..., :n]
    wavio.save(str(tmp_path / "host.wav"), sr.enhance_lr(lr), 48000)
    assert open(str(tmp_path / "host.wav"), "rb").read() == open(str(tmp_path / "first.wav"), "rb").read()
    # an int: the first N channels, all of them where the file has fewer
    two = sr.enhance_file(str(tmp_path / "three.wav"), str(tmp_path / "two.wav"), channels=2)
    assert wavio.info(str(tmp_path / "two.wav")).num_channels == 2 and len(two['metrics']) == 2
    assert torch.equal(two['sr'], sr.enhance_file(str(tmp_path / "three.wav"), channels='all')['sr'][:2])
    assert sr.enhance_file(src, channels=5)['sr'].shape[0] == 2
    # float32 output: the samples themselves; pcm24: the restated quantiser on them
    f32 = str(tmp_path / "f32.wav")
    res = sr.enhance_file(src, f32, channels='all', encoding='float32')
    meta = wavio.info(f32)
    assert (meta.format_tag, meta.bits_per_sample, meta.block_align, meta.num_channels) == (3, 32, 8, 2)
    assert torch.equal(wavio.load(f32)[0], res['sr'].cpu())
    import _pcm_ref as P
    p24 = str(tmp_path / "p24.wav")
    res24 = sr.enhance_file(src, p24, channels='all', encoding='pcm24')
    assert torch.equal(res24['sr'], res['sr']) and _data(p24)[0] == P.encode(res['sr'].cpu().numpy(), "pcm24")
    assert _data(p24)[1].bits_per_sample == 24
    with pytest.raises(ValueError, match="encoding"):
        sr.enhance_file(src, f32, encoding='pcm8')
    with pytest.raises(ValueError, match="channels"):
        sr.enhance_file(src, f32, channels='both')


# ------------------------------------------------------------------------------------------
# 9. a folder, through the API and the command line
# ------------------------------------------------------------------------------------------
def _conv_launches(reset=1):
    from pix2pixhdaudiosr_amd import _lib
    return sum(_lib.lib().p2phd_launch_count(f, reset) for f in CONV_FAMILIES)


def _tree(tmp_path, T):
    """mono, stereo, a nested 3-channel file and one whose header is cut short; every good file has full groups of 2."""
    from pix2pixhdaudiosr_amd.data import wavio
    src = tmp_path / "in"
    (src / "sub" / "deep").mkdir(parents=True)
    n = 3 * (T - T // 4) + T - 200                               # 4 segments at the default overlap of 0.25
    wavio.save(str(src / "a_mono.wav"), _clip(n, 0), 48000)
    wavio.save(str(src / "b_stereo.wav"), torch.stack([_clip(n + 50, 2000), -0.5 * _clip(n + 50, 7000)]), 48000)
    wavio.save(str(src / "sub" / "deep" / "c.wav"), torch.stack([0.5 * _clip(n, 100), _clip(n, 300), 0.1 * _clip(n, 500)]), 48000,
               encoding="pcm24")
    good = open(str(src / "a_mono.wav"), "rb").read()
    (src / "sub" / "bad.wav").write_bytes(good[:30])              # ends inside the fmt chunk
    (src / "notes.txt").write_text("not audio")
    return src, ["a_mono.wav", "b_stereo.wav", os.path.join("sub", "deep", "c.wav")], os.path.join("sub", "bad.wav")


def _checkpoint(tmp_path, **kw):
    from test_gpu_model import make_opt
    from pix2pixhdaudiosr_amd.generate import opt_from_file
    from pix2pixhdaudiosr_amd.models.models import create_model
    common = dict(mdct_type="mdct4", segment_length=127 * 32, batchSize=2, checkpoints_dir=str(tmp_path), name="run", seed=1234, **kw)
    torch.manual_seed(1234)
    create_model(make_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:                      # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(make_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    opt = opt_from_file(str(folder / "opt.txt"))
    model = create_model(opt)
    model.eval()
    return folder, model, opt


def test_folder_and_cli(tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    folder, model, opt = _checkpoint(tmp_path)                    # mask on: the noise is drawn, every file starts from the seed
    src, good, bad = _tree(tmp_path, opt.segment_length)
    # single-file runs, each from the seed
    single = tmp_path / "single"
    single.mkdir()
    one = SuperResolver(model, opt)
    want_metrics = {}
    for rel in good:
        torch.manual_seed(opt.seed)
        res = one.enhance_file(str(src / rel), str(single / rel.replace(os.sep, "_")), channels='all')
        want_metrics[rel] = res['metrics']
    # the folder through the API: one capture serves the run
    sr = SuperResolver(model, opt)
    seen = []
    _conv_launches()
    records = sr.enhance_folder(str(src), str(tmp_path / "out_api"), channels='all', seed=opt.seed, report=seen.append)
    assert [r['path'] for r in records] == sorted(good + [bad]) and seen == records
    by = {r['path']: r for r in records}
    assert by[bad]['error'] is not None and by[bad]['metrics'] is None and by[bad]['written_channels'] == 0
    assert not os.path.exists(str(tmp_path / "out_api" / bad))
    for rel, C in zip(good, (1, 2, 3)):
        r = by[rel]
        meta = wavio.info(str(src / rel))
        assert r['error'] is None and (r['rate'], r['channels'], r['frames']) == (48000, C, meta.num_frames)
        assert (r['written_channels'], r['out_frames']) == (C, meta.num_frames)
        assert [tuple(m) for m in r['metrics']] == [tuple(m) for m in want_metrics[rel]]
        assert open(str(tmp_path / "out_api" / rel), "rb").read() == open(str(single / rel.replace(os.sep, "_")), "rb").read()
    _conv_launches()
    again = sr.enhance_folder(str(src), str(tmp_path / "out_api2"), channels='all', seed=opt.seed)
    assert _conv_launches() == 0                                  # every group of the files is full: replays only
    assert [r['metrics'] for r in again] == [r['metrics'] for r in records]
    # a fresh resolver: the first full group runs eagerly once and is captured; every later one of the whole folder replays
    fresh = SuperResolver(model, opt)
    _conv_launches()
    fresh.enhance_file(str(src / good[0]), None)
    per_capture = _conv_launches()
    assert per_capture > 0
    fresh2 = SuperResolver(model, opt)
    fresh2.enhance_folder(str(src), str(tmp_path / "out_api3"), channels='all', seed=opt.seed)
    assert _conv_launches() == per_capture                        # 12 full groups in the folder, launches of the first only

    # the command line, in a process of its own
    env = dict(os.environ, PYTHONPATH=ROOT)
    out_cli = tmp_path / "out_cli"
    csv_path = str(tmp_path / "m.csv")
    p = subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.generate", "--input", str(src), "--output", str(out_cli),
                        "--load_pretrain", str(folder), "--channels", "all", "--metrics_csv", csv_path],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert ("skipped %s" % bad) in p.stdout and "3 of 4 files enhanced, 1 skipped" in p.stdout
    found = sorted(os.path.relpath(os.path.join(d, f), str(out_cli)) for d, _, fs in os.walk(str(out_cli)) for f in fs)
    assert found == sorted(good)
    for rel in good:
        assert open(str(out_cli / rel), "rb").read() == open(str(single / rel.replace(os.sep, "_")), "rb").read(), rel
    with open(csv_path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["file", "channel", "frames", "mse", "snr_sr", "snr_lr", "lsd"]
    assert [(r[0], r[1]) for r in rows[1:]] == [(good[0], "0"), (good[1], "0"), (good[1], "1"), (good[2], "0"), (good[2], "1"),
                                                (good[2], "2"), ("mean", "")]
    body = [[float(v) for v in r[3:]] for r in rows[1:]]
    for k in range(4):
        assert body[-1][k] == sum(r[k] for r in body[:-1]) / 6
    flat = [m for rel in good for m in want_metrics[rel]]
    assert [tuple(b) for b in body[:-1]] == [(m[0], m[1], m[2], m[6]) for m in flat]
    # the default --channels first on the folder: one channel each, a line that names --channels all for the others
    out_first = tmp_path / "out_first"
    p = subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.generate", "--input", str(src), "--output", str(out_first),
                        "--load_pretrain", str(folder), "--encoding", "pcm24"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if "--channels all" in l]
    assert len(lines) == 2 and good[1] in lines[0] and good[2] in lines[1]
    for rel in good:
        meta = wavio.info(str(out_first / rel))
        assert (meta.num_channels, meta.bits_per_sample, meta.num_frames) == (1, 24, wavio.info(str(src / rel)).num_frames)
    # a file and a directory do not mix
    p = subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.generate", "--input", str(src), "--output", str(src / good[0]),
                        "--load_pretrain", str(folder)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "directory" in p.stderr
