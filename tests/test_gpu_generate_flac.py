"""FLAC inputs through whole-file generation on the GPU: enhance_file on x.flac writes the bytes it writes for x.wav with the same
samples, with launches of the family "flac" in place of the PCM decoder's one and none of them for a wav; mono, stereo (mid/side
coded) and 24-bit inputs; folder mode with and without input_formats; the album flow; verify_input; the command line; a corrupt
file is a ValueError in file mode and a skipped file in folder mode.  The tiny model is that of tests/test_gpu_generate_shaped.py,
restated; the FLAC files come from the restatement tests/_flac_ref.py."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _flac_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE = 48000
NAMES = ("a_mono", "b_stereo", "c_24bit")


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


def _count(family=b"flac", reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(family, 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _ints(bits, n, flip=False, gain=0.5):
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    x = F["test_wav_excerpt_i16"].astype(np.float64) / 32768.0
    x = np.concatenate([x, 0.7 * x[::-1]])[:n]
    if flip:
        x = -0.6 * x[::-1]
    return [int(v) for v in np.clip(np.rint(gain * x * (1 << (bits - 1))), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)]


def _build_files(d):
    """Two folders with the same samples: `wav` holds three wav files, `mixed` the first as wav and the other two as FLAC."""
    from pix2pixhdaudiosr_amd.data import wavio
    wav, mixed = d / "wav", d / "mixed"
    wav.mkdir()
    mixed.mkdir()
    n = 3 * 4096 + 1234
    clips = {"a_mono": ([_ints(16, n)], 16), "b_stereo": ([_ints(16, n - 500), _ints(16, n - 500, True)], 16), "c_24bit": ([_ints(24, n - 900)], 24)}
    # three whole frames of 4096 and a short one, whose length no partition order divides
    fixed = lambda k, c: [dict(kind="fixed", order=2, porder=4 if k < 3 else 0), dict(kind="fixed", order=1, porder=2 if k < 3 else 0, method=1)][(k + c) % 2]
    for name, (chs, bits) in clips.items():
        x = torch.tensor(chs, dtype=torch.float32) / float(1 << (bits - 1))
        wavio.save(str(wav / (name + ".wav")), x, RATE, "pcm16" if bits == 16 else "pcm24")
        data, _ = R.make_stream(chs, bits, 4096, rate=RATE, assign=R.MID_SIDE if len(chs) == 2 else None, specs=fixed)
        open(str(d / (name + ".flac")), "wb").write(data)
    shutil.copy(str(wav / "a_mono.wav"), str(mixed / "a_mono.wav"))
    for name in NAMES[1:]:
        shutil.copy(str(d / (name + ".flac")), str(mixed / (name + ".flac")))
    (mixed / "notes.txt").write_text("not audio")
    return d


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return _build_files(tmp_path_factory.mktemp("flac_in"))


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    from pix2pixhdaudiosr_amd.models.models import create_model
    opt = _opt(mdct_type="mdct4")
    torch.manual_seed(1234)
    model = create_model(opt)
    model.eval()
    return SuperResolver(model, opt, crossover='input')


@pytest.mark.parametrize("name", NAMES)
def test_flac_writes_the_bytes_of_the_wav(resolver, files, tmp_path, name):
    from pix2pixhdaudiosr_amd.data import flacio, wavio
    wav, flac = str(files / "wav" / (name + ".wav")), str(files / (name + ".flac"))
    assert torch.equal(flacio.load(flac)[0], wavio.load(wav)[0])
    resolver.enhance_file(wav, None, channels='all')                # capture, tables, packed weights
    _count(reset=True)
    _count(b"pcm", reset=True)
    torch.manual_seed(5)
    a = resolver.enhance_file(wav, str(tmp_path / "w.wav"), channels='all')
    assert _count(reset=True) == 0                                  # a wav launches nothing of the family
    pcm_wav = _count(b"pcm", reset=True)
    torch.manual_seed(5)
    b = resolver.enhance_file(flac, str(tmp_path / "f.wav"), channels='all')
    assert _count(reset=True) == 2 and _count(b"pcm", reset=True) == pcm_wav - 1      # in place of the PCM decoder's launch
    assert _bytes(str(tmp_path / "f.wav")) == _bytes(str(tmp_path / "w.wav"))
    assert sorted(a) == sorted(b) and torch.equal(a['sr'], b['sr']) and torch.equal(a['lr'], b['lr']) and a['metrics'] == b['metrics']
    assert isinstance(b['info'], flacio.FlacInfo) and isinstance(a['info'], wavio.WavInfo) and b['info'][:4] == a['info'][:4]


def test_folder_mode(resolver, files, tmp_path):
    base = resolver.enhance_folder(str(files / "wav"), str(tmp_path / "w"), channels='all', seed=11)
    _count(reset=True)
    off = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "off"), channels='all', seed=11)
    assert _count() == 0 and [r['path'] for r in off] == ["a_mono.wav"] and off[0] == base[0] and 'written' not in off[0]
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["a_mono.wav"]
    on = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "on"), channels='all', seed=11, input_formats=('wav', 'flac'))
    assert _count(reset=True) == 4
    assert [r['path'] for r in on] == ["a_mono.wav", "b_stereo.flac", "c_24bit.flac"] and [r['written'] for r in on] == [n + ".wav" for n in NAMES]
    for r, w, name in zip(on, base, NAMES):
        assert r['error'] is None and {k: v for k, v in r.items() if k not in ('path', 'written')} == {k: v for k, v in w.items() if k != 'path'}
        assert _bytes(str(tmp_path / "on" / (name + ".wav"))) == _bytes(str(tmp_path / "w" / (name + ".wav")))
    clash = tmp_path / "clash"
    clash.mkdir()
    shutil.copy(str(files / "wav" / "b_stereo.wav"), str(clash / "b_stereo.wav"))
    shutil.copy(str(files / "b_stereo.flac"), str(clash / "b_stereo.flac"))
    with pytest.raises(ValueError, match="both be written"):
        resolver.enhance_folder(str(clash), str(tmp_path / "never"), input_formats='wav,flac')
    assert not os.path.exists(str(tmp_path / "never"))


def test_album_flow(resolver, files, tmp_path):
    kw = dict(channels='all', seed=11, loudness=-23.0, loudness_scope='folder', clip='guard', ceiling_dbfs=-3.0)
    base = resolver.enhance_folder(str(files / "wav"), str(tmp_path / "w"), **kw)
    _count(reset=True)
    on = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "on"), input_formats=('wav', 'flac'), **kw)
    assert _count(reset=True) == 4 and len(on) == len(base) == 3
    for r, w, name in zip(on, base, NAMES):
        assert r['error'] is None and r['album'] == w['album'] and r['loudness'] == w['loudness'] and r['output'] == w['output']
        assert r['written'] == name + ".wav" and _bytes(str(tmp_path / "on" / (name + ".wav"))) == _bytes(str(tmp_path / "w" / (name + ".wav")))
    off = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "off"), **kw)
    assert _count() == 0 and [r['path'] for r in off] == ["a_mono.wav"]


def _patched(files, tmp_path, what):
    data = bytearray(_bytes(str(files / "b_stereo.flac")))
    if what == "md5":
        data[4 + 4 + 18] ^= 1                                       # STREAMINFO's MD5: the frames still verify
    else:
        data[len(data) // 2] ^= 0x10                                # a frame's CRC-16 no longer closes
    d = tmp_path / what
    d.mkdir()
    open(str(d / "bad.flac"), "wb").write(bytes(data))
    shutil.copy(str(files / "c_24bit.flac"), str(d / "good.flac"))
    return d


def test_verify_input(resolver, files, tmp_path):
    d = _patched(files, tmp_path, "md5")
    torch.manual_seed(5)
    a = resolver.enhance_file(str(d / "bad.flac"), str(tmp_path / "a.wav"))                  # without the option the MD5 is not looked at
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "b_stereo.flac"), str(tmp_path / "b.wav"), verify_input=True)
    assert a['info'].md5 != b"\0" * 16 and _bytes(str(tmp_path / "a.wav")) == _bytes(str(tmp_path / "b.wav"))
    _count(reset=True)
    with pytest.raises(ValueError, match="bad.flac.*MD5"):
        resolver.enhance_file(str(d / "bad.flac"), str(tmp_path / "never.wav"), verify_input=True)
    assert _count() == 0 and not os.path.exists(str(tmp_path / "never.wav"))
    recs = resolver.enhance_folder(str(d), str(tmp_path / "out"), input_formats='flac', verify_input=True)
    assert [r['path'] for r in recs] == ["bad.flac", "good.flac"] and "MD5" in recs[0]['error'] and recs[1]['error'] is None
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["good.wav"]
    recs = resolver.enhance_folder(str(d), str(tmp_path / "out2"), input_formats='flac')
    assert [r['error'] for r in recs] == [None, None]


def test_corrupt_file(resolver, files, tmp_path):
    d = _patched(files, tmp_path, "crc")
    _count(reset=True)
    with pytest.raises(ValueError, match=r"bad.flac.*frame \d+ at byte \d+"):
        resolver.enhance_file(str(d / "bad.flac"), str(tmp_path / "never.wav"))
    assert _count() == 0 and not os.path.exists(str(tmp_path / "never.wav"))              # refused before anything is launched
    recs = resolver.enhance_folder(str(d), str(tmp_path / "out"), input_formats=('flac',))
    assert recs[0]['error'].startswith("ValueError") and "frame" in recs[0]['error'] and recs[1]['error'] is None
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["good.wav"]


def test_a_decoder_refusal_names_the_file(resolver, tmp_path):
    """A negative LPC shift sits in a subframe: the index passes the file, the device decoder refuses frame 1, and the error names
    the file and the frame; nothing is written."""
    ch = _ints(16, 48)
    base = dict(kind="fixed", order=2)
    neg = dict(kind="lpc", coefs=[3, -1], precision=4, shift=-1)
    frames = [R.encode_frame([ch[16 * k:16 * k + 16]], 16, k, rate=RATE, specs=[neg if k == 1 else base]) for k in range(3)]
    p = str(tmp_path / "neg.flac")
    open(p, "wb").write(R.encode_stream(frames, RATE, 1, 16, 48, 16, 16))
    with pytest.raises(ValueError, match=r"neg\.flac: flac_decode: frame 1 does not decode: a reserved code"):
        resolver.enhance_file(p, str(tmp_path / "never.wav"))
    assert not os.path.exists(str(tmp_path / "never.wav"))


def test_cli(files, tmp_path, capsys):
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
    tail = ["--load_pretrain", str(folder), "--channels", "all"]
    assert G.main(["--input", str(files / "wav" / "b_stereo.wav"), "--output", str(tmp_path / "w.wav")] + tail) == 0
    w = capsys.readouterr().out.splitlines()
    _count(reset=True)
    assert G.main(["--input", str(files / "b_stereo.flac"), "--output", str(tmp_path / "f.wav")] + tail) == 0
    f = capsys.readouterr().out.splitlines()
    assert _count(reset=True) == 2 and [l.replace("f.wav", "w.wav") for l in f] == w
    assert _bytes(str(tmp_path / "f.wav")) == _bytes(str(tmp_path / "w.wav"))
    line = "input: every FLAC file's MD5 is checked on the host before it is read"
    assert G.main(["--input", str(files / "wav"), "--output", str(tmp_path / "dw")] + tail) == 0
    dw = capsys.readouterr().out.splitlines()
    assert G.main(["--input", str(files / "mixed"), "--output", str(tmp_path / "dm"), "--input_formats", "wav,flac", "--verify_input"] + tail) == 0
    dm = capsys.readouterr().out.splitlines()
    assert dm.count(line) == 1 and [l.replace(str(tmp_path / "dm"), str(tmp_path / "dw")) for l in dm if l != line] == dw
    assert _count(reset=True) == 4
    for name in NAMES:
        assert _bytes(str(tmp_path / "dm" / (name + ".wav"))) == _bytes(str(tmp_path / "dw" / (name + ".wav")))
    assert G.main(["--input", str(files / "mixed"), "--output", str(tmp_path / "d1")] + tail) == 0     # the default lists the wav alone
    assert "1 of 1 files enhanced, 0 skipped" in capsys.readouterr().out and _count() == 0
    for extra, word in ((["--input", str(files / "mixed"), "--output", str(tmp_path / "never"), "--input_formats", "wav,mp3"], "input formats"),
                        (["--input", str(files / "b_stereo.flac"), "--output", str(tmp_path / "never.wav"), "--input_formats", "flac"], "folder")):
        with pytest.raises(SystemExit):
            G.main(extra + tail)
        assert word in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "never")) and not os.path.exists(str(tmp_path / "never.wav"))
