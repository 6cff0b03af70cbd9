"""AIFF / AIFF-C, AU and NIST SPHERE inputs through whole-file generation on the GPU: enhance_file on such a file writes the bytes it
writes for the file's WAV twin, with one launch of the decoder the input needs -- p2phd_pcm_decode_ex for big-endian or signed 8-bit
samples, p2phd_pcm_decode for little-endian ones (sowt, SPHERE 01), the family "wavcodec" for G.711 -- and a plain WAV input never
reaches the new entry; is_lr_input at 8 kHz; a folder that mixes the containers with a WAV input, in both loudness scopes;
container='flac'; an ima4 file is refused by name and skipped in folder mode; the command line.  The tiny model and the set-up are
those of tests/test_gpu_generate_wavcodec.py, restated; the files come from tests/_containers_ref.py."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _containers_ref as R
import _wavcodec_ref as W

pytestmark = pytest.mark.gpu

RATE = 48000
FRAMES = 1500                                                              # two segments of the tiny model


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


def _count(family=b"wavcodec", reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(family, 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _put(path, data):
    with open(str(path), "wb") as f:
        f.write(data)


def _i16(C, seed, frames=FRAMES):
    return W.speech_like(C, frames, seed)


def _i24(C, seed):
    return _i16(C, seed) * 256 + np.random.default_rng(seed).integers(-128, 128, size=(C, FRAMES))


def _g711(x, law):
    payload = W.g711_encode(x, law)
    return payload, W.g711_decode(payload, x.shape[1], x.shape[0], law)


# name -> (file name, channels, rate, make() -> (file bytes, twin), the entry its one decoder launch goes through)
def _makers():
    def aiff16():
        x = _i16(2, 1)
        return R.aiff(R.int_bytes(x, 2), 2, FRAMES, 16, rate=RATE), (1, 16, R.int_bytes(x, 2, False))

    def sowt():
        x = _i16(1, 2)
        return R.aiff(R.int_bytes(x, 2, False), 1, FRAMES, 16, rate=RATE, ctype=b"sowt", cname=b""), (1, 16, R.int_bytes(x, 2, False))

    def fl32():
        x = (_i24(2, 3) / 8388608.0).astype(np.float32)
        return R.aiff(R.float_bytes(x, 4), 2, FRAMES, 32, rate=RATE, ctype=b"fl32", cname=b"32-bit floating point"), (3, 32, R.float_bytes(x, 4, False))

    def aifc_ulaw():
        payload, ints = _g711(_i16(2, 4), W.ULAW)
        return R.aiff(payload, 2, FRAMES, 16, rate=RATE, ctype=b"ulaw", cname=b"CCITT G.711 u-law"), (1, 16, R.int_bytes(ints, 2, False))

    def au24():
        x = _i24(2, 5)
        return R.au(R.int_bytes(x, 3), 4, RATE, 2, annotation=b"take 1"), (1, 24, R.int_bytes(x, 3, False))

    def au_alaw():
        payload, ints = _g711(_i16(1, 6), W.ALAW)
        return R.au(payload, 27, RATE, 1, size=0xFFFFFFFF), (1, 16, R.int_bytes(ints, 2, False))

    def au_f64():
        x = _i24(1, 7) / 8388608.0 + 1e-9                                      # (not float32 values: the conversion rounds)
        return R.au(R.float_bytes(x, 8), 7, RATE, 1), (3, 64, R.float_bytes(x, 8, False))

    def sphere10():
        x = _i16(2, 8)
        return R.sphere(R.int_bytes(x, 2), R.sphere_fields(2, RATE, 2, FRAMES, "pcm", "10")), (1, 16, R.int_bytes(x, 2, False))

    def sphere01():
        x = _i16(1, 9)
        return R.sphere(R.int_bytes(x, 2, False), R.sphere_fields(1, RATE, 2, None, "pcm", "01")), (1, 16, R.int_bytes(x, 2, False))

    return {"aiff16": ("a.aif", 2, aiff16, "ex"), "sowt": ("b.aifc", 1, sowt, "pcm"), "fl32": ("c.aifc", 2, fl32, "ex"),
            "aifc_ulaw": ("d.aifc", 2, aifc_ulaw, "wavcodec"), "au24": ("e.au", 2, au24, "ex"), "au_alaw": ("f.snd", 1, au_alaw, "wavcodec"),
            "au_f64": ("g.au", 1, au_f64, "ex"), "sphere10": ("h.sph", 2, sphere10, "ex"), "sphere01": ("i.WAV", 1, sphere01, "pcm")}


MAKERS = _makers()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("containers_in")
    for sub in ("in", "twin", "lr", "mixed", "mixed_twin"):
        (d / sub).mkdir()
    for name, (fname, C, make, _) in MAKERS.items():
        data, twin = make()
        _put(d / "in" / fname, data)
        R.write_twin(str(d / "twin" / (name + ".wav")), twin, RATE, C)
    # a two-channel 8 kHz telephone file (Switchboard's shape) and its twin
    payload, ints = _g711(_i16(2, 10, 2500), W.ULAW)
    _put(d / "lr" / "sw.sph", R.sphere(payload, R.sphere_fields(2, 8000, 1, 2500, "ulaw")))
    W.write_pcm16_wav(str(d / "lr" / "sw_pcm.wav"), ints, 8000)
    # a folder of the three containers beside a WAV input, and the same folder with every file replaced by its twin
    for name in ("aiff16", "au24", "sphere10", "aifc_ulaw"):
        stem = os.path.splitext(MAKERS[name][0])[0]
        shutil.copy(str(d / "in" / MAKERS[name][0]), str(d / "mixed" / MAKERS[name][0]))
        shutil.copy(str(d / "twin" / (name + ".wav")), str(d / "mixed_twin" / (stem + ".wav")))
    pcm = torch.from_numpy(W.scale(_i16(1, 21, 2000)))
    for sub in ("mixed", "mixed_twin"):
        wavio.save(str(d / sub / "plain.wav"), pcm, RATE)
    return d


@pytest.fixture(scope="module")
def resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    from pix2pixhdaudiosr_amd.models.models import create_model
    opt = _opt(mdct_type="mdct4")
    torch.manual_seed(1234)
    model = create_model(opt)
    model.eval()
    return SuperResolver(model, opt, crossover='input')


@pytest.fixture
def ex_calls(monkeypatch):
    """Counts the calls of p2phd_pcm_decode_ex (which shares its launch family with the rest of csrc/pcm.hip)."""
    from pix2pixhdaudiosr_amd import _lib
    lib, calls = _lib.lib(), []
    entry = lib.p2phd_pcm_decode_ex

    def counted(*args):
        calls.append(args[4])                                              # (the flags)
        return entry(*args)
    monkeypatch.setattr(lib, "p2phd_pcm_decode_ex", counted)
    return calls


@pytest.mark.parametrize("name", list(MAKERS))
def test_container_writes_the_bytes_of_the_twin(resolver, files, tmp_path, ex_calls, name):
    from pix2pixhdaudiosr_amd.data import audiofile, containers, wavio
    fname, C, _, entry = MAKERS[name]
    src, twin = str(files / "in" / fname), str(files / "twin" / (name + ".wav"))
    assert torch.equal(audiofile.load(src)[0].view(torch.int32), wavio.load(twin)[0].view(torch.int32))
    resolver.enhance_file(twin, None, channels='all')                   # capture, tables, packed weights
    _count(reset=True)
    _count(b"pcm", reset=True)
    torch.manual_seed(5)
    a = resolver.enhance_file(twin, str(tmp_path / "t.wav"), channels='all')
    assert _count(reset=True) == 0 and ex_calls == []                   # a WAV input: nothing of "wavcodec", nothing through the new entry
    pcm_twin = _count(b"pcm", reset=True)
    torch.manual_seed(5)
    b = resolver.enhance_file(src, str(tmp_path / "c.wav"), channels='all')
    coded, pcm = _count(reset=True), _count(b"pcm", reset=True)
    if entry == "wavcodec":
        assert (coded, pcm, ex_calls) == (1, pcm_twin - 1, [])          # in place of the PCM decoder's launch
    else:
        assert (coded, pcm) == (0, pcm_twin) and len(ex_calls) == (1 if entry == "ex" else 0)           # one decoder launch, as the twin's
    assert _bytes(str(tmp_path / "c.wav")) == _bytes(str(tmp_path / "t.wav"))
    assert sorted(a) == sorted(b) and torch.equal(a['sr'], b['sr']) and torch.equal(a['lr'], b['lr']) and a['metrics'] == b['metrics']
    assert torch.equal(a['hr'].view(torch.int32), b['hr'].view(torch.int32))
    assert isinstance(b['info'], containers.AudioInfo) and b['info'] == containers.info(src) and b['info'][:3] == a['info'][:3]
    assert isinstance(a['info'], wavio.WavInfo) and b['info'].num_channels == C and b['info'].num_frames == FRAMES


def test_lr_input_at_8k(resolver, files, tmp_path, ex_calls):
    torch.manual_seed(5)
    a = resolver.enhance_file(str(files / "lr" / "sw_pcm.wav"), str(tmp_path / "t.wav"), is_lr_input=True, channels='all')
    _count(reset=True)
    torch.manual_seed(5)
    b = resolver.enhance_file(str(files / "lr" / "sw.sph"), str(tmp_path / "c.wav"), is_lr_input=True, channels='all')
    assert _count(reset=True) == 1 and ex_calls == []
    assert _bytes(str(tmp_path / "c.wav")) == _bytes(str(tmp_path / "t.wav")) and torch.equal(a['sr'], b['sr'])
    assert b['hr'] is None and b['metrics'] is None and b['info'].sample_rate == 8000 and b['sr'].shape == (2, a['sr'].shape[-1])
    assert b['info'].container == 'sphere' and b['sr'].shape[-1] >= 6 * 2500


def test_container_flac(resolver, files, tmp_path, ex_calls):
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "twin" / "au24.wav"), str(tmp_path / "t.flac"), channels='all', container='flac', encoding='pcm24')
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "in" / MAKERS["au24"][0]), str(tmp_path / "c.flac"), channels='all', container='flac', encoding='pcm24')
    assert len(ex_calls) == 1
    assert _bytes(str(tmp_path / "c.flac")) == _bytes(str(tmp_path / "t.flac")) and _bytes(str(tmp_path / "c.flac"))[:4] == b"fLaC"


@pytest.mark.parametrize("scope", ["file", "folder"])
def test_mixed_folder(resolver, files, tmp_path, ex_calls, scope):
    kw = dict(channels='all', seed=11)
    if scope == "folder":
        kw.update(loudness=-23.0, loudness_scope='folder', clip='guard', ceiling_dbfs=-3.0)
    base = resolver.enhance_folder(str(files / "mixed_twin"), str(tmp_path / "t"), input_formats=('wav',), **kw)
    assert ex_calls == []
    _count(reset=True)
    on = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "c"), input_formats='wav,aif,aifc,au,sph', **kw)
    assert _count(reset=True) == 1 and len(ex_calls) == 3               # the G.711 file; the three big-endian PCM files; the WAV input neither
    assert [r['path'] for r in on] == ["a.aif", "d.aifc", "e.au", "h.sph", "plain.wav"]
    assert [r['path'] for r in base] == ["a.wav", "d.wav", "e.wav", "h.wav", "plain.wav"] == [r['written'] for r in on]
    for r, w in zip(on, base):
        assert r['error'] is None and {k: v for k, v in r.items() if k != 'path'} == {k: v for k, v in w.items() if k != 'path'}
        assert _bytes(str(tmp_path / "c" / r['written'])) == _bytes(str(tmp_path / "t" / w['written']))
    # the default scan lists the WAV input alone, as before
    only = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "d"), **kw)
    assert [r['path'] for r in only] == ["plain.wav"] and sorted(os.listdir(str(tmp_path / "d"))) == ["plain.wav"]


def test_mixed_folder_to_flac(resolver, files, tmp_path):
    kw = dict(channels='all', seed=11, container='flac')
    base = resolver.enhance_folder(str(files / "mixed_twin"), str(tmp_path / "t"), **kw)
    on = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "c"), input_formats=('wav', 'aif', 'aifc', 'au', 'sph'), **kw)
    assert [r['written'] for r in on] == ["a.flac", "d.flac", "e.flac", "h.flac", "plain.flac"] == [r['written'] for r in base]
    for r in on:
        assert r['error'] is None and _bytes(str(tmp_path / "c" / r['written'])) == _bytes(str(tmp_path / "t" / r['written']))


def test_refused_file(resolver, files, tmp_path, ex_calls):
    d = tmp_path / "bad"
    d.mkdir()
    _put(d / "bad.aifc", R.aiff(bytes(34 * 2 * 40), 2, 64 * 40, 16, rate=RATE, ctype=b"ima4", cname=b"IMA 4:1"))
    shutil.copy(str(files / "in" / MAKERS["aiff16"][0]), str(d / "good.aif"))
    shutil.copy(str(files / "in" / MAKERS["au_alaw"][0]), str(d / "zgood.snd"))
    _count(reset=True)
    _count(b"pcm", reset=True)
    with pytest.raises(ValueError, match=r"bad\.aifc: AIFF-C compression type 'ima4' \(IMA 4:1\) is not read"):
        resolver.enhance_file(str(d / "bad.aifc"), str(tmp_path / "never.wav"), channels='all')
    assert _count() == 0 and _count(b"pcm") == 0 and ex_calls == [] and not os.path.exists(str(tmp_path / "never.wav"))      # before any launch
    recs = resolver.enhance_folder(str(d), str(tmp_path / "out"), channels='all', input_formats='aif,aifc,snd')
    assert [r['path'] for r in recs] == ["bad.aifc", "good.aif", "zgood.snd"]
    assert recs[0]['error'].startswith("ValueError") and "'ima4'" in recs[0]['error'] and recs[1]['error'] is None and recs[2]['error'] is None
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["good.wav", "zgood.wav"]
    # a truncated header is a skipped file too
    _put(d / "bad.aifc", _bytes(str(d / "good.aif"))[:30])
    recs = resolver.enhance_folder(str(d), str(tmp_path / "out2"), channels='all', input_formats='aif,aifc')
    assert recs[0]['error'].startswith("ValueError") and recs[1]['error'] is None and sorted(os.listdir(str(tmp_path / "out2"))) == ["good.wav"]


def test_wav_input_is_the_parents(resolver, files, tmp_path, ex_calls):
    """A plain WAV input: the data chunk goes through p2phd_pcm_decode, never the new entry, and result and file are those of the
    samples decoded by wavio on the host (the parent's path, restated: tests/test_gpu_generate_wavcodec.py)."""
    from pix2pixhdaudiosr_amd.data import wavio
    p = str(files / "mixed" / "plain.wav")
    _count(reset=True)
    _count(b"pcm", reset=True)
    torch.manual_seed(5)
    a = resolver.enhance_file(p, str(tmp_path / "a.wav"))
    assert _count() == 0 and _count(b"pcm") >= 2 and ex_calls == []
    assert a['info'] == wavio.WavInfo(RATE, 2000, 1, 16, 1, 44, 2) and type(a['info']) is wavio.WavInfo and sorted(a) == ['hr', 'info', 'lr', 'metrics', 'sr']
    assert torch.equal(a['hr'].cpu().reshape(-1).view(torch.int32), wavio.load(p)[0].reshape(-1).view(torch.int32))
    torch.manual_seed(5)
    b = resolver.enhance_file(p, str(tmp_path / "b.wav"))
    assert _bytes(str(tmp_path / "a.wav")) == _bytes(str(tmp_path / "b.wav")) and torch.equal(a['sr'], b['sr'])


def test_cli(files, tmp_path, capsys, ex_calls):
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
    assert G.main(["--input", str(files / "twin" / "aiff16.wav"), "--output", str(tmp_path / "w.wav")] + tail) == 0
    w = capsys.readouterr().out.splitlines()
    assert ex_calls == []
    assert G.main(["--input", str(files / "in" / "a.aif"), "--output", str(tmp_path / "f.wav")] + tail) == 0      # no new flag
    f = capsys.readouterr().out.splitlines()
    assert len(ex_calls) == 1 and [l.replace("f.wav", "w.wav") for l in f] == w
    assert _bytes(str(tmp_path / "f.wav")) == _bytes(str(tmp_path / "w.wav"))
    assert G.main(["--input", str(files / "mixed_twin"), "--output", str(tmp_path / "dw")] + tail) == 0
    dw = capsys.readouterr().out.splitlines()
    assert G.main(["--input", str(files / "mixed"), "--output", str(tmp_path / "dm"), "--input_formats", "wav,aif,aifc,au,sph"] + tail) == 0
    dm = capsys.readouterr().out.splitlines()
    swap = lambda l: l.replace(str(tmp_path / "dm"), str(tmp_path / "dw")).replace(str(files / "mixed"), str(files / "mixed_twin"))
    for ext in ("a.aif", "d.aifc", "e.au", "h.sph"):
        swap = (lambda l, ext=ext, inner=swap: inner(l).replace(ext, ext.split(".")[0] + ".wav"))
    assert [swap(l) for l in dm] == dw
    for name in ("a", "d", "e", "h", "plain"):
        assert _bytes(str(tmp_path / "dm" / (name + ".wav"))) == _bytes(str(tmp_path / "dw" / (name + ".wav")))
    assert G.main(["--input", str(files / "mixed"), "--output", str(tmp_path / "d1")] + tail) == 0     # the default lists the wav alone
    assert "1 of 1 files enhanced, 0 skipped" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        G.main(["--input", str(files / "mixed"), "--output", str(tmp_path / "never"), "--input_formats", "wav,aif,mp3"] + tail)
    assert "input formats" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "never"))
