"""Coded WAV inputs (G.711 mu-law / A-law, IMA ADPCM) through whole-file generation on the GPU: enhance_file on a coded file writes
the bytes it writes for the file's PCM16 twin, with one launch of the family "wavcodec" in place of the PCM decoder's and none of it
for a PCM input; is_lr_input at 8 kHz; folders that mix coded, PCM and FLAC inputs, in both loudness scopes; container='flac'; a bad
IMA block header is a ValueError that names file and block, and a skipped file in folder mode.  The tiny model is that of
tests/test_gpu_generate_flac.py, restated; the coded files come from the restatement tests/_wavcodec_ref.py."""
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _wavcodec_ref as R

pytestmark = pytest.mark.gpu

RATE = 48000
KINDS = ("ulaw", "alaw", "ima_mono", "ima_stereo")


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


def _write_pair(d, kind, rate, frames, seed):
    """`kind`.wav (coded) under d / 'coded' and its PCM16 twin of the same name under d / 'twin'."""
    C = 2 if kind == "ima_stereo" else 1
    x = R.speech_like(C, frames, seed)
    coded, twin = str(d / "coded" / (kind + ".wav")), str(d / "twin" / (kind + ".wav"))
    if kind.startswith("ima"):
        align = 256 * C
        payload = R.ima_encode(x, align)                                    # ends in a partial block
        ints = R.ima_decode(payload, C, align)
        R.write_coded_wav(coded, R.TAG_IMA, payload, rate, C, block_align=align, fact=ints.shape[1] - 3)      # `fact` cuts three frames
        ints = ints[:, :-3]
    else:
        law = R.ULAW if kind == "ulaw" else R.ALAW
        payload = R.g711_encode(x, law)
        ints = R.g711_decode(payload, frames, C, law)
        R.write_coded_wav(coded, R.TAG_ULAW if kind == "ulaw" else R.TAG_ALAW, payload, rate, C, extensible=kind == "alaw")
    R.write_pcm16_wav(twin, ints, rate)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import flacio, wavio
    d = tmp_path_factory.mktemp("wavcodec_in")
    for sub in ("coded", "twin", "lr", "mixed", "mixed_twin"):
        (d / sub).mkdir()
    for i, kind in enumerate(KINDS):
        _write_pair(d, kind, RATE, 3 * 4096 + 777 - 100 * i, seed=i)
    # an 8 kHz telephone file and its twin
    x = R.speech_like(1, 2500, 9)
    payload = R.g711_encode(x, R.ULAW)
    R.write_coded_wav(str(d / "lr" / "phone.wav"), R.TAG_ULAW, payload, 8000, 1)
    R.write_pcm16_wav(str(d / "lr" / "phone_pcm.wav"), R.g711_decode(payload, 2500, 1, R.ULAW), 8000)
    # a folder of coded, PCM and FLAC inputs, and the same folder with every coded file replaced by its twin
    for kind in ("ulaw", "ima_stereo"):
        shutil.copy(str(d / "coded" / (kind + ".wav")), str(d / "mixed" / (kind + ".wav")))
        shutil.copy(str(d / "twin" / (kind + ".wav")), str(d / "mixed_twin" / (kind + ".wav")))
    pcm = torch.from_numpy(R.scale(R.speech_like(1, 9000, 21)))
    for sub in ("mixed", "mixed_twin"):
        wavio.save(str(d / sub / "plain.wav"), pcm, RATE)
        flacio.save(str(d / sub / "zz.flac"), pcm.flip(-1), RATE)
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


@pytest.mark.parametrize("kind", KINDS)
def test_coded_writes_the_bytes_of_the_twin(resolver, files, tmp_path, kind):
    from pix2pixhdaudiosr_amd.data import wavio
    coded, twin = str(files / "coded" / (kind + ".wav")), str(files / "twin" / (kind + ".wav"))
    assert torch.equal(wavio.load(coded)[0].view(torch.int32), wavio.load(twin)[0].view(torch.int32))
    resolver.enhance_file(twin, None, channels='all')                   # capture, tables, packed weights
    _count(reset=True)
    _count(b"pcm", reset=True)
    torch.manual_seed(5)
    a = resolver.enhance_file(twin, str(tmp_path / "t.wav"), channels='all')
    assert _count(reset=True) == 0                                      # a PCM input launches nothing of the family
    pcm_twin = _count(b"pcm", reset=True)
    torch.manual_seed(5)
    b = resolver.enhance_file(coded, str(tmp_path / "c.wav"), channels='all')
    assert _count(reset=True) == 1 and _count(b"pcm", reset=True) == pcm_twin - 1        # in place of the PCM decoder's launch
    assert _bytes(str(tmp_path / "c.wav")) == _bytes(str(tmp_path / "t.wav"))
    assert sorted(a) == sorted(b) and torch.equal(a['sr'], b['sr']) and torch.equal(a['lr'], b['lr']) and a['metrics'] == b['metrics']
    assert torch.equal(a['hr'].view(torch.int32), b['hr'].view(torch.int32))
    assert isinstance(b['info'], wavio.WavInfo) and b['info'] == wavio.info(coded) and b['info'][:3] == a['info'][:3]
    assert b['info'].format_tag == {"ulaw": 7, "alaw": 6}.get(kind, 0x11) and a['info'].format_tag == 1


def test_lr_input_at_8k(resolver, files, tmp_path):
    torch.manual_seed(5)
    a = resolver.enhance_file(str(files / "lr" / "phone_pcm.wav"), str(tmp_path / "t.wav"), is_lr_input=True)
    _count(reset=True)
    torch.manual_seed(5)
    b = resolver.enhance_file(str(files / "lr" / "phone.wav"), str(tmp_path / "c.wav"), is_lr_input=True)
    assert _count(reset=True) == 1
    assert _bytes(str(tmp_path / "c.wav")) == _bytes(str(tmp_path / "t.wav")) and torch.equal(a['sr'], b['sr'])
    assert b['hr'] is None and b['metrics'] is None and b['info'].sample_rate == 8000 and b['sr'].shape[-1] >= 6 * 2500


def test_container_flac(resolver, files, tmp_path):
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "twin" / "ima_stereo.wav"), str(tmp_path / "t.flac"), channels='all', container='flac')
    _count(reset=True)
    torch.manual_seed(5)
    resolver.enhance_file(str(files / "coded" / "ima_stereo.wav"), str(tmp_path / "c.flac"), channels='all', container='flac')
    assert _count(reset=True) == 1
    assert _bytes(str(tmp_path / "c.flac")) == _bytes(str(tmp_path / "t.flac")) and _bytes(str(tmp_path / "c.flac"))[:4] == b"fLaC"


@pytest.mark.parametrize("scope", ["file", "folder"])
def test_mixed_folder(resolver, files, tmp_path, scope):
    kw = dict(channels='all', seed=11, input_formats=('wav', 'flac'))
    if scope == "folder":
        kw.update(loudness=-23.0, loudness_scope='folder', clip='guard', ceiling_dbfs=-3.0)
    base = resolver.enhance_folder(str(files / "mixed_twin"), str(tmp_path / "t"), **kw)
    _count(reset=True)
    on = resolver.enhance_folder(str(files / "mixed"), str(tmp_path / "c"), **kw)
    assert _count(reset=True) == 2                                      # the two coded files; the PCM and the FLAC input launch none
    names = ["ima_stereo.wav", "plain.wav", "ulaw.wav", "zz.flac"]
    assert [r['path'] for r in on] == names == [r['path'] for r in base]
    for r, w in zip(on, base):
        assert r['error'] is None and r == w
        assert _bytes(str(tmp_path / "c" / r['written'])) == _bytes(str(tmp_path / "t" / w['written']))


def test_bad_block_header(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path / "bad"
    d.mkdir()
    src = str(files / "coded" / "ima_stereo.wav")
    meta = wavio.info(src)
    data = bytearray(_bytes(src))
    data[meta.data_offset + 5 * meta.block_align + 4 + 2] = 89              # block 5, channel 1: a step index above 88
    open(str(d / "bad.wav"), "wb").write(bytes(data))
    shutil.copy(str(files / "coded" / "ulaw.wav"), str(d / "good.wav"))
    _count(reset=True)
    with pytest.raises(ValueError, match=r"bad\.wav: block 5: a step index above 88"):
        resolver.enhance_file(str(d / "bad.wav"), str(tmp_path / "never.wav"), channels='all')
    assert _count() == 0 and not os.path.exists(str(tmp_path / "never.wav"))           # refused before anything is launched
    recs = resolver.enhance_folder(str(d), str(tmp_path / "out"), channels='all')
    assert [r['path'] for r in recs] == ["bad.wav", "good.wav"]
    assert recs[0]['error'].startswith("ValueError") and "block 5" in recs[0]['error'] and recs[1]['error'] is None
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["good.wav"]
    # what wavio refuses is a ValueError in file mode and a skipped file in folder mode too (MS ADPCM: not built)
    R.write_coded_wav(str(d / "bad.wav"), 2, b"\0" * 512, RATE, 1, block_align=256, bits=4)
    with pytest.raises(ValueError, match=r"unsupported WAVE format \(tag 2, 4 bit, 1 ch\)"):
        resolver.enhance_file(str(d / "bad.wav"), str(tmp_path / "never.wav"))
    assert not os.path.exists(str(tmp_path / "never.wav"))


def test_pcm_input_is_the_parents(resolver, files, tmp_path):
    """A PCM input: nothing of the family is launched, the data chunk goes through the PCM decoder, and result and file are those of
    the samples decoded by wavio on the host (the parent's path, restated: enhance_lr on the same waveform)."""
    from pix2pixhdaudiosr_amd.data import wavio
    p = str(files / "mixed" / "plain.wav")
    _count(reset=True)
    _count(b"pcm", reset=True)
    torch.manual_seed(5)
    a = resolver.enhance_file(p, str(tmp_path / "a.wav"))
    assert _count() == 0 and _count(b"pcm") >= 2                          # decode and encode
    assert a['info'] == wavio.WavInfo(RATE, 9000, 1, 16, 1, 44, 2) and sorted(a) == ['hr', 'info', 'lr', 'metrics', 'sr']
    assert torch.equal(a['hr'].cpu().reshape(-1).view(torch.int32), wavio.load(p)[0].reshape(-1).view(torch.int32))
    torch.manual_seed(5)
    b = resolver.enhance_file(p, str(tmp_path / "b.wav"))
    assert _bytes(str(tmp_path / "a.wav")) == _bytes(str(tmp_path / "b.wav")) and torch.equal(a['sr'], b['sr'])
