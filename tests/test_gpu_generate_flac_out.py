"""FLAC output of whole-file generation on the GPU (container='flac'): out.flac, decoded by the host decoder, is out.wav's data chunk
byte for byte -- under both encodings, both dithers, the true-peak guard, another output rate and with all channels -- with three
launches of the family "flacenc" and none of them for a wav, which is written as before; the MD5 option; the written FLAC as the
next run's input; the result's figures; folders, the album flow, the command line and the refusals.  The tiny model is that of
tests/test_gpu_generate_flac.py, restated."""
import hashlib
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RATE = 48000
NAMES = ("a_mono", "b_stereo")


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


def _count(reset=False):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(b"flacenc", 1 if reset else 0)


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _wav_chunk(path):
    """The data chunk of a wav this build wrote: 44 bytes of header, then the payload (and a pad byte where it is odd)."""
    from pix2pixhdaudiosr_amd.data import wavio
    meta = wavio.info(path)
    n = meta.num_frames * meta.num_channels * meta.bits_per_sample // 8
    return _bytes(path)[44:44 + n], meta


def _flac_chunk(path):
    """The file through p2phd_flac_index and p2phd_flac_decode_host -> its samples as the interleaved little-endian payload."""
    from pix2pixhdaudiosr_amd.data import flacio
    data = _bytes(path)
    meta, table = flacio.index_bytes(data, path)
    pcm = flacio.decode_frames(data, table, 0, len(table), meta.num_channels, path)
    nb = meta.bits_per_sample // 8
    le = np.ascontiguousarray(pcm.T).astype("<i4").reshape(-1, 1).view(np.uint8)[:, :nb]
    return np.ascontiguousarray(le).tobytes(), meta, table


def _signal(n, flip=False, gain=0.9):
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    x = F["test_wav_excerpt_i16"].astype(np.float64) / 32768.0
    x = np.concatenate([x, 0.7 * x[::-1]])[:n]
    return torch.tensor(gain * (-0.6 * x[::-1] if flip else x).copy(), dtype=torch.float32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("flac_out")
    (d / "in").mkdir()
    n = 2 * 4096 + 1234
    wavio.save(str(d / "in" / "a_mono.wav"), _signal(n).unsqueeze(0), RATE)
    wavio.save(str(d / "in" / "b_stereo.wav"), torch.stack([_signal(n - 500), _signal(n - 500, True)]), RATE)
    wavio.save(str(d / "nine.wav"), torch.stack([_signal(2000, gain=0.1 * (c + 1)) for c in range(9)]), RATE)
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


def _pair(resolver, src, tmp_path, tag, **kw):
    """The same call twice, container 'wav' and 'flac' -> (wav result, flac result, wav path, flac path)."""
    pw, pf = str(tmp_path / (tag + ".wav")), str(tmp_path / (tag + ".flac"))
    torch.manual_seed(5)
    _count(reset=True)
    a = resolver.enhance_file(src, pw, **kw)
    assert _count(reset=True) == 0 and 'flac' not in a                 # a wav launches nothing of the family
    torch.manual_seed(5)
    b = resolver.enhance_file(src, pf, container='flac', **kw)
    assert _count(reset=True) == 3
    return a, b, pw, pf


def _same_result(a, b):
    assert sorted(list(a) + ['flac']) == sorted(b)
    assert torch.equal(a['sr'], b['sr']) and torch.equal(a['lr'], b['lr']) and a['metrics'] == b['metrics'] and a.get('output') == b.get('output')


def test_wav_is_written_as_before(resolver, files, tmp_path):
    src = str(files / "in" / "b_stereo.wav")
    torch.manual_seed(5)
    a = resolver.enhance_file(src, str(tmp_path / "a.wav"), channels='all')
    _count(reset=True)
    torch.manual_seed(5)
    b = resolver.enhance_file(src, str(tmp_path / "b.wav"), channels='all', container='wav')
    assert _count() == 0 and sorted(a) == sorted(b) and 'flac' not in b
    assert _bytes(str(tmp_path / "a.wav")) == _bytes(str(tmp_path / "b.wav"))


OPTIONS = {
    "pcm16": dict(),
    "pcm24": dict(encoding='pcm24'),
    "tpdf": dict(dither='tpdf', dither_seed=3),
    "shaped": dict(dither='shaped', dither_seed=3),
    "guard-true-peak": dict(clip='guard', ceiling_dbfs=-6.0, true_peak=True),
    "rate-44100": dict(output_rate=44100),
    "all-channels": dict(channels='all'),
    "block-1000": dict(channels='all', flac_block=1000),
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_flac_decodes_to_the_wavs_data_chunk(resolver, files, tmp_path, name):
    from pix2pixhdaudiosr_amd.data import flacio
    kw = dict(OPTIONS[name])
    block = kw.pop('flac_block', None)
    src = str(files / "in" / "b_stereo.wav")
    pw, pf = str(tmp_path / "o.wav"), str(tmp_path / "o.flac")
    torch.manual_seed(5)
    _count(reset=True)
    a = resolver.enhance_file(src, pw, **kw)
    assert _count(reset=True) == 0 and 'flac' not in a                 # a wav launches nothing of the family
    torch.manual_seed(5)
    b = resolver.enhance_file(src, pf, container='flac', **kw, **({} if block is None else dict(flac_block=block)))
    assert _count(reset=True) == 3
    _same_result(a, b)
    want, wmeta = _wav_chunk(pw)
    got, meta, table = _flac_chunk(pf)
    assert got == want and len(want) > 0
    assert (meta.sample_rate, meta.num_channels, meta.bits_per_sample, meta.num_frames) == \
           (wmeta.sample_rate, wmeta.num_channels, wmeta.bits_per_sample, wmeta.num_frames)
    assert meta.sample_rate == (44100 if name == "rate-44100" else RATE) and meta.num_channels == (2 if 'channels' in kw else 1)
    assert meta.min_block == meta.max_block == (block or 4096) and meta.md5 == b"\0" * 16 and flacio.verify(pf) is None
    # the result's figures are the file's
    assert b['flac'] == {'block': block or 4096, 'frames': len(table), 'bytes': os.path.getsize(pf), 'pcm_bytes': len(want), 'md5': None}
    assert len(table) == -(-meta.num_frames // (block or 4096))
    # ... and the file is the host encoder's, to the byte
    frames, lengths = flacio.encode(want, meta.num_channels, meta.bits_per_sample, meta.sample_rate, block or 4096)
    assert _bytes(pf) == flacio.stream_header(lengths, meta.sample_rate, meta.num_channels, meta.bits_per_sample, meta.num_frames, block or 4096) + frames


def test_md5(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.data import flacio
    a, b, pw, pf = _pair(resolver, str(files / "in" / "b_stereo.wav"), tmp_path, "m", channels='all')
    torch.manual_seed(5)
    c = resolver.enhance_file(str(files / "in" / "b_stereo.wav"), str(tmp_path / "m5.flac"), channels='all', container='flac', flac_md5=True)
    want, _ = _wav_chunk(pw)
    digest = hashlib.md5(want).digest()
    assert c['flac']['md5'] == digest.hex() and flacio.info(str(tmp_path / "m5.flac")).md5 == digest
    assert flacio.verify(str(tmp_path / "m5.flac")) is True
    x, y = _bytes(pf), _bytes(str(tmp_path / "m5.flac"))
    assert x[:26] == y[:26] and x[42:] == y[42:] and y[26:42] == digest     # nothing but the MD5 field differs


def test_the_written_flac_as_input(resolver, files, tmp_path):
    """out.flac fed back gives what out.wav fed back gives."""
    a, b, pw, pf = _pair(resolver, str(files / "in" / "b_stereo.wav"), tmp_path, "first", channels='all')
    torch.manual_seed(7)
    resolver.enhance_file(pw, str(tmp_path / "second_w.wav"), channels='all')
    torch.manual_seed(7)
    resolver.enhance_file(pf, str(tmp_path / "second_f.wav"), channels='all')
    assert _bytes(str(tmp_path / "second_w.wav")) == _bytes(str(tmp_path / "second_f.wav"))


def test_folder(resolver, files, tmp_path):
    base = resolver.enhance_folder(str(files / "in"), str(tmp_path / "w"), channels='all', seed=11)
    _count(reset=True)
    on = resolver.enhance_folder(str(files / "in"), str(tmp_path / "f"), channels='all', seed=11, container='flac', flac_block=576)
    assert _count(reset=True) == 6
    assert sorted(os.listdir(str(tmp_path / "f"))) == [n + ".flac" for n in NAMES]
    assert [r['path'] for r in on] == [n + ".wav" for n in NAMES] and [r['written'] for r in on] == [n + ".flac" for n in NAMES]
    for r, w, name in zip(on, base, NAMES):
        assert 'written' not in w and 'flac' not in w and r['error'] is None
        assert {k: v for k, v in r.items() if k not in ('written', 'flac')} == w
        got, meta, table = _flac_chunk(str(tmp_path / "f" / (name + ".flac")))
        assert got == _wav_chunk(str(tmp_path / "w" / (name + ".wav")))[0]
        assert r['flac'] == {'block': 576, 'frames': len(table), 'bytes': os.path.getsize(str(tmp_path / "f" / (name + ".flac"))), 'pcm_bytes': len(got), 'md5': None}
    # x.wav beside x.flac would both be written to x.flac
    clash = tmp_path / "clash"
    clash.mkdir()
    shutil.copy(str(files / "in" / "a_mono.wav"), str(clash / "a_mono.wav"))
    shutil.copy(str(tmp_path / "f" / "a_mono.flac"), str(clash / "a_mono.flac"))
    with pytest.raises(ValueError, match="both be written"):
        resolver.enhance_folder(str(clash), str(tmp_path / "never"), input_formats='wav,flac', container='flac')
    assert not os.path.exists(str(tmp_path / "never"))
    # a file with more channels than a FLAC stream holds is a skipped file
    nine = tmp_path / "nine"
    nine.mkdir()
    shutil.copy(str(files / "nine.wav"), str(nine / "nine.wav"))
    shutil.copy(str(files / "in" / "a_mono.wav"), str(nine / "ok.wav"))
    recs = resolver.enhance_folder(str(nine), str(tmp_path / "nine_out"), channels='all', container='flac')
    assert "at most 8 channels" in recs[0]['error'] and recs[1]['error'] is None and os.listdir(str(tmp_path / "nine_out")) == ["ok.flac"]


def test_album_flow(resolver, files, tmp_path):
    kw = dict(channels='all', seed=11, loudness=-23.0, loudness_scope='folder', clip='guard', ceiling_dbfs=-3.0)
    base = resolver.enhance_folder(str(files / "in"), str(tmp_path / "w"), **kw)
    _count(reset=True)
    on = resolver.enhance_folder(str(files / "in"), str(tmp_path / "f"), container='flac', flac_md5=True, **kw)
    assert _count(reset=True) == 6 and len(on) == len(base) == 2
    from pix2pixhdaudiosr_amd.data import flacio
    for r, w, name in zip(on, base, NAMES):
        assert r['error'] is None and r['album'] == w['album'] and r['loudness'] == w['loudness'] and r['output'] == w['output']
        assert r['written'] == name + ".flac"
        want = _wav_chunk(str(tmp_path / "w" / (name + ".wav")))[0]
        assert _flac_chunk(str(tmp_path / "f" / (name + ".flac")))[0] == want
        assert r['flac']['md5'] == hashlib.md5(want).hexdigest() and flacio.verify(str(tmp_path / "f" / (name + ".flac"))) is True


def test_refusals(resolver, files, tmp_path):
    src, out = str(files / "in" / "a_mono.wav"), str(tmp_path / "never.flac")
    _count(reset=True)
    for kw, text in ((dict(container='flac', encoding='float32'), "pcm16"), (dict(container='flac', flac_block=15), "flac_block"),
                     (dict(container='flac', flac_block=65536), "flac_block"), (dict(container='flac', flac_block=4096.0), "flac_block"),
                     (dict(flac_block=4096), "container"), (dict(flac_md5=True), "container"), (dict(container='ogg'), "container"),
                     (dict(container='flac', output_rate=2000000), "rate")):
        with pytest.raises(ValueError, match=text):
            resolver.enhance_file(src, out, **kw)
        with pytest.raises(ValueError, match=text):
            resolver.enhance_folder(str(files / "in"), str(tmp_path / "never_dir"), **kw)
    with pytest.raises(ValueError, match="at most 8 channels"):
        resolver.enhance_file(str(files / "nine.wav"), out, channels='all', container='flac')
    assert _count() == 0 and not os.path.exists(out) and not os.path.exists(str(tmp_path / "never_dir"))
    assert resolver.enhance_file(src, None, container='flac')['flac'] is None      # no file asked for: nothing is encoded
    assert _count() == 0


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
    src = str(files / "in" / "b_stereo.wav")
    assert G.main(["--input", src, "--output", str(tmp_path / "o.wav")] + tail) == 0
    w = capsys.readouterr().out.splitlines()
    _count(reset=True)
    assert G.main(["--input", src, "--output", str(tmp_path / "o.flac"), "--container", "flac", "--flac_md5"] + tail) == 0
    f = capsys.readouterr().out.splitlines()
    want = _wav_chunk(str(tmp_path / "o.wav"))[0]
    size = os.path.getsize(str(tmp_path / "o.flac"))
    line = "%s: FLAC 16 bit, %d frames of 4096, %d bytes (%.1f %% of the PCM), MD5 %s" % (
        str(tmp_path / "o.flac"), -(-len(want) // 4 // 4096), size, 100.0 * size / len(want), hashlib.md5(want).hexdigest())
    assert _count(reset=True) == 3 and f.count(line) == 1
    assert [l.replace("o.flac", "o.wav") for l in f if l != line] == w           # one line more, nothing else
    assert _flac_chunk(str(tmp_path / "o.flac"))[0] == want
    assert G.main(["--input", str(files / "in"), "--output", str(tmp_path / "d"), "--container", "flac", "--flac_block", "192"] + tail) == 0
    out = capsys.readouterr().out
    assert sorted(os.listdir(str(tmp_path / "d"))) == [n + ".flac" for n in NAMES]
    for n in NAMES:
        assert "wrote %s" % str(tmp_path / "d" / (n + ".flac")) in out and "%s: FLAC 16 bit," % str(tmp_path / "d" / (n + ".flac")) in out
    assert " frames of 192, " in out
    for extra, word in ((["--flac_block", "192"], "container"), (["--flac_md5"], "container"), (["--container", "flac", "--encoding", "float32"], "pcm16"),
                        (["--container", "flac", "--flac_block", "8"], "flac_block")):
        with pytest.raises(SystemExit):
            G.main(["--input", src, "--output", str(tmp_path / "never.flac")] + extra + tail)
        assert word in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "never.flac"))
