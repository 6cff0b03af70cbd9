"""The LPC option of FLAC output in whole-file generation on the GPU (container='flac', flac_lpc=M): with the option off the file is
the parent's, byte for byte, with the parent's launches; with it on out.flac, decoded by the host decoder, is still out.wav's data
chunk -- pcm16 and pcm24, with a dither, at another output rate -- the file is no longer than without and is the host encoder's to the
byte; the written FLAC as the next run's input; folders, the album flow, the command line and the refusals.  The tiny model and the
helpers are those of tests/test_gpu_generate_flac_out.py, restated."""
import os
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
    d = tmp_path_factory.mktemp("flac_lpc")
    (d / "in").mkdir()
    n = 2 * 4096 + 1234
    wavio.save(str(d / "in" / "a_mono.wav"), _signal(n).unsqueeze(0), RATE)
    wavio.save(str(d / "in" / "b_stereo.wav"), torch.stack([_signal(n - 500), _signal(n - 500, True)]), RATE)
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


def test_option_off_is_the_parent(resolver, files, tmp_path):
    """Without flac_lpc, with None and with 0: the same file, the same result keys, three launches each."""
    src = str(files / "in" / "b_stereo.wav")
    outs = []
    for i, kw in enumerate((dict(), dict(flac_lpc=None), dict(flac_lpc=0))):
        torch.manual_seed(5)
        _count(reset=True)
        r = resolver.enhance_file(src, str(tmp_path / ("%d.flac" % i)), channels='all', container='flac', **kw)
        assert _count(reset=True) == 3
        assert sorted(r['flac']) == ['block', 'bytes', 'frames', 'md5', 'pcm_bytes']
        outs.append((_bytes(str(tmp_path / ("%d.flac" % i))), r['flac']))
    assert outs[0] == outs[1] == outs[2]
    # ... and the file is the host encoder's without the option
    from pix2pixhdaudiosr_amd.data import flacio
    got, meta, table = _flac_chunk(str(tmp_path / "0.flac"))
    frames, lengths = flacio.encode(got, 2, 16, RATE, 4096)
    assert outs[0][0] == flacio.stream_header(lengths, RATE, 2, 16, meta.num_frames, 4096) + frames


OPTIONS = {
    "pcm16": dict(),
    "pcm24": dict(encoding='pcm24'),
    "tpdf": dict(dither='tpdf', dither_seed=3),
    "rate-44100": dict(output_rate=44100),
    "all-channels": dict(channels='all'),
    "block-1000-order-5": dict(channels='all', flac_block=1000, flac_lpc=5),
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_flac_decodes_to_the_wavs_data_chunk(resolver, files, tmp_path, name):
    from pix2pixhdaudiosr_amd.data import flacio
    kw = dict(OPTIONS[name])
    block, M = kw.pop('flac_block', None), kw.pop('flac_lpc', 12)
    fk = {} if block is None else dict(flac_block=block)
    src = str(files / "in" / "b_stereo.wav")
    pw, p0, pf = str(tmp_path / "o.wav"), str(tmp_path / "o0.flac"), str(tmp_path / "o.flac")
    torch.manual_seed(5)
    a = resolver.enhance_file(src, pw, **kw)
    torch.manual_seed(5)
    z = resolver.enhance_file(src, p0, container='flac', **kw, **fk)
    torch.manual_seed(5)
    _count(reset=True)
    b = resolver.enhance_file(src, pf, container='flac', flac_lpc=M, **kw, **fk)
    assert _count(reset=True) == 3
    assert sorted(list(a) + ['flac']) == sorted(b) and torch.equal(a['sr'], b['sr']) and a['metrics'] == b['metrics'] and a.get('output') == b.get('output')
    want, wmeta = _wav_chunk(pw)
    got, meta, table = _flac_chunk(pf)
    assert got == want and len(want) > 0
    assert (meta.sample_rate, meta.num_channels, meta.bits_per_sample, meta.num_frames) == \
           (wmeta.sample_rate, wmeta.num_channels, wmeta.bits_per_sample, wmeta.num_frames)
    assert meta.sample_rate == (44100 if name == "rate-44100" else RATE) and meta.min_block == meta.max_block == (block or 4096)
    assert b['flac'] == {'block': block or 4096, 'frames': len(table), 'bytes': os.path.getsize(pf), 'pcm_bytes': len(want), 'md5': None, 'lpc': M}
    assert 'lpc' not in z['flac']
    # no longer than without the option, frame by frame
    t0 = flacio.index_bytes(_bytes(p0), p0)[1]
    assert len(t0) == len(table) and (table[:, 1] <= t0[:, 1]).all() and os.path.getsize(pf) <= os.path.getsize(p0)
    # ... and the file is the host encoder's, to the byte
    frames, lengths = flacio.encode(want, meta.num_channels, meta.bits_per_sample, meta.sample_rate, block or 4096, lpc_order=M)
    assert _bytes(pf) == flacio.stream_header(lengths, meta.sample_rate, meta.num_channels, meta.bits_per_sample, meta.num_frames, block or 4096) + frames


def test_the_written_flac_as_input(resolver, files, tmp_path):
    """out.flac with LPC subframes fed back (the device decoder) gives what out.wav fed back gives."""
    src = str(files / "in" / "b_stereo.wav")
    pw, pf = str(tmp_path / "first.wav"), str(tmp_path / "first.flac")
    torch.manual_seed(5)
    resolver.enhance_file(src, pw, channels='all')
    torch.manual_seed(5)
    resolver.enhance_file(src, pf, channels='all', container='flac', flac_lpc=12)
    torch.manual_seed(7)
    resolver.enhance_file(pw, str(tmp_path / "second_w.wav"), channels='all')
    torch.manual_seed(7)
    resolver.enhance_file(pf, str(tmp_path / "second_f.wav"), channels='all')
    assert _bytes(str(tmp_path / "second_w.wav")) == _bytes(str(tmp_path / "second_f.wav"))


def test_folder_and_album_flow(resolver, files, tmp_path):
    from pix2pixhdaudiosr_amd.data import flacio
    for tag, kw in (("folder", dict(channels='all', seed=11)),
                    ("album", dict(channels='all', seed=11, loudness=-23.0, loudness_scope='folder', clip='guard', ceiling_dbfs=-3.0))):
        base = resolver.enhance_folder(str(files / "in"), str(tmp_path / (tag + "_w")), **kw)
        off = resolver.enhance_folder(str(files / "in"), str(tmp_path / (tag + "_0")), container='flac', flac_block=576, **kw)
        _count(reset=True)
        on = resolver.enhance_folder(str(files / "in"), str(tmp_path / (tag + "_f")), container='flac', flac_block=576, flac_lpc=8, **kw)
        assert _count(reset=True) == 6 and len(on) == len(base) == 2
        for r, z, w, name in zip(on, off, base, NAMES):
            pf = str(tmp_path / (tag + "_f") / (name + ".flac"))
            assert r['error'] is None and r['written'] == name + ".flac" and r.get('output') == w.get('output')
            got, meta, table = _flac_chunk(pf)
            assert got == _wav_chunk(str(tmp_path / (tag + "_w") / (name + ".wav")))[0]
            assert r['flac'] == {'block': 576, 'frames': len(table), 'bytes': os.path.getsize(pf), 'pcm_bytes': len(got), 'md5': None, 'lpc': 8}
            assert 'lpc' not in z['flac'] and r['flac']['bytes'] <= z['flac']['bytes']
            frames, lengths = flacio.encode(got, meta.num_channels, 16, RATE, 576, lpc_order=8)
            assert _bytes(pf) == flacio.stream_header(lengths, RATE, meta.num_channels, 16, meta.num_frames, 576) + frames


def test_refusals(resolver, files, tmp_path):
    src, out = str(files / "in" / "a_mono.wav"), str(tmp_path / "never.flac")
    _count(reset=True)
    for kw, text in ((dict(flac_lpc=4), "container"), (dict(flac_lpc=0), "container"), (dict(container='flac', flac_lpc=13), "flac_lpc"),
                     (dict(container='flac', flac_lpc=-1), "flac_lpc"), (dict(container='flac', flac_lpc=4.0), "flac_lpc"),
                     (dict(container='flac', flac_lpc=True), "flac_lpc"), (dict(container='flac', flac_lpc=1, flac_block=16385), "16384"),
                     (dict(container='flac', flac_lpc=12, encoding='float32'), "pcm16")):
        with pytest.raises(ValueError, match=text):
            resolver.enhance_file(src, out, **kw)
        with pytest.raises(ValueError, match=text):
            resolver.enhance_folder(str(files / "in"), str(tmp_path / "never_dir"), **kw)
    assert _count() == 0 and not os.path.exists(out) and not os.path.exists(str(tmp_path / "never_dir"))
    assert resolver.enhance_file(src, None, container='flac', flac_lpc=12)['flac'] is None      # no file asked for: nothing is encoded
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
    capsys.readouterr()
    assert G.main(["--input", src, "--output", str(tmp_path / "o0.flac"), "--container", "flac"] + tail) == 0
    off = capsys.readouterr().out.splitlines()
    _count(reset=True)
    assert G.main(["--input", src, "--output", str(tmp_path / "o.flac"), "--container", "flac", "--flac_lpc", "12"] + tail) == 0
    on = capsys.readouterr().out.splitlines()
    want = _wav_chunk(str(tmp_path / "o.wav"))[0]
    size = os.path.getsize(str(tmp_path / "o.flac"))
    line = "%s: FLAC 16 bit, %d frames of 4096, %d bytes (%.1f %% of the PCM), LPC up to order 12" % (
        str(tmp_path / "o.flac"), -(-len(want) // 4 // 4096), size, 100.0 * size / len(want))
    assert _count(reset=True) == 3 and on.count(line) == 1 and size <= os.path.getsize(str(tmp_path / "o0.flac"))
    assert not any("LPC" in l for l in off)                                 # without the flag: the lines of before
    assert [l for l in on if l != line] == [l.replace("o0.flac", "o.flac") for l in off if ": FLAC 16 bit," not in l]
    assert _flac_chunk(str(tmp_path / "o.flac"))[0] == want
    assert G.main(["--input", str(files / "in"), "--output", str(tmp_path / "d"), "--container", "flac", "--flac_block", "192", "--flac_lpc", "4"] + tail) == 0
    out = capsys.readouterr().out
    assert sorted(os.listdir(str(tmp_path / "d"))) == [n + ".flac" for n in NAMES] and out.count(", LPC up to order 4") == 2
    for extra, word in ((["--flac_lpc", "4"], "container"), (["--container", "flac", "--flac_lpc", "13"], "flac_lpc"),
                        (["--container", "flac", "--flac_lpc", "2", "--flac_block", "20000"], "16384")):
        with pytest.raises(SystemExit):
            G.main(["--input", src, "--output", str(tmp_path / "never.flac")] + extra + tail)
        assert word in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "never.flac"))
