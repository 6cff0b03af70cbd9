"""enhance_folder(pack_files=N) / --pack_files on the GPU: 1 is the run without the option; with a pass-through generator a packed
folder is written byte for byte as the unpacked one -- both transforms, with and without overlapping segments, and once with
every stage behind the rows switched on --, records and reports stay in plan order, a pack runs ceil(sum R / batch) groups on
the one capture; with the real tiny generator and a seed every segment's encoded input, mask noise and range are the same bits
packed and unpacked, and the waveform difference that is left -- what the generator does with a row's neighbours -- is printed.
The tiny model and the wrapped models are those of tests/test_gpu_generate_segment_norm.py."""
import math
import os

import pytest
import torch

from test_gpu_generate_segment_norm import PassThroughRows, RecordingRows, _real_rows
from test_gpu_lowband import _clip, _opt, _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCH = 4
# (name, channels, samples): different lengths and channel counts; c.wav does not parse
FILES = (("a.wav", 1, 2100), ("b.wav", 2, 4101), ("c.wav", 0, 0), ("d.wav", 1, 2000), ("sub/e.wav", 2, 23000))
STARTS = (1000, 7000, 0, 15000, 0)                                   # where in the 24000 samples of the golden excerpt each begins
GOOD = [f for f in FILES if f[1]]


def _count(family=b"stitch"):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib().p2phd_launch_count(family, 0)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from pix2pixhdaudiosr_amd.data import wavio
    d = tmp_path_factory.mktemp("pack_in")
    (d / "sub").mkdir()
    for k, (name, channels, n) in enumerate(FILES):
        if not channels:
            (d / name).write_bytes(b"RIFF this is no wav file at all")
            continue
        x = 0.5 * _clip(n, start=STARTS[k])
        assert x.numel() == n
        wavio.save(str(d / name), x if channels == 1 else torch.stack([x, 0.3 * x.flip(0)]), 48000)
    return d


def _rows(sr, opt):
    from pix2pixhdaudiosr_amd.generate import segment_plan
    return [c * segment_plan(n, opt.segment_length, sr.overlap)[0] for _, c, n in GOOD]


def _read_all(d, names):
    out = []
    for name in names:
        with open(os.path.join(str(d), name), "rb") as f:
            out.append(f.read())
    return out


def _run(sr, folder, out, **kw):
    reported = []
    records = sr.enhance_folder(str(folder), str(out), channels='all', report=reported.append, **kw)
    assert [r['path'] for r in records] == [f[0] for f in FILES]       # plan order
    assert len(reported) == len(records) and all(a is b for a, b in zip(reported, records))
    bad = records[2]
    assert bad['error'] is not None and bad['written_channels'] == 0 and [r['error'] for r in records if r is not bad] == [None] * 4
    return records


def _eq(a, b):
    """Records compare as they are; a tensor by its bits, a NaN equal to a NaN."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(_eq(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def _same_records(got, want):
    for g, w in zip(got, want):
        assert list(g) == list(w)
        for key in g:
            assert _eq(g[key], w[key]), (g['path'], key, g[key], w[key])


# ------------------------------------------------------------------------------------------
# a pass-through generator: the folder byte for byte
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [0, 0.25])
@pytest.mark.parametrize("mdct_type", ["mdct2", "mdct4"])
def test_packed_folder_is_the_unpacked_folder(folder, tmp_path, mdct_type, overlap):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny(mdct_type)
    sr = SuperResolver(PassThroughRows(model), opt, overlap=overlap, batch=BATCH, segment_norm=True)
    rows = _rows(sr, opt)
    names = [f[0] for f in GOOD]
    groups = []
    inner = sr._group_rows
    sr._group_rows = lambda seg, noise: (groups.append(1), inner(seg, noise))[1]
    before = _count()
    parent = _run(sr, folder, tmp_path / "p")                           # the call as it was before the option
    per_file = _count() - before
    assert per_file == 2 * len(GOOD)                                    # a planar gather and a planar stitch per file
    assert len(groups) == sum(math.ceil(r / BATCH) for r in rows)
    capture = sr._g['graph']
    assert capture is not None
    want = _read_all(tmp_path / "p", names)
    assert not os.path.exists(str(tmp_path / "p" / "c.wav"))
    for n, packs in ((1, [[0], [1], [2], [3]]), (3, [[0, 1, 2], [3]]), (8, [[0, 1, 2, 3]])):
        del groups[:]
        before = _count()
        records = _run(sr, folder, tmp_path / ("n%d" % n), pack_files=n)
        if n == 1:
            assert _count() - before == per_file                        # no ragged launch: the same launches as without the option
        else:
            assert _count() - before == 2 * len(packs)                  # one ragged gather and one ragged stitch per pack
        assert len(groups) == sum(math.ceil(sum(rows[i] for i in p) / BATCH) for p in packs)
        assert sr._g['graph'] is capture                                # one capture serves every pack
        assert _read_all(tmp_path / ("n%d" % n), names) == want, n
        assert not os.path.exists(str(tmp_path / ("n%d" % n) / "c.wav"))
        _same_records(records, parent)
    assert sum(math.ceil(r / BATCH) for r in rows) > math.ceil(sum(rows) / BATCH)    # the folder is one the option helps


@pytest.mark.parametrize("crossover_hz", [None, 'auto'])
def test_every_stage_behind_the_rows_packed_is_unpacked(folder, tmp_path, crossover_hz):
    """lowband 'input', a fixed or an auto crossover and mid/side around the rows; loudness to -23 LUFS, the true-peak guard, 44.1 kHz
    and the FLAC encoder behind them; the metrics table written from the records."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver, write_metrics_csv
    model, opt = _tiny("mdct4")
    sr = SuperResolver(PassThroughRows(model), opt, overlap=0.25, batch=BATCH, segment_norm=True, lowband='input', crossover='input',
                       stereo='ms', **({} if crossover_hz is None else dict(crossover_hz=crossover_hz)))
    stage = dict(loudness=-23.0, true_peak=True, clip='guard', output_rate=44100, container='flac', extended_metrics=True, dither='tpdf', dither_seed=5)
    names = [os.path.splitext(f[0])[0] + ".flac" for f in GOOD]
    outs = {}
    for n in (1, 3, 8):
        records = _run(sr, folder, tmp_path / ("n%d" % n), pack_files=n, **stage)
        csv = str(tmp_path / ("n%d.csv" % n))
        write_metrics_csv(csv, records, True, False, loudness=True, true_peak=True)
        with open(csv, "rb") as f:
            outs[n] = (_read_all(tmp_path / ("n%d" % n), names), f.read(), records)
        assert all(r['loudness'] is not None and r['flac'] is not None and r['output_rate'] is not None for r in records if r['error'] is None)
        assert all(('crossover' in r) == (crossover_hz == 'auto') for r in records)
        assert crossover_hz is None or all(r['crossover'] is not None for r in records if r['error'] is None)
    assert math.isfinite(outs[1][2][4]['loudness']['output'])           # the long file has a loudness, so the gain stage is in the bytes
    for n in (3, 8):
        assert outs[n][0] == outs[1][0] and outs[n][1] == outs[1][1], n
        _same_records(outs[n][2], outs[1][2])


# ------------------------------------------------------------------------------------------
# the real tiny generator, mask noise and a seed
# ------------------------------------------------------------------------------------------
class RecordingNoise(RecordingRows):
    """RecordingRows, with the mask noise every row was given kept beside its encoded input and range."""

    def __init__(self, real):
        super().__init__(real)
        self.noise = []

    def inference(self, lr_audio, inst, noise=None, **kw):
        self.noise.extend(noise[i].clone() for i in range(lr_audio.shape[0]))
        return super().inference(lr_audio, inst, noise=noise, **kw)


def test_with_the_generator_and_a_seed(folder, tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    kept = {}
    for n in (1, 8):
        rec = RecordingNoise(model)
        sr = SuperResolver(rec, opt, overlap=0.25, batch=BATCH, graph=False, segment_norm=True)
        rows = _rows(sr, opt)
        _run(sr, folder, tmp_path / ("n%d" % n), pack_files=n, seed=1234, encoding='float32')
        both = [r + (z,) for r, z in zip(rec.rows, rec.noise)]
        if n == 1:                                                      # file by file: every file's own fillers behind its rows
            real, at = [], 0
            for r in rows:
                padded = math.ceil(r / BATCH) * BATCH
                real += _real_rows(both[at:at + padded], r, BATCH)
                at += padded
            assert at == len(both)
        else:
            real = _real_rows(both, sum(rows), BATCH)
        kept[n] = real
    assert len(kept[1]) == len(kept[8]) == sum(_rows(sr, opt))
    for i, (got, want) in enumerate(zip(kept[8], kept[1])):
        for k, (g, w) in enumerate(zip(got, want)):                     # encoded input, phase, range, noise
            assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (i, k)
    # a file's noise is that of a run of its own: the rows of a file differ, and every file starts from the seed's first row
    assert len({tuple(r[3].reshape(-1)[:4].tolist()) for r in kept[8][:rows[0]]}) == rows[0] > 1
    assert torch.equal(kept[8][rows[0]][3], kept[8][0][3]) and torch.equal(kept[8][rows[0] + rows[1]][3], kept[8][0][3])
    # what the generator does with a row's neighbours in the batch: reported only
    worst = peak = 0.0
    for name, _, _ in GOOD:
        a, _ = wavio.load(str(tmp_path / "n1" / name))
        b, _ = wavio.load(str(tmp_path / "n8" / name))
        worst, peak = max(worst, float((a - b).abs().max())), max(peak, float(a.abs().max()))
    print(f"largest difference between the packed and the unpacked waveform {worst:.3e} at a peak of {peak:.3e}")


# ------------------------------------------------------------------------------------------
# refusals, the command line
# ------------------------------------------------------------------------------------------
def test_refusals(folder, tmp_path):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model, opt = _tiny("mdct4")
    off, on = SuperResolver(model, opt), SuperResolver(model, opt, segment_norm=True)
    with pytest.raises(ValueError, match=r"enhance_folder: pack_files 2 .* needs segment_norm"):
        off.enhance_folder(str(folder), str(tmp_path / "o"), pack_files=2)
    with pytest.raises(ValueError, match=r"pack_files is not built for loudness_scope 'folder'"):
        on.enhance_folder(str(folder), str(tmp_path / "o"), pack_files=2, loudness=-23.0, loudness_scope='folder')
    for bad in (0, True, 2.0):
        with pytest.raises(ValueError, match=r"pack_files must be an int >= 1"):
            on.enhance_folder(str(folder), str(tmp_path / "o"), pack_files=bad)
    with pytest.raises(ValueError, match=r"enhance_file: pack_files 2 .* is an option of enhance_folder"):
        on.enhance_file(str(folder / "a.wav"), str(tmp_path / "o" / "a.wav"), pack_files=2)
    assert on.enhance_file(str(folder / "a.wav"), None, pack_files=1)['sr'].shape == (1, 2100)
    with pytest.raises(ValueError, match=r"enhance_lr_many: .* needs segment_norm=True"):
        off.enhance_lr_many([torch.zeros(1, 100, device=DEV)])
    assert not os.path.exists(str(tmp_path / "o"))


def test_command_line(folder, tmp_path, capsys):
    from pix2pixhdaudiosr_amd.generate import main
    from pix2pixhdaudiosr_amd.models.models import create_model
    common = dict(mdct_type="mdct4", checkpoints_dir=str(tmp_path), name="run", seed=1234)
    torch.manual_seed(1234)
    create_model(_opt(**common)).save('latest')
    run = tmp_path / "run"
    with open(run / "opt.txt", "w") as f:                              # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    base = ["--input", str(folder), "--load_pretrain", str(run), "--channels", "all", "--segment_norm"]
    line = 'packing: up to 4 files share groups'
    capsys.readouterr()
    assert main(base + ["--output", str(tmp_path / "plain")]) == 0
    plain = capsys.readouterr().out
    assert 'packing' not in plain
    assert main(base + ["--output", str(tmp_path / "one"), "--pack_files", "1"]) == 0
    assert capsys.readouterr().out.replace(str(tmp_path / "one"), str(tmp_path / "plain")) == plain
    assert _read_all(tmp_path / "one", [f[0] for f in GOOD]) == _read_all(tmp_path / "plain", [f[0] for f in GOOD])
    before = _count()
    assert main(base + ["--output", str(tmp_path / "four"), "--pack_files", "4"]) == 0
    out = capsys.readouterr().out
    assert _count() - before == 2                                      # four files open: one pack
    assert out.splitlines().count(line) == 1 and len(out.splitlines()) == len(plain.splitlines()) + 1
    for word in ('wrote', 'skipped'):                                  # (the metric lines carry what the generator does with a batch)
        assert sum(l.startswith(word) for l in out.splitlines()) == sum(l.startswith(word) for l in plain.splitlines())
    assert [len(b) for b in _read_all(tmp_path / "four", [f[0] for f in GOOD])] == [len(b) for b in _read_all(tmp_path / "plain", [f[0] for f in GOOD])]
    with pytest.raises(SystemExit):
        main(["--input", str(folder), "--load_pretrain", str(run), "--output", str(tmp_path / "never"), "--pack_files", "4"])
    assert "needs segment_norm" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "never"))
