"""pack_files without a GPU: how a folder's files form packs (plans.pack_plan), every refusal of the option, of enhance_lr_many and
of the command line, the numpy restatement of the ragged gather and stitch (tests/_ragged_ref.py) against the per-clip restatement
(tests/_generate_ref.py), and the three parts of enhance_lr_many on a SuperResolver built without a device, its two ragged
launches replaced by the restatement: the group function runs ceil(sum R / batch) times for the pack."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _generate_ref as G
import _ragged_ref as RG


# ------------------------------------------------------------------------------------------
# the packs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[], [7], [1, 2, 3, 4, 5], [5, 5, 20, 1, 1, 1], [10, 10, 10], [11, 1, 11], [0, 0, 0, 0], [3, 3, 3, 3, 3, 3, 3]])
@pytest.mark.parametrize("pack_files", [1, 2, 3, 8])
@pytest.mark.parametrize("max_bytes", [10, 1 << 30])
def test_pack_plan(sizes, pack_files, max_bytes):
    from pix2pixhdaudiosr_amd.generate import pack_plan
    packs = pack_plan(sizes, pack_files, max_bytes)
    assert [i for p in packs for i in p] == list(range(len(sizes)))                  # every file in exactly one pack, order kept
    assert all(1 <= len(p) <= pack_files for p in packs)
    for p, nxt in zip(packs, packs[1:] + [None]):
        held = sum(sizes[i] for i in p)
        assert held <= max_bytes or len(p) == 1                                      # the byte cap; an oversized file alone
        if nxt is not None:                                                          # a pack closes for one of the two reasons only
            assert len(p) == pack_files or held + sizes[nxt[0]] > max_bytes
    if pack_files == 1:
        assert packs == [[i] for i in range(len(sizes))]


def test_pack_plan_figures_and_refusals():
    from pix2pixhdaudiosr_amd.generate import PACK_MAX_BYTES, pack_plan
    assert PACK_MAX_BYTES == 1 << 30
    assert pack_plan([5, 5, 20, 1, 1, 1], 3, 10) == [[0, 1], [2], [3, 4, 5]]
    assert pack_plan([4] * 5, 2) == [[0, 1], [2, 3], [4]]
    assert pack_plan([PACK_MAX_BYTES + 1, 1, PACK_MAX_BYTES - 1, 1], 4) == [[0], [1, 2], [3]]      # 1 + (cap - 1) still fits, one more not
    for bad in (0, -1, True, 2.0, None, '2'):
        with pytest.raises(ValueError, match=r"pack_plan: pack_files must be an int >= 1"):
            pack_plan([1, 2], bad)
    for bad in (0, -5, 1.5, None):
        with pytest.raises(ValueError, match=r"pack_plan: max_bytes"):
            pack_plan([1, 2], 2, bad)
    for bad in ([1, -1], [1.0], [None], [True]):
        with pytest.raises(ValueError, match=r"pack_plan: sizes"):
            pack_plan(bad, 2)


# ------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------
def test_check_pack_files():
    from pix2pixhdaudiosr_amd.generate import check_pack_files
    assert check_pack_files() == 1
    assert check_pack_files(1, False) == 1 and check_pack_files(1, False, 'folder') == 1     # the default changes nothing anywhere
    assert check_pack_files(4, True) == 4 and check_pack_files(65536, True, 'file') == 65536
    for bad in (True, False, 0, -3, 2.0, None, '4'):
        with pytest.raises(ValueError, match=r"^enhance_folder: pack_files must be an int >= 1"):
            check_pack_files(bad)
    with pytest.raises(ValueError, match=r"^enhance_folder: pack_files 2 .* needs segment_norm"):
        check_pack_files(2, False)
    with pytest.raises(ValueError, match=r"^generate: pack_files is not built for loudness_scope 'folder'"):
        check_pack_files(2, True, 'folder', who="generate")


def _bare(batch=4, T=8, overlap=0.25, segment_norm=True):
    """A SuperResolver built without __init__ and without a device: what the three parts of enhance_lr_many read."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver.__new__(SuperResolver)
    sr.device, sr.batch, sr.T, sr.graph, sr.segment_norm, sr.overlap = torch.device('cpu'), batch, T, False, segment_norm, overlap
    sr.crossover_plan, sr.gain = None, 1.5
    sr.opt = SimpleNamespace(hr_sampling_rate=48000, lr_sampling_rate=8000)
    sr.model = SimpleNamespace(mask_noise_shape=None)
    sr.calls = []

    def group(seg, noise):                                         # the rows back, doubled; a row's range: (its first sample, its sum)
        sr.calls.append(seg.clone())
        ranges = torch.zeros((seg.shape[0], 8))
        ranges[:, 0], ranges[:, 1] = seg[:, 0], seg.sum(dim=1)
        return 2 * seg, ranges

    sr._group_rows = group
    return sr


def test_refused_before_a_file_is_opened(tmp_path):
    opened = []
    for kw, segment_norm, word in ((dict(pack_files=2), False, r"needs segment_norm"),
                                   (dict(pack_files=2, loudness=-23.0, loudness_scope='folder'), True, r"loudness_scope 'folder'"),
                                   (dict(pack_files=0), True, r"pack_files must be an int >= 1"),
                                   (dict(pack_files=True), True, r"pack_files must be an int >= 1")):
        sr = _bare(segment_norm=segment_norm)
        sr._read = lambda *a, **k: opened.append(a)
        with pytest.raises(ValueError, match=word):
            sr.enhance_folder(str(tmp_path / "no_such_folder"), str(tmp_path / "out"), **kw)
    assert not opened and not (tmp_path / "out").exists()
    # enhance_file takes the option as enhance_folder does -- the two entry points take the same options -- and refuses more than 1
    for kw, segment_norm, word in ((dict(pack_files=2), True, r"enhance_file: pack_files 2 .* is an option of enhance_folder"),
                                   (dict(pack_files=2), False, r"enhance_file: pack_files 2 .* needs segment_norm"),
                                   (dict(pack_files=0), True, r"enhance_file: pack_files must be an int >= 1")):
        sr = _bare(segment_norm=segment_norm)
        sr._read = lambda *a, **k: opened.append(a)
        with pytest.raises(ValueError, match=word):
            sr.enhance_file(str(tmp_path / "no_such.wav"), str(tmp_path / "out.wav"), **kw)
    assert not opened and not (tmp_path / "out.wav").exists()
    with pytest.raises(ValueError, match=r"enhance_lr_many: .* needs segment_norm=True"):
        _bare(segment_norm=False).enhance_lr_many([torch.zeros(1, 5)])
    assert _bare().enhance_lr_many([]) == []


def test_command_line(capsys, tmp_path):
    from pix2pixhdaudiosr_amd.generate import _parser, main
    (tmp_path / "in").mkdir()
    folder = ["--input", str(tmp_path / "in"), "--output", str(tmp_path / "out"), "--load_pretrain", str(tmp_path / "no_such_checkpoint")]
    single = ["--input", str(tmp_path / "a.wav"), "--output", str(tmp_path / "b.wav"), "--load_pretrain", str(tmp_path / "no_such_checkpoint")]
    assert _parser().parse_args(folder).pack_files == 1
    assert _parser().parse_args(folder + ["--pack_files", "16"]).pack_files == 16
    assert "--pack_files" in _parser().format_help()
    # each refused before the options file, the checkpoint or an input is opened (none of them exists)
    for argv, word in ((folder + ["--pack_files", "4"], "needs segment_norm"),
                       (folder + ["--pack_files", "0", "--segment_norm"], "pack_files must be an int >= 1"),
                       (folder + ["--pack_files", "4", "--segment_norm", "--loudness", "-23", "--loudness_scope", "folder"], "loudness_scope 'folder'"),
                       (single + ["--pack_files", "4", "--segment_norm"], "--pack_files is an option of a folder")):
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------
# the restatement of the ragged launches against the per-clip restatement
# ------------------------------------------------------------------------------------------
def _clips(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]


@pytest.mark.parametrize("T,stride", [(8, 8), (8, 6), (8, 4), (10, 10), (10, 5), (12, 9)])
def test_ragged_restatement_is_the_per_clip_restatement(T, stride):
    shapes = [(1, 0), (2, 1), (1, T - 1), (3, T), (1, T + 1), (2, 5 * T // 2), (1, 7 * T + 3)]
    clips = _clips(shapes, T * 100 + stride)
    seg = RG.gather_ragged(clips, T, stride)
    rows, total = RG.table(clips, T, stride)
    assert seg.shape == (total, T) and total == sum(C * G.plan(L, T, 1 - stride / T)[0] for C, L in shapes)
    at = 0
    for clip in clips:
        S = RG.segments(clip.shape[1], T, stride)
        assert S == G.plan(clip.shape[1], T, 1 - stride / T)[0]
        for c in range(clip.shape[0]):
            assert np.array_equal(seg[at:at + S], G.gather(clip[c], T, stride, S))
            at += S
    assert at == total
    work = np.random.default_rng(5).standard_normal(seg.shape).astype(np.float32)
    for gain in (1.0, 0.75):
        outs = RG.stitch_ragged(work, [s[1] for s in shapes], [s[0] for s in shapes], stride, gain)
        at = 0
        for (C, L), out in zip(shapes, outs):
            S = RG.segments(L, T, stride)
            assert out.shape == (C, L)
            for c in range(C):
                want = G.stitch(work[at:at + S], stride, gain, L)
                # the same two products and one sum per sample, scaled before or behind the sum: a few float64 roundings apart
                assert np.abs(out[c] - want).max(initial=0.0) <= 2.0 ** -50 * max(1.0, np.abs(want).max(initial=0.0))
                if stride == T:
                    assert np.array_equal(out[c], want)
                at += S
        assert at == total


# ------------------------------------------------------------------------------------------
# the three parts, on an object built without a device
# ------------------------------------------------------------------------------------------
def _on_the_host(monkeypatch):
    """The four launches of the row ends -> the restatements, as float32 tensors on the host."""
    from pix2pixhdaudiosr_amd.generate import rows as resolver     # (where the four are looked up)

    def gather_ragged(clips, T, stride, S_list):
        assert [RG.segments(c.shape[1], T, stride) for c in clips] == list(S_list)
        return torch.from_numpy(RG.gather_ragged([c.numpy() for c in clips], T, stride))

    def stitch_ragged(seg, lengths, channel_counts, stride, gain):
        return [torch.from_numpy(o.astype(np.float32)) for o in RG.stitch_ragged(seg.numpy(), lengths, channel_counts, stride, gain)]

    def gather_planar(audio, T, stride, S):
        return torch.from_numpy(np.concatenate([G.gather(row, T, stride, S) for row in audio.numpy()]))

    def stitch_planar(seg, C, stride, gain, L):
        S = seg.shape[0] // C
        return torch.from_numpy(np.stack([G.stitch(seg.numpy()[c * S:(c + 1) * S], stride, gain, L) for c in range(C)]).astype(np.float32))

    monkeypatch.setattr(resolver, "segments_gather_ragged", gather_ragged)
    monkeypatch.setattr(resolver, "segments_stitch_ragged", stitch_ragged)
    monkeypatch.setattr(resolver, "segments_gather_planar", gather_planar)
    monkeypatch.setattr(resolver, "segments_stitch_planar", stitch_planar)


@pytest.mark.parametrize("batch", [1, 4, 32])
@pytest.mark.parametrize("overlap", [0.0, 0.25])
def test_a_pack_runs_the_group_function_once_per_full_group(monkeypatch, batch, overlap):
    """Six clips of 1 to 6 rows: the pack's rows are walked in ceil(sum R / batch) groups, where clip by clip each clip's rows round
    up on their own.  Every clip comes out as enhance_lr gives it alone, and last_norm is one [C, S, 2] view per clip."""
    from pix2pixhdaudiosr_amd.generate import segment_plan
    _on_the_host(monkeypatch)
    T = 8
    shapes = [(1, 0), (2, 3), (1, 2 * T + 1), (2, 3 * T - 2), (1, 5 * T), (3, 9)]
    clips = [torch.from_numpy(c) for c in _clips(shapes, 17)]
    rows = [C * segment_plan(L, T, overlap)[0] for C, L in shapes]
    many = _bare(batch, T, overlap)
    outs = many.enhance_lr_many(clips)
    assert len(many.calls) == math.ceil(sum(rows) / batch)
    assert all(tuple(g.shape) == (batch, T) for g in many.calls)                     # full groups, the fillers in the last one only
    walked = torch.cat(many.calls)
    assert bool((walked[sum(rows):] == 0).all()) and walked.shape[0] - sum(rows) < batch
    one = _bare(batch, T, overlap)
    alone = [one.enhance_lr(c) for c in clips]
    assert len(one.calls) == sum(math.ceil(r / batch) for r in rows)
    if batch > 1:
        assert len(many.calls) < len(one.calls)
    assert isinstance(many.last_norm, list) and len(many.last_norm) == len(clips)
    at = 0
    for (C, L), got, want, norm, r in zip(shapes, outs, alone, many.last_norm, rows):
        assert tuple(got.shape) == (C, L) and torch.equal(got, want)
        assert tuple(norm.shape) == (C, r // C, 2)
        assert torch.equal(norm.reshape(-1, 2), torch.stack([walked[at:at + r, 0], walked[at:at + r].sum(dim=1)], dim=1))
        at += r
    # enhance_lr is the one-clip case of the same parts: a list of one clip gives the same clip, and the planar entries
    single = _bare(batch, T, overlap)
    assert torch.equal(single.enhance_lr_many(clips[3:4])[0], alone[3])


def test_given_noise_is_taken_in_row_order(monkeypatch):
    _on_the_host(monkeypatch)
    T, batch, shape = 8, 4, (2, 3)
    sr = _bare(batch, T, 0.0)
    sr.model = SimpleNamespace(mask_noise_shape=lambda b, t: (b,) + shape)
    seen = []
    inner = sr._group_rows
    sr._group_rows = lambda seg, noise: (seen.append(noise.clone()), inner(seg, noise))[1]
    clips = [torch.ones(2, T + 1), torch.ones(1, 3 * T)]                              # 4 + 3 rows
    noise = 1.0 + torch.arange(7 * 6, dtype=torch.float32).reshape((7,) + shape)
    sr.enhance_lr_many(clips, noise=noise)
    assert [tuple(n.shape) for n in seen] == [(batch,) + shape] * 2
    assert torch.equal(torch.cat(seen)[:7], noise) and bool((seen[1][3:] == 0).all())
    with pytest.raises(ValueError, match=r"noise for rows 0\.\.3 has shape"):
        sr.enhance_lr_many(clips, noise=noise[:, :1])
