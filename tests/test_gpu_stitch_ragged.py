"""The ragged gather and stitch on the GPU (csrc/stitch.hip: p2phd_segments_gather_ragged, p2phd_segments_stitch_ragged), through the
C ABI and through the wrappers of generate/ops.py: every clip row is compared as int32, bit for bit, with what the planar entry
gives on that clip alone (C = 1, on a copy of its own, so 16-byte aligned whatever the row's own base is).  Outputs sit between
canaries, prefilled with a sentinel.  A refused call launches nothing: the family's counter, the payload and the canaries stay."""
import ctypes

import numpy as np
import pytest
import torch

import _exact as E
import _long as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT32 = 0xA5A5A5A5                                                  # a payload prefilled with E.GUARD_BYTE, read as uint32
GAIN = 0.75


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _count():
    return _lib().lib().p2phd_launch_count(b"stitch", 0)


def _vp(p):
    return ctypes.c_void_p(int(p))


def _segments(L, T, stride):
    return max(1, -((T - stride - L) // stride))


def _lengths(T):
    return [0, 1, T - 1, T, T + 1, 5 * T // 2, 7 * T + 3]


def _table(rows):
    """[(address, L, S), ..] -> (the N x 4 int64 table on the host, the segment rows it closes at)."""
    t = np.zeros((len(rows), 4), dtype=np.int64)
    at = 0
    for j, (addr, L, S) in enumerate(rows):
        t[j] = (addr, L, S, at)
        at += S
    return t, at


def _table_dev(n):
    want = _lib().lib().p2phd_segments_ragged_table_bytes(n)
    assert want == 32 * n
    return torch.zeros((want,), dtype=torch.uint8, device=DEV)


def _gather(table, total, T, stride, seg_ptr, n=None):
    """The raw entry -> its return code."""
    L = _lib()
    n = len(table) if n is None else n
    dev = _table_dev(max(len(table), 1))
    return L.lib().p2phd_segments_gather_ragged(_vp(table.ctypes.data), n, T, stride, total, _vp(seg_ptr), _vp(dev.data_ptr()), L.stream_ptr())


def _stitch(seg_ptr, table, total, T, stride, gain, n=None):
    L = _lib()
    n = len(table) if n is None else n
    dev = _table_dev(max(len(table), 1))
    return L.lib().p2phd_segments_stitch_ragged(_vp(seg_ptr), _vp(table.ctypes.data), n, total, T, stride, gain, _vp(dev.data_ptr()), L.stream_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _audio(n, seed):
    return torch.from_numpy(K.hashed_floats(max(n, 1), seed=seed)[:n]).to(DEV)


def _check_rows(rows_audio, T, stride, what):
    """rows_audio: 1-D float32 views on the GPU, one per clip row, at whatever base they have.  Runs the ragged gather into a guarded
    seg, compares every row's segments with the planar entry on a copy of that row alone; fills seg with other data, runs the ragged
    stitch into one guarded output per row -- at the row's own misalignment -- and compares with the planar stitch of those rows."""
    from pix2pixhdaudiosr_amd.generate import segments_gather_planar, segments_stitch_planar
    rows = [(a.data_ptr() if a.numel() else 0, a.numel(), _segments(a.numel(), T, stride)) for a in rows_audio]
    table, total = _table(rows)
    g = E.Guarded(total * T * 4, DEV, E.GUARD_BYTE)
    before = _count()
    assert _gather(table, total, T, stride, g.ptr()) == 0, _lib().lib().p2phd_last_error()
    assert _count() == before + 1                                     # one launch whatever N is
    torch.cuda.synchronize()
    assert not g.touched(), (what, g.touched())
    seg = g.view(torch.float32, (total, T))
    for j, (a, (_, L, S, row0)) in enumerate(zip(rows_audio, table.tolist())):
        want = segments_gather_planar(a.clone()[None], T, stride, S)
        assert torch.equal(_bits(seg[row0:row0 + S]), _bits(want)), (what, "gather row", j, L, S)
    # the stitch: the gathered rows would only copy back, so the segments are other data
    work = _audio(total * T, seed=total + T).reshape(total, T)
    outs, srows = [], []
    for a, (_, L, S) in zip(rows_audio, rows):
        shift = (a.data_ptr() % 16) if a.numel() else 0               # the output at the input's own misalignment
        o = E.Guarded(L * 4 + shift, DEV, E.GUARD_BYTE)
        outs.append((o, shift))
        srows.append((o.ptr() + shift if L else 0, L, S))
    stable, _ = _table(srows)
    before = _count()
    assert _stitch(work.data_ptr(), stable, total, T, stride, GAIN) == 0, _lib().lib().p2phd_last_error()
    assert _count() == before + (1 if any(L for _, L, _ in rows) else 0)
    torch.cuda.synchronize()
    for j, ((o, shift), (_, L, S, row0)) in enumerate(zip(outs, stable.tolist())):
        assert not o.touched(), (what, "stitch row", j, o.touched())
        got = o.bytes[shift:].view(torch.int32)
        assert bool((o.bytes[:shift] == E.GUARD_BYTE).all())
        want = segments_stitch_planar(work[row0:row0 + S].clone(), 1, stride, GAIN, L)
        assert torch.equal(got, _bits(want).reshape(-1)), (what, "stitch row", j, L, S)


# ------------------------------------------------------------------------------------------
# every clip row is the planar entry on that clip alone
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3, 7])
@pytest.mark.parametrize("T,stride", [(8, 8), (8, 6), (8, 4), (10, 10), (10, 5), (64, 64), (64, 48), (64, 32)])
def test_rows_are_the_planar_entry_on_each_clip_alone(T, stride, N):
    """T 8 and 64 with strides that are multiples of 4 take the 16-byte paths, T 10 and stride 6 the scalar ones.  Every length of
    {0, 1, T - 1, T, T + 1, 2.5 T, 7 T + 3} appears at every N: N = 1 runs seven launches (and is the planar entry itself), N = 3
    three, N = 7 one."""
    lengths = _lengths(T)
    for start in range(0, len(lengths), N):
        mine = [lengths[(start + j) % len(lengths)] for j in range(N)]
        rows = [_audio(L, seed=100 * T + L + j) for j, L in enumerate(mine)]     # each an allocation of its own: aligned
        _check_rows(rows, T, stride, (T, stride, N, mine))


@pytest.mark.parametrize("T,stride", [(8, 8), (8, 4), (64, 48), (10, 5)])
def test_channels_of_odd_length_tensors_are_unaligned_rows(T, stride):
    """Rows that are the channels of [2, L] tensors with odd L: row 1 starts 4 * L bytes in, off the 16-byte grid, and takes the
    scalar path beside an aligned row 0 in the same launch.  The reference runs on an aligned copy: access width changes no bit."""
    rows = []
    for k, L in enumerate(x for x in _lengths(T) + [2 * T + 1] if x % 2 == 1):
        clip = _audio(2 * L, seed=7 * T + L).reshape(2, L)
        assert clip[1].data_ptr() % 16 != 0 or L % 4 == 0
        rows += [clip[0], clip[1]]
    assert any(r.data_ptr() % 16 for r in rows)
    _check_rows(rows, T, stride, (T, stride, "odd"))


def test_a_row_past_the_cap_beside_a_one_sample_row():
    """One row long enough for the grid-stride loops to take a third trip (asked of p2phd_stream_grid, not assumed), a one-sample row
    on either side of it: the short rows' surplus workgroups leave, the long row's walk the rest."""
    L = _lib().lib()
    T, stride = 4096, 3072
    unit = K.stream_grid(L, "segments_stitch_ragged", 0, 1 << 30)[1]
    long_len = 2 * unit + unit // 2 + 2 * 1237 + 1
    for family, work in (("segments_stitch_ragged", long_len), ("segments_gather_ragged", _segments(long_len, T, stride) * T)):
        rc, u, wanted, used = K.stream_grid(L, family, 0, work, 3)
        assert rc == 0 and used < wanted and work > 2 * u and u == unit, (family, work, u, wanted, used)
    _check_rows([_audio(1, seed=1), _audio(long_len, seed=2), _audio(1, seed=3)], T, stride, "long")


def test_stream_grid_of_the_family():
    L = _lib().lib()
    for family in ("segments_gather_ragged", "segments_stitch_ragged"):
        assert K.stream_grid(L, family, 0, 100) == (0, 1024, 1, 1)
        assert K.stream_grid(L, family, 0, 1024 * 1024, 7) == (0, 1024 * 1024, 1024, 1024)         # at the edge: one trip
        assert K.stream_grid(L, family, 0, 1024 * 1024 + 1, 7) == (0, 1024 * 1024, 1025, 1024)     # one more quad: it loops
        assert K.stream_grid(L, family, 0, 1 << 34, 65535)[3] == 1024                              # the cap is a row's, whatever N


# ------------------------------------------------------------------------------------------
# the wrappers
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,stride", [(8, 6), (64, 48)])
def test_wrappers_are_the_planar_wrappers_clip_by_clip(T, stride):
    from pix2pixhdaudiosr_amd.generate import segments_gather_planar, segments_gather_ragged, segments_stitch_planar, segments_stitch_ragged
    shapes = [(1, 0), (2, 1), (1, T), (2, 2 * T + 1), (3, 7 * T + 3), (2, 0)]
    clips = [_audio(C * L, seed=31 * C + L).reshape(C, L) for C, L in shapes]
    S_list = [_segments(L, T, stride) for _, L in shapes]
    before = _count()
    seg = segments_gather_ragged(clips, T, stride, S_list)
    assert _count() == before + 1 and tuple(seg.shape) == (sum(C * S for (C, _), S in zip(shapes, S_list)), T)
    work = _audio(seg.numel(), seed=9).reshape(seg.shape)
    before = _count()
    outs = segments_stitch_ragged(work, [L for _, L in shapes], [C for C, _ in shapes], stride, GAIN)
    assert _count() == before + 1
    at = 0
    for clip, (C, L), S, out in zip(clips, shapes, S_list, outs):
        assert torch.equal(_bits(seg[at:at + C * S]), _bits(segments_gather_planar(clip, T, stride, S)))
        assert tuple(out.shape) == (C, L)
        assert torch.equal(_bits(out), _bits(segments_stitch_planar(work[at:at + C * S].clone(), C, stride, GAIN, L)))
        at += C * S
    with pytest.raises(ValueError, match=r"segments_stitch_ragged: the clips take"):
        segments_stitch_ragged(work[:-1], [L for _, L in shapes], [C for C, _ in shapes], stride, GAIN)
    with pytest.raises(ValueError, match=r"segments_gather_ragged: expected as many"):
        segments_gather_ragged(clips, T, stride, S_list[:-1])


def test_an_empty_clip_gathers_one_zero_row_and_stitches_nothing():
    from pix2pixhdaudiosr_amd.generate import segments_gather_ragged, segments_stitch_ragged
    T, stride = 8, 6
    empty, some = torch.zeros((1, 0), device=DEV), _audio(5, seed=4).reshape(1, 5)
    seg = segments_gather_ragged([empty, some], T, stride, [1, 1])
    assert tuple(seg.shape) == (2, T) and bool((seg[0] == 0).all()) and torch.equal(seg[1, :5], some[0]) and bool((seg[1, 5:] == 0).all())
    outs = segments_stitch_ragged(seg, [0, 5], [1, 1], stride, 1.0)
    assert tuple(outs[0].shape) == (1, 0) and torch.equal(outs[1], some)
    before = _count()
    assert [tuple(o.shape) for o in segments_stitch_ragged(seg, [0, 0], [1, 1], stride, 1.0)] == [(1, 0), (1, 0)]
    assert _count() == before                                         # every clip empty: nothing to write, nothing launched


def test_two_runs_and_a_side_stream_give_the_same_bits():
    from pix2pixhdaudiosr_amd.generate import segments_gather_ragged, segments_stitch_ragged
    T, stride = 64, 48
    shapes = [(2, 7 * T + 3), (1, 1), (2, 5 * T // 2 + 1), (1, 40 * T)]
    clips = [_audio(C * L, seed=C + L).reshape(C, L) for C, L in shapes]
    S_list = [_segments(L, T, stride) for _, L in shapes]

    def run():
        seg = segments_gather_ragged(clips, T, stride, S_list)
        return seg, segments_stitch_ragged(seg, [L for _, L in shapes], [C for C, _ in shapes], stride, GAIN)

    first, again = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for other in (again, aside):
        assert torch.equal(_bits(other[0]), _bits(first[0]))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(other[1], first[1]))


# ------------------------------------------------------------------------------------------
# refusals: on the host, before anything is launched
# ------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing():
    L = _lib().lib()
    T, stride = 8, 6
    audio = [_audio(n, seed=n) for n in (5, 20, 9)]
    rows = [(a.data_ptr(), a.numel(), _segments(a.numel(), T, stride)) for a in audio]
    good, total = _table(rows)
    seg = E.Guarded(total * T * 4, DEV, E.GUARD_BYTE)
    outs = [E.Guarded(a.numel() * 4, DEV, E.GUARD_BYTE) for a in audio]
    sgood, _ = _table([(o.ptr(), n, S) for o, (_, n, S) in zip(outs, rows)])

    def broken(table, j, col, value):
        t = table.copy()
        t[j, col] = value
        return t

    big = np.zeros((1, 4), dtype=np.int64)
    cases = []
    for name, table, base in (("gather", good, rows), ("stitch", sgood, None)):
        cases += [(name, "row0 of the first row", broken(table, 0, 3, 1), total, T, stride, None),
                  (name, "a gap in the chain", broken(table, 1, 3, int(table[1, 3]) + 1), total, T, stride, None),
                  (name, "an overlap in the chain", broken(table, 2, 3, int(table[2, 3]) - 1), total, T, stride, None),
                  (name, "the chain closes short of rows", table, total + 1, T, stride, None),
                  (name, "the chain closes beyond rows", table, total - 1, T, stride, None),
                  (name, "a null address with L > 0", broken(table, 1, 0, 0), total, T, stride, None),
                  (name, "an address that is no float's", broken(table, 1, 0, int(table[1, 0]) + 2), total, T, stride, None),
                  (name, "L < 0", broken(table, 0, 1, -1), total, T, stride, None),
                  (name, "S < 1", broken(table, 0, 2, 0), total, T, stride, None),
                  (name, "N = 0", table, total, T, stride, 0),
                  (name, "N > 65535", big, total, T, stride, 65536),
                  (name, "T < 1", table, total, 0, 0, None)]
    cases += [("gather", "stride 0", good, total, T, 0, None), ("gather", "stride > T", good, total, T, T + 1, None),
              ("stitch", "an overlap above T / 2", sgood, total, T, T // 2 - 1, None), ("stitch", "stride > T", sgood, total, T, T + 1, None),
              ("stitch", "L beyond the span", broken(sgood, 0, 1, (int(sgood[0, 2]) - 1) * stride + T + 1), total, T, stride, None)]
    before = _count()
    for name, what, table, rows_arg, t, s, n in cases:
        if name == "gather":
            rc = _gather(table, rows_arg, t, s, seg.ptr(), n)
        else:
            rc = _stitch(seg.ptr(), table, rows_arg, t, s, GAIN, n)
        assert rc == -1 and L.p2phd_last_error(), (name, what, rc)     # (P2PHD_EINVAL)
    # a null table, a null device buffer, a null seg
    lib = _lib()
    dev = _table_dev(3)
    assert L.p2phd_segments_gather_ragged(None, 3, T, stride, total, _vp(seg.ptr()), _vp(dev.data_ptr()), lib.stream_ptr()) == -1
    assert L.p2phd_segments_gather_ragged(_vp(good.ctypes.data), 3, T, stride, total, _vp(seg.ptr()), None, lib.stream_ptr()) == -1
    assert L.p2phd_segments_gather_ragged(_vp(good.ctypes.data), 3, T, stride, total, None, _vp(dev.data_ptr()), lib.stream_ptr()) == -1
    assert L.p2phd_segments_stitch_ragged(None, _vp(sgood.ctypes.data), 3, total, T, stride, GAIN, _vp(dev.data_ptr()), lib.stream_ptr()) == -1
    assert L.p2phd_segments_ragged_table_bytes(0) == 0 and L.p2phd_segments_ragged_table_bytes(65536) == 0
    torch.cuda.synchronize()
    assert _count() == before
    for g in [seg] + outs:
        assert not g.touched() and bool((g.bytes == E.GUARD_BYTE).all())
    # and the tables as they were meant run
    assert _gather(good, total, T, stride, seg.ptr()) == 0 and _stitch(seg.ptr(), sgood, total, T, stride, 1.0) == 0
    torch.cuda.synchronize()
    assert _count() == before + 2
    for a, o in zip(audio, outs):
        assert not o.touched() and torch.equal(o.bytes.view(torch.float32), a)       # gain 1, gathered and stitched: the clip again
