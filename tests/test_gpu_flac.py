"""The FLAC decoder on the GPU (csrc/flac.hip: p2phd_flac_decode; generate.flac_decode) against the host decoder
p2phd_flac_decode_host -- which tests/test_flac_host.py holds to the restatement -- bit for bit as float32 (exact up to 24 bits).
Every call writes its rows between canaries, with a row pitch longer than the rows.  Shapes: the lane, wave and workgroup edges of
the frame kernel (1, 2, 63, 64, 65, 130 frames), block sizes around the element-wise kernel's tile, every construct of the host
matrix once, variable block sizes from 1 to 32768 in one stream; the bounded-read case (a frame cut short and re-sealed with right
CRCs: an error path, not a fault); runs and streams; the launch counter; every refusal."""
import ctypes
import functools
import struct

import numpy as np
import pytest
import torch

import _flac_cases as K
import _flac_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 77.0
CASES = K.all_cases()
NONE = -1                                                           # P2PHD_FLAC_STATUS_NONE as an int64


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _flacio():
    from pix2pixhdaudiosr_amd.data import flacio
    return flacio


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"flac", 1 if reset else 0)


def _host(data, name="case"):
    """-> (FlacInfo, table, the host decoder's samples as float32 [C, L])."""
    f = _flacio()
    meta, table = f.index_bytes(data, name)
    pcm = f.decode_frames(data, table, 0, len(table), meta.num_channels, name)
    return meta, table, pcm.astype(np.float32) * np.float32(2.0 ** -(meta.bits_per_sample - 1))


def _call(data, table, channels, bits, L, pitch=5, slack=0, stream=None, over=None):
    """p2phd_flac_decode with the rows between canaries -> (rc, rows [C, L] as numpy, status, canaries intact)."""
    L_ = _lib()
    ld = L + pitch
    buf = torch.full((4 + channels * ld + 4,), CANARY, dtype=torch.float32, device=DEV)
    rows = buf[4:]
    raw = torch.zeros((len(data) + slack,), dtype=torch.uint8, device=DEV)
    raw[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64)).to(DEV)
    status = torch.full((1,), NONE, dtype=torch.int64, device=DEV)
    n = L_.lib().p2phd_flac_workspace_bytes(channels, ld)
    work = torch.full((max(n, 4),), 0xEE, dtype=torch.uint8, device=DEV)
    a = dict(bytes=L_.ptr(raw), nbytes=len(data), table=L_.ptr(t), nframes=len(table), channels=channels, bits=bits, out=L_.ptr(rows), ld=ld,
             work=L_.ptr(work), status=L_.ptr(status))
    a.update(over or {})
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    rc = L_.lib().p2phd_flac_decode(a['bytes'], a['nbytes'], a['table'], a['nframes'], a['channels'], a['bits'], a['out'], a['ld'], a['work'],
                                    a['status'], L_.stream_ptr() if stream is None else ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    body = got[4:4 + channels * ld].reshape(channels, ld)
    intact = bool((got[:4] == CANARY).all() and (got[-4:] == CANARY).all() and (body[:, L:] == CANARY).all())
    return rc, body[:, :L].copy(), int(status.item()), intact


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _check(data, name="case", **kw):
    meta, table, want = _host(data, name)
    rc, got, status, intact = _call(data, table, meta.num_channels, meta.bits_per_sample, meta.num_frames, **kw)
    assert rc == 0, _lib().lib().p2phd_last_error()
    assert status == NONE and intact
    assert _same_bits(got, want), name
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_construct(name):
    """Every case of the host matrix: the 64-bit sums, the long unary runs, escapes, wasted bits, the stereo assignments, every
    header code, variable block sizes from 1 to 32768 in one stream, three frames of 4096 / 4608, a short last frame."""
    _check(CASES[name]()[0], name)


@functools.lru_cache(maxsize=None)
def _frames(n, block, nch=1):
    chs = [K.signal(n * block - (block // 2 if n > 2 else 0), 16, n + c) for c in range(nch)]
    table = [dict(kind="fixed", order=2), dict(kind="verbatim"), K.lpc_spec(3, 1), dict(kind="fixed", order=0, method=1)]
    return R.make_stream(chs, 16, block, assign=R.MID_SIDE if nch == 2 else None, specs=lambda k, c: table[(k + c) % 4])[0]


@pytest.mark.parametrize("block", [16, 17])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_frame_counts(n, block):
    """Lane, wave and workgroup edges of the frame kernel (one lane per frame, 64 to a workgroup); the last frame is short."""
    assert _lib().lib().p2phd_flac_frames_per_workgroup() == 64
    _check(_frames(n, block), pitch=1 + n % 3)


def test_tile_edges():
    """Block sizes around the element-wise kernel's tile, two channels, mid/side."""
    T = _lib().lib().p2phd_flac_tile_len()
    assert T == 256
    sizes = [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3]
    chs = [K.signal(sum(sizes), 16, 1), K.signal(sum(sizes), 16, 2)]
    data, _ = R.make_stream(chs, 16, None, variable=True, sizes=sizes, assign=R.MID_SIDE, specs=lambda k, c: [dict(kind="verbatim"), dict(kind="fixed", order=1)][c])
    _check(data)


def test_cut_frame_is_reported_not_overrun():
    """Frame 2 lost its last 5 bytes and was sealed again with a correct CRC-16: the index passes it, its lane runs out of bits inside
    its own byte range, writes zeros, and reports itself; every other frame and the canaries are intact.  (The byte buffer has a
    whole frame of slack behind it.)"""
    chs = [K.signal(5 * 32, 16, 1), K.signal(5 * 32, 16, 2)]
    spec = [dict(kind="fixed", order=2), dict(kind="fixed", order=1)]
    frames = [R.encode_frame([c[32 * k:32 * k + 32] for c in chs], 16, k, specs=spec, cut=5 if k == 2 else 0) for k in range(5)]
    data = R.encode_stream(frames, 44100, 2, 16, 160, 32, 32)
    f = _flacio()
    meta, table = f.index_bytes(data)
    assert table[:, 1].tolist() == [len(x) for x in frames]
    with pytest.raises(ValueError, match="frame 2 at byte"):
        f.decode_frames(data, table, 0, 5, 2)
    want = np.array(chs, dtype=np.float32) * np.float32(2.0 ** -15)
    want[:, 64:96] = 0.0
    rc, got, status, intact = _call(data, table, 2, 16, 160, slack=max(len(x) for x in frames))
    assert rc == 0 and intact
    assert status >> 8 == 2 and status & 255 in (1, 4)
    assert _same_bits(got, want)
    # two bad frames: the lowest is reported
    frames[4] = R.encode_frame([c[128:160] for c in chs], 16, 4, specs=spec, cut=7)
    data = R.encode_stream(frames, 44100, 2, 16, 160, 32, 32)
    meta, table = f.index_bytes(data)
    want[:, 128:] = 0.0
    rc, got, status, intact = _call(data, table, 2, 16, 160, slack=max(len(x) for x in frames))
    assert rc == 0 and intact and status >> 8 == 2 and _same_bits(got, want)
    from pix2pixhdaudiosr_amd.generate import flac_decode
    raw = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    with pytest.raises(ValueError, match="frame 2 does not decode"):
        flac_decode(raw, table, meta)
    out, st = flac_decode(raw, table, meta, check=False)
    assert int(st.item()) >> 8 == 2 and _same_bits(out.cpu().numpy(), want)


@pytest.mark.parametrize("spec", [dict(type_bits=2), dict(type_bits=13), dict(pad_bit=1), dict(method_field=2),
                                  dict(kind="lpc", coefs=[3, -1], precision=4, shift=-1)])
def test_reserved_subframe_codes_are_reason_2(spec):
    """A reserved subframe type, the padding bit, a reserved residual method and a negative LPC shift in frame 1 of 3: frames the index
    passes (their CRCs are right); the lane writes zeros and reports frame 1 with reason 2, the other frames are intact."""
    ch = K.signal(48, 16, 8)
    base = dict(kind="fixed", order=2)
    frames = [R.encode_frame([ch[16 * k:16 * k + 16]], 16, k, specs=[dict(base, **spec) if k == 1 else base]) for k in range(3)]
    data = R.encode_stream(frames, 44100, 1, 16, 48, 16, 16)
    meta, table = _flacio().index_bytes(data)
    want = np.array([ch], dtype=np.float32) * np.float32(2.0 ** -15)
    want[:, 16:32] = 0.0
    rc, got, status, intact = _call(data, table, 1, 16, 48, slack=64)
    assert rc == 0 and intact and status == (1 << 8 | 2) and _same_bits(got, want)


def test_more_frames_than_workgroups_of_the_elementwise_kernel():
    """The element-wise kernel has at most 2^20 workgroups, each walking frames b, b + 2^20, ...: a table of 2^20 + 7 rows that point
    at the four one-sample frames of a small stream in turn, each row with a column of its own."""
    ch = K.signal(4, 16, 4)
    data, _ = R.make_stream([ch], 16, 1, specs=[dict(kind="verbatim")])
    meta, table = _flacio().index_bytes(data)
    n = (1 << 20) + 7
    big = np.tile(table, (-(-n // 4), 1))[:n].copy()
    big[:, 2] = np.arange(n)
    rc, got, status, intact = _call(data, big, 1, 16, n)
    assert rc == 0 and intact and status == NONE
    want = (np.tile(np.array(ch, dtype=np.float32), -(-n // 4))[:n] * np.float32(2.0 ** -15))[None]
    assert _same_bits(got, want)


def test_rows_that_do_not_fit_are_reported_and_not_written():
    """A table row whose bytes lie outside the buffer, or whose samples lie outside the rows: reason 5, nothing of it is written."""
    data = _frames(5, 16)
    meta, table, want = _host(data)
    for col, value in ((1, len(data)), (0, len(data) - 3), (3, 4096), (2, -16)):
        bad = table.copy()
        bad[3, col] = value
        rc, got, status, intact = _call(data, bad, 1, 16, meta.num_frames)
        assert rc == 0 and intact and status == (3 << 8 | 5), (col, value)
        keep = np.ones(meta.num_frames, dtype=bool)
        keep[48:64] = False
        assert _same_bits(got[:, keep], want[:, keep]) and (got[:, ~keep] == CANARY).all()
    bad = table.copy()
    bad[1, 4] = 8                                                   # a stereo assignment in a mono stream: zeros, reason 5
    rc, got, status, intact = _call(data, bad, 1, 16, meta.num_frames)
    assert rc == 0 and intact and status == (1 << 8 | 5) and (got[:, 16:32] == 0).all() and _same_bits(got[:, 32:], want[:, 32:])


def test_runs_and_streams_repeat_the_bits():
    data = CASES["matrix-3ch-20bit"]()[0]
    meta, table, want = _host(data)
    side = torch.cuda.Stream()
    a = _call(data, table, 3, 20, meta.num_frames)[1]
    b = _call(data, table, 3, 20, meta.num_frames, pitch=64)[1]
    c = _call(data, table, 3, 20, meta.num_frames, stream=side)[1]
    assert _same_bits(a, want) and _same_bits(b, want) and _same_bits(c, want)


def test_launch_counter_and_no_op():
    data = _frames(2, 16)
    meta, table, _ = _host(data)
    _count(reset=True)
    _call(data, table, 1, 16, meta.num_frames)
    assert _count() == 2                                            # the frame kernel and the element-wise kernel
    rc, got, status, intact = _call(data, table[:0], 1, 16, meta.num_frames)
    assert rc == 0 and intact and status == NONE and (got == CANARY).all() and _count() == 2       # nframes = 0 launches nothing
    _call(data, table, 1, 16, meta.num_frames)
    assert _count(reset=True) == 4 and _count() == 0


def test_refusals():
    data = _frames(2, 16)
    meta, table, _ = _host(data)
    null = ctypes.c_void_p(None)
    for over, text in ((dict(channels=0), b"channels"), (dict(channels=9), b"channels"), (dict(bits=10), b"bits per sample"), (dict(bits=32), b"bits per sample"),
                       (dict(nframes=-1), b"nframes"), (dict(nframes=1 << 31), b"nframes"), (dict(nbytes=-1), b"nbytes"), (dict(ld=-1), b"ld"),
                       (dict(bytes=null), b"null"), (dict(table=null), b"null"), (dict(out=null), b"null"), (dict(work=null), b"null"),
                       (dict(status=null), b"null")):
        before = _count()
        rc, got, status, intact = _call(data, table, 1, 16, meta.num_frames, over=over)
        assert rc != 0 and intact and (got == CANARY).all() and status == NONE and _count() == before, over
        assert text in _lib().lib().p2phd_last_error(), (over, _lib().lib().p2phd_last_error())
    buf = torch.zeros((64,), dtype=torch.uint8, device=DEV)
    rc = _call(data, table, 1, 16, meta.num_frames, over=dict(out=ctypes.c_void_p(buf.data_ptr() + 2)))[0]
    assert rc != 0 and b"aligned" in _lib().lib().p2phd_last_error()
    assert _lib().lib().p2phd_flac_workspace_bytes(0, 10) == 0 and _lib().lib().p2phd_flac_workspace_bytes(9, 10) == 0
    assert _lib().lib().p2phd_flac_workspace_bytes(2, 10) == 80


def test_op_equals_load(tmp_path):
    """generate.flac_decode on the file's bytes and index: the tensor flacio.load returns."""
    from pix2pixhdaudiosr_amd.generate import flac_decode
    f = _flacio()
    for name in ("stereo-24bit-10", "matrix-8ch-12bit", "variable-small"):
        data = CASES[name]()[0]
        p = str(tmp_path / (name + ".flac"))
        open(p, "wb").write(data)
        want, rate = f.load(p)
        got, meta, table = f.read_file(p)
        raw = torch.frombuffer(bytearray(got), dtype=torch.uint8).to(DEV)
        out = flac_decode(raw, table, meta)
        assert out.dtype == torch.float32 and torch.equal(out.cpu(), want)
        assert torch.equal(flac_decode(raw, torch.from_numpy(table.copy()).to(DEV), meta).cpu(), want)
    with pytest.raises(ValueError, match="table"):
        flac_decode(raw, table[:, :5], meta)
