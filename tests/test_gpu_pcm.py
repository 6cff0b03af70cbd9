"""The PCM codec kernels (csrc/pcm.hip) and the planar gather / stitch (csrc/stitch.hip) on the GPU: decode against
wavio.load and encode against wavio.save / the numpy restatement (tests/_pcm_ref.py), bit for bit, at every byte alignment
of the payload and with the output between canaries; the planar entries against the single-row ones, row by row."""
import ctypes

import numpy as np
import pytest
import torch

import _pcm_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                                                      # bytes of sentinel on either side, as _ops._GUARD
SENTINEL = 0xA5


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _guarded(nbytes):
    """(whole allocation, the nbytes in its middle), everything filled with the sentinel."""
    raw = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD:GUARD + nbytes]


def _untouched(raw, nbytes):
    return bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[GUARD + nbytes:] == SENTINEL).all())


def _stream():
    return _lib().stream_ptr()


# ------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.FORMATS))
@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_decode_is_wavio_load(tmp_path, name, channels):
    from pix2pixhdaudiosr_amd.data import wavio
    L = _lib()
    tag, bits, code = P.FORMATS[name]
    for frames in (0, 1, 5, 4097):
        pay = P.payload(name, frames, channels)
        path = str(tmp_path / f"{frames}.wav")
        with open(path, "wb") as f:
            f.write(P.wav_bytes(pay, 48000, channels, name, extensible=frames == 5))
        want = wavio.load(path)[0].numpy()
        assert np.array_equal(want.view(np.uint32), P.decode(pay, channels, name).view(np.uint32))
        ld = frames + 3
        for offset in (0, 1, 2, 3):
            big = torch.full((len(pay) + 64,), 0x5A, dtype=torch.uint8, device=DEV)
            assert big.data_ptr() % 16 == 0
            if pay:
                big[offset:offset + len(pay)] = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
            raw, mid = _guarded(channels * ld * 4)
            L.check(L.lib().p2phd_pcm_decode(ctypes.c_void_p(big.data_ptr() + offset), frames, channels, code,
                                             ctypes.c_void_p(mid.data_ptr()), ld, _stream()), "pcm_decode")
            torch.cuda.synchronize()
            out = mid.cpu().numpy().view(np.uint32).reshape(channels, ld)
            assert np.array_equal(out[:, :frames], want.view(np.uint32)), (name, channels, frames, offset)
            assert (out[:, frames:] == 0xA5A5A5A5).all()              # the rest of a row is not written
            assert _untouched(raw, channels * ld * 4)


def test_decode_wrapper_and_errors(tmp_path):
    from pix2pixhdaudiosr_amd.generate import pcm_decode
    L = _lib()
    pay = P.payload("s24", 100, 2)
    dev = torch.frombuffer(bytearray(b"\0" + pay), dtype=torch.uint8).to(DEV)[1:]      # storage offset of one byte
    got = pcm_decode(dev, 100, 2, 1, 24)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), P.decode(pay, 2, "s24").view(np.uint32))
    with pytest.raises(ValueError, match="unsupported"):
        pcm_decode(dev, 100, 2, 1, 12)
    with pytest.raises(ValueError, match="do not hold"):
        pcm_decode(dev, 101, 2, 1, 24)
    with pytest.raises(L.P2PHDError):
        pcm_decode(dev.cpu(), 100, 2, 1, 24)
    out = torch.zeros(8, device=DEV)
    for args, text in (((4, 0, 1, 4), b"channels"), ((4, 1, 9, 4), b"format"), ((4, 1, 1, 3), b"ld"), ((-1, 1, 1, 4), b"frames")):
        frames, ch, fmt, ld = args
        rc = L.lib().p2phd_pcm_decode(L.ptr(dev), frames, ch, fmt, L.ptr(out), ld, _stream())
        assert rc != 0 and text in L.lib().p2phd_last_error()


# ------------------------------------------------------------------------------------------
# encode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", ["pcm16", "pcm24", "float32"])
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_encode_is_wavio_save(tmp_path, encoding, channels):
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import pcm_encode
    L = _lib()
    tag, bits, code = P.ENCODINGS[encoding]
    for frames in (1, 5, 4097, 1231):
        x = P.encode_input(frames, channels)
        want = P.encode(x, encoding)
        path = str(tmp_path / "a.wav")
        wavio.save(path, torch.from_numpy(x), 48000, encoding=encoding)
        with open(path, "rb") as f:
            assert f.read()[44:44 + len(want)] == want            # for pcm16: the bytes wavio.save has always written
        ld = frames + 5
        planar = torch.full((channels, ld), float("nan"), device=DEV)
        planar[:, :frames] = torch.from_numpy(x).to(DEV)
        nbytes = frames * channels * bits // 8
        for offset in (0, 1):                                     # an output that is not aligned to its sample size
            raw, mid = _guarded(nbytes + offset)
            L.check(L.lib().p2phd_pcm_encode(L.ptr(planar), frames, channels, ld, code, ctypes.c_void_p(mid.data_ptr() + offset),
                                             _stream()), "pcm_encode")
            torch.cuda.synchronize()
            assert mid[offset:].cpu().numpy().tobytes() == want, (encoding, channels, frames, offset)
            assert _untouched(raw, nbytes + offset) and (offset == 0 or int(mid[0]) == SENTINEL)
        got = pcm_encode(planar[:, :frames], encoding)            # the wrapper takes the row pitch from the view
        assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want


def test_encode_nan_is_zero_and_errors():
    from pix2pixhdaudiosr_amd.generate import pcm_encode
    L = _lib()
    x = torch.tensor([[float("nan"), 0.5, -float("nan")], [0.25, float("nan"), -1.0]], device=DEV)
    assert np.frombuffer(pcm_encode(x, "pcm16").cpu().numpy().tobytes(), dtype="<i2").tolist() == [0, 8192, 16384, 0, 0, -32768]
    b = pcm_encode(x, "pcm24").cpu().numpy().reshape(-1, 3)
    assert b[0].tolist() == [0, 0, 0] and b[3].tolist() == [0, 0, 0] and b[1].tolist() == [0, 0, 0x20] and b[5].tolist() == [0, 0, 0x80]
    nan_bits = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32).to(DEV)[None]
    assert pcm_encode(nan_bits, "float32").cpu().numpy().view("<u4").tolist() == [0x7FC12345]
    with pytest.raises(ValueError, match="encoding"):
        pcm_encode(x, "pcm8")
    with pytest.raises(L.P2PHDError):
        pcm_encode(x.cpu(), "pcm16")
    out = torch.zeros(64, dtype=torch.uint8, device=DEV)
    for fmt in (0, 3, 5, 7):                                      # formats the encoder does not write
        assert L.lib().p2phd_pcm_encode(L.ptr(x), 3, 2, 3, fmt, L.ptr(out), _stream()) != 0
        assert b"format" in L.lib().p2phd_last_error()
    assert L.lib().p2phd_pcm_encode(L.ptr(x), 3, 2, 2, 1, L.ptr(out), _stream()) != 0 and b"ld" in L.lib().p2phd_last_error()


def _both_entries(planar, frames, channels, ld, code, nbytes):
    """The payload of p2phd_pcm_encode and of p2phd_pcm_encode_ex with a null gain and no dither, each between canaries."""
    L = _lib()
    got = []
    for ex in (False, True):
        raw, mid = _guarded(nbytes)
        tail = (L.ptr(mid), _stream())
        if ex:
            L.check(L.lib().p2phd_pcm_encode_ex(L.ptr(planar), frames, channels, ld, code, None, 0, 0, 0, *tail), "pcm_encode_ex")
        else:
            L.check(L.lib().p2phd_pcm_encode(L.ptr(planar), frames, channels, ld, code, *tail), "pcm_encode")
        torch.cuda.synchronize()
        assert _untouched(raw, nbytes)
        got.append(mid.cpu().numpy().tobytes())
    return got


@pytest.mark.parametrize("encoding", ["pcm16", "pcm24"])
def test_both_entries_on_the_quantiser_edges(encoding):
    """One kernel serves both entries: on every value at which clamping before or after the rounding could differ
    (P.quantise_edges), as one row and as three rows with a row pitch, both write the bytes of the restatement."""
    tag, bits, code = P.ENCODINGS[encoding]
    edges = P.quantise_edges(bits)
    n = len(edges) // 3 * 3
    for channels, pad in ((1, 0), (3, 7)):
        frames = n // channels
        x = np.ascontiguousarray(edges[:n].reshape(channels, frames))
        planar = torch.full((channels, frames + pad), float("nan"), device=DEV)
        planar[:, :frames] = torch.from_numpy(x).to(DEV)
        want = P.encode(x, encoding)
        for got in _both_entries(planar, frames, channels, frames + pad, code, n * bits // 8):
            assert got == want, (encoding, channels)


def test_both_entries_copy_float32_bits():
    """NaNs with payloads, +-inf, denormals: float32 without a gain is a bit copy through either entry."""
    x = P.quantise_edges(16)[-2048:].reshape(2, 1024)
    assert len(np.unique(x.view(np.uint32)[np.isnan(x)])) == 6 and np.isinf(x).sum() == 2 and (np.abs(x[x != 0]) < 1e-38).sum() == 4
    planar = torch.from_numpy(x.copy()).to(DEV)
    for got in _both_entries(planar, 1024, 2, 1024, P.ENCODINGS["float32"][2], x.size * 4):
        assert np.array_equal(np.frombuffer(got, dtype="<u4"), np.ascontiguousarray(x.T).view(np.uint32).ravel())


def test_pcm_launch_family():
    from pix2pixhdaudiosr_amd.generate import pcm_decode, pcm_encode
    lib = _lib().lib()
    lib.p2phd_launch_count(b"pcm", 1)
    x = pcm_decode(torch.zeros(64, dtype=torch.uint8, device=DEV), 8, 2, 1, 32)
    assert lib.p2phd_launch_count(b"pcm", 0) == 1
    pcm_encode(x, "pcm24")
    assert lib.p2phd_launch_count(b"pcm", 1) == 2
    assert pcm_decode(torch.zeros(0, dtype=torch.uint8, device=DEV), 0, 2, 1, 16).shape == (2, 0)
    assert lib.p2phd_launch_count(b"pcm", 1) == 0                 # nothing to do: no launch


# ------------------------------------------------------------------------------------------
# planar gather / stitch
# ------------------------------------------------------------------------------------------
# the SHAPES of tests/test_gpu_generate.py: (S, T, V, samples short of the full span)
SHAPES = [(1, 64, 0, 0), (1, 37, 0, 5), (3, 64, 0, 0), (4, 64, 32, 0), (5, 37, 18, 11), (3, 50, 7, 3), (6, 992, 248, 500),
          (2, 4064, 1, 0), (4, 33, 16, 0)]


def test_shapes_are_those_of_the_single_row_suite():
    import test_gpu_generate as G
    assert SHAPES == G.SHAPES


@pytest.mark.parametrize("S,T,V,short", SHAPES)
@pytest.mark.parametrize("C", [1, 2, 5])
def test_planar_rows_are_the_single_row_entries(S, T, V, short, C):
    from pix2pixhdaudiosr_amd.generate import segments_gather, segments_gather_planar, segments_stitch, segments_stitch_planar
    stride = T - V
    L = (S - 1) * stride + T - short
    gen = torch.Generator().manual_seed(S * 1000 + T + V + C)
    gain = float(np.float32(np.sqrt(5.0)))
    for pad in (0, 3, 4):                                         # row pitch L, odd and 16-byte-friendly
        ld = L + pad
        buf = torch.randn(C, ld, generator=gen).to(DEV)
        audio = buf[:, :L]
        seg = segments_gather_planar(audio, T, stride, S)
        assert tuple(seg.shape) == (C * S, T)
        for c in range(C):
            assert torch.equal(seg[c * S:(c + 1) * S], segments_gather(audio[c].contiguous(), T, stride, S)), (c, pad)
        y = torch.randn(C * S, T, generator=gen).to(DEV)          # neighbours disagree inside the overlaps
        for L_out in sorted({L, max(L - 1, 0), (S - 1) * stride + T}):
            ldo = L_out + pad
            out = segments_stitch_planar(y, C, stride, gain, L_out, ld=ldo)
            assert tuple(out.shape) == (C, L_out) and (out.stride(0) == ldo or C == 1)
            for c in range(C):
                want = segments_stitch(y[c * S:(c + 1) * S].contiguous(), stride, gain, L_out)
                assert torch.equal(out[c].view(torch.int32), want.view(torch.int32)), (c, pad, L_out)


def test_planar_writes_stay_inside_their_rows():
    L = _lib()
    C, S, T, stride = 3, 4, 64, 48
    Lc = (S - 1) * stride + T - 7
    ld = Lc + 9
    audio = torch.randn(C, ld, device=DEV)
    raw, mid = _guarded(C * S * T * 4)
    L.check(L.lib().p2phd_segments_gather_planar(L.ptr(audio), C, ld, Lc, T, stride, S, ctypes.c_void_p(mid.data_ptr()), _stream()))
    torch.cuda.synchronize()
    assert _untouched(raw, C * S * T * 4)
    seg = mid.view(torch.float32).view(C * S, T).clone()
    raw, mid = _guarded(C * ld * 4)
    L.check(L.lib().p2phd_segments_stitch_planar(L.ptr(seg), C, S, T, stride, 1.0, ctypes.c_void_p(mid.data_ptr()), ld, Lc, _stream()))
    torch.cuda.synchronize()
    out = mid.view(torch.int32).view(C, ld)
    assert _untouched(raw, C * ld * 4) and bool((out[:, Lc:] == -0x5A5A5A5B).all())     # 0xA5A5A5A5: the tail of a row is not written


def test_planar_precondition_errors_and_count():
    from pix2pixhdaudiosr_amd.generate import segments_gather_planar, segments_stitch_planar
    L = _lib()
    lib = L.lib()
    seg = torch.zeros(6, 64, device=DEV)
    with pytest.raises(L.P2PHDError, match=r"overlap"):
        segments_stitch_planar(seg, 2, 31)                        # V = 33 > T / 2
    with pytest.raises(L.P2PHDError, match=r"overlap"):
        segments_stitch_planar(seg, 2, 65)
    with pytest.raises(L.P2PHDError, match=r"L_out"):
        segments_stitch_planar(seg, 2, 48, 1.0, 2 * 48 + 64 + 1)
    with pytest.raises(L.P2PHDError, match=r"ld"):
        segments_stitch_planar(seg, 2, 48, 1.0, 100, ld=99)
    with pytest.raises(ValueError):
        segments_stitch_planar(seg, 4, 48)                        # 6 rows are not 4 channels
    with pytest.raises(L.P2PHDError, match=r"stride"):
        segments_gather_planar(torch.zeros(2, 100, device=DEV), 64, 0, 2)
    with pytest.raises(L.P2PHDError, match=r"S >= 1"):
        segments_gather_planar(torch.zeros(2, 100, device=DEV), 64, 64, 0)
    with pytest.raises(L.P2PHDError):
        segments_gather_planar(torch.zeros(2, 100), 64, 64, 2)    # a host tensor: no CPU path
    with pytest.raises(L.P2PHDError):
        segments_gather_planar(torch.zeros(2, 200, device=DEV)[:, ::2], 64, 64, 2)
    a = torch.zeros(2, 100, device=DEV)
    out = torch.zeros(4, 64, device=DEV)
    for C, ld, text in ((0, 100, b"C"), (2, 99, b"ld")):
        assert lib.p2phd_segments_gather_planar(L.ptr(a), C, ld, 100, 64, 64, 2, L.ptr(out), _stream()) != 0
        assert text in lib.p2phd_last_error()
    assert lib.p2phd_segments_stitch_planar(L.ptr(out), 0, 2, 64, 64, 1.0, L.ptr(a), 128, 128, _stream()) != 0
    # launch family "stitch": one launch each, whatever C is
    x = torch.randn(3, 1000, device=DEV)
    lib.p2phd_launch_count(b"stitch", 1)
    s = segments_gather_planar(x, 64, 48, 21)
    segments_stitch_planar(s, 3, 48, 1.0, 1000)
    assert lib.p2phd_launch_count(b"stitch", 1) == 2
