"""p2phd_pcm_decode_ex (csrc/pcm.hip) on the GPU: the device decoder of the big-endian containers against numpy, bit for bit as
uint32 -- every format in both byte orders and with signed 8-bit samples, at every byte offset 0 .. 7 of the payload (the typed loads
with their byte swap and the byte-wise ones), between guard rows; float and integer edge values; flags = 0 against p2phd_pcm_decode;
a payload past the cap of the grid; streams, repeats, the launch counter and every refusal."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U8, S16, S24, S32, F32, F64 = range(6)                                      # P2PHD_PCM_* of include/p2phd.h
BIG, SIGNED8 = 1, 2
WIDTH = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
CASES = [("u8", U8, 0), ("u8_be", U8, BIG), ("s8", U8, SIGNED8), ("s8_be", U8, SIGNED8 | BIG), ("s16_le", S16, 0), ("s16_be", S16, BIG),
         ("s24_le", S24, 0), ("s24_be", S24, BIG), ("s32_le", S32, 0), ("s32_be", S32, BIG), ("f32_le", F32, 0), ("f32_be", F32, BIG),
         ("f64_le", F64, 0), ("f64_be", F64, BIG)]


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"pcm", 1 if reset else 0)


def reference(payload, channels, fmt, flags):
    """numpy: the interleaved payload -> uint32 [channels, frames], the bits of the WAV twin's float32 samples."""
    raw = np.frombuffer(bytes(payload), dtype=np.uint8)
    order = ">" if flags & BIG else "<"
    if fmt == U8:
        a = raw.view(np.int8).astype(np.float32) if flags & SIGNED8 else raw.astype(np.float32) - np.float32(128.0)
        a = a * np.float32(1.0 / 128.0)
    elif fmt == S16:
        a = raw.view(order + "i2").astype(np.float32) * np.float32(2.0 ** -15)
    elif fmt == S24:
        b = raw.reshape(-1, 3).astype(np.int32)
        hi, lo = (0, 2) if flags & BIG else (2, 0)
        a = (((b[:, lo] | (b[:, 1] << 8) | (b[:, hi] << 16)) << 8) >> 8).astype(np.float32) * np.float32(2.0 ** -23)
    elif fmt == S32:
        a = raw.view(order + "i4").astype(np.float32) * np.float32(2.0 ** -31)
    elif fmt == F32:
        a = raw.view(order + "u4").astype(np.uint32).view(np.float32)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            a = raw.view(order + "f8").astype(np.float32)
    return np.ascontiguousarray(a.view(np.uint32).reshape(-1, channels).T)


def make_payload(rng, fmt, flags, samples):
    """Random bytes -- every bit pattern of an integer or float32 sample is a case; float64: finite values of every size (a NaN's
    payload is looked at by test_float64_edges)."""
    if fmt != F64:
        return rng.integers(0, 256, size=samples * WIDTH[fmt], dtype=np.uint8).tobytes()
    x = rng.standard_normal(samples) * 10.0 ** rng.integers(-50, 42, size=samples)
    return x.astype(">f8" if flags & BIG else "<f8").tobytes()


def decode(payload, frames, channels, fmt, flags, offset=0, ld=None, entry="ex"):
    """-> (uint32 [channels + 2, ld] with the guard rows, host copy).  The payload stands `offset` bytes into a 512-byte aligned
    allocation; the output is rows 1 .. channels of a buffer filled with 0xA5."""
    L = _lib()
    ld = frames + 5 if ld is None else ld
    big = torch.full((len(payload) + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    if payload:
        big[offset:offset + len(payload)] = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(DEV)
    out = torch.full(((channels + 2) * ld * 4,), 0xA5, dtype=torch.uint8, device=DEV)
    src, dst = ctypes.c_void_p(big.data_ptr() + offset), ctypes.c_void_p(out.data_ptr() + 4 * ld)
    if entry == "ex":
        L.check(L.lib().p2phd_pcm_decode_ex(src, frames, channels, fmt, flags, dst, ld, L.stream_ptr()), "pcm_decode_ex")
    else:
        L.check(L.lib().p2phd_pcm_decode(src, frames, channels, fmt, dst, ld, L.stream_ptr()), "pcm_decode")
    return out, big


def rows(out, channels, ld):
    return out.cpu().numpy().view(np.uint32).reshape(channels + 2, ld)


def check_guarded(host, want, frames, what):
    assert np.array_equal(host[1:-1, :frames], want), what
    assert (host[0] == 0xA5A5A5A5).all() and (host[-1] == 0xA5A5A5A5).all() and (host[1:-1, frames:] == 0xA5A5A5A5).all(), what


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fmt,flags", CASES, ids=[c[0] for c in CASES])
def test_matrix_against_numpy(name, fmt, flags):
    rng = np.random.default_rng(100 + fmt * 4 + flags)
    for channels in (1, 2, 3, 8):
        for frames in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000):
            payload = make_payload(rng, fmt, flags, frames * channels)
            want = reference(payload, channels, fmt, flags)
            outs = [decode(payload, frames, channels, fmt, flags, offset) for offset in range(8)]
            torch.cuda.synchronize()
            for offset, (out, _) in enumerate(outs):
                check_guarded(rows(out, channels, frames + 5), want, frames, (name, channels, frames, offset))


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
def test_float32_edges_are_bit_copies():
    words = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFBFFFFF, 0x7FA55AA5, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                      0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x12345678],
                     dtype=np.uint32)
    for order, flags in ((">u4", BIG), ("<u4", 0)):
        for offset in (0, 1, 2, 4):
            out, _ = decode(words.astype(order).tobytes(), 10, 2, F32, flags, offset)
            check_guarded(rows(out, 2, 15), np.ascontiguousarray(words.reshape(10, 2).T), 10, (order, offset))


def test_float64_edges():
    f32 = lambda bits_: np.array([bits_], dtype=np.uint32).view(np.float32)[0].astype(np.float64)
    one, eps, big, tiny = 1.0, 2.0 ** -24, float(f32(0x7F7FFFFF)), 2.0 ** -149
    values = np.array([
        one + eps, one + 3 * eps, one + eps * (1 + 2.0 ** -20), one + eps * (1 - 2.0 ** -20), -(one + eps), -(one + 3 * eps),     # ties, and beside them
        big, big + 2.0 ** 102, big + 2.0 ** 103, big + 2.0 ** 103 * (1 - 2.0 ** -30), -(big + 2.0 ** 103), 1e300, -1e300,          # up to and over the top
        tiny, tiny / 2, tiny / 2 * (1 + 2.0 ** -30), 1.5 * tiny, 2.5 * tiny, 3 * tiny, 2.0 ** -126, 2.0 ** -126 - tiny / 2, 2.0 ** -127, 1e-40, -1e-40,
        1e-46, -1e-46, 5e-324, 0.0, -0.0, float("inf"), -float("inf"), 0.1, -1.0 / 3.0], dtype=np.float64)                         # subnormal results
    values = np.concatenate([values, [float("nan")]])
    nan_at = len(values) - 1
    for order, flags in ((">f8", BIG), ("<f8", 0)):
        payload = values.astype(order).tobytes()
        want = reference(payload, 1, F64, flags)
        assert want[0, 0] == 0x3F800000 and want[0, 1] == 0x3F800002 and want[0, 8] == 0x7F800000 and want[0, 14] == 0 and want[0, 16] == 2
        for offset in (0, 3, 4):
            got = rows(decode(payload, len(values), 1, F64, flags, offset)[0], 1, len(values) + 5)
            assert np.array_equal(got[1, :nan_at], want[0, :nan_at]), (order, offset)
            assert got[1, nan_at] & 0x7FFFFFFF > 0x7F800000                       # a NaN stays one
    # NaNs with payloads: quiet, signalling, negative -- what P2PHD_PCM_F64 gives for the byte-swapped twin
    nans = np.array([0x7FF8000000000000, 0x7FF8123456789ABC, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFF4000000000000], dtype=np.uint64)
    be = rows(decode(nans.astype(">u8").tobytes(), 5, 1, F64, BIG)[0], 1, 10)
    le = rows(decode(nans.astype("<u8").tobytes(), 5, 1, F64, 0, entry="old")[0], 1, 10)
    assert np.array_equal(be, le) and ((be[1, :5] & 0x7FFFFFFF) > 0x7F800000).all()


def test_int32_edges_round_like_numpy():
    near = [2 ** 31 - 1, 2 ** 31 - 64, 2 ** 31 - 65, 2 ** 31 - 127, 2 ** 31 - 128, 2 ** 31 - 129, 2 ** 31 - 192, -2 ** 31, -2 ** 31 + 1, -2 ** 31 + 64,
            -2 ** 31 + 65, -2 ** 31 + 128, -2 ** 31 + 129, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 25 + 1, 2 ** 25 + 3, -(2 ** 24) - 1,
            -(2 ** 24) - 3, 2 ** 30 + 32, 2 ** 30 + 96, 2 ** 30 + 33, 0, 1, -1, 2 ** 24, 2 ** 24 - 1, 123456789]
    x = np.array(near, dtype=np.int64).astype(np.int32)
    want = (x.astype(np.float32) * np.float32(2.0 ** -31)).view(np.uint32)
    assert want[0] == 0x3F800000 and want[7] == 0xBF800000                         # (2^31 - 1 rounds to 1.0)
    for order, flags in ((">i4", BIG), ("<i4", 0)):
        for offset in (0, 1):
            got = rows(decode(x.astype(order).tobytes(), len(x) // 2, 2, S32, flags, offset)[0], 2, len(x) // 2 + 5)
            assert np.array_equal(got[1:-1, :len(x) // 2], np.ascontiguousarray(want.reshape(-1, 2).T)), (order, offset)


def test_signed8_is_the_twin_of_unsigned():
    """Every byte: the signed sample s decodes to what its twin's byte s + 128 decodes to, and to s / 128."""
    s = np.arange(-128, 128, dtype=np.int64)
    signed = rows(decode(s.astype(np.int8).tobytes(), 128, 2, U8, SIGNED8)[0], 2, 133)
    twin = rows(decode((s + 128).astype(np.uint8).tobytes(), 128, 2, U8, 0, entry="old")[0], 2, 133)
    assert np.array_equal(signed, twin)
    assert np.array_equal(signed[1:-1, :128].T.reshape(-1).view(np.float32), (s / 128.0).astype(np.float32))


# ---- flags = 0, the cap, streams, the counter ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [U8, S16, S24, S32, F32, F64])
def test_flags_zero_is_pcm_decode(fmt):
    rng = np.random.default_rng(40 + fmt)
    for channels, frames in ((1, 257), (3, 1000)):
        payload = rng.integers(0, 256, size=frames * channels * WIDTH[fmt], dtype=np.uint8).tobytes()       # (float64: NaNs among them)
        for offset in (0, 1, 4):
            new = rows(decode(payload, frames, channels, fmt, 0, offset)[0], channels, frames + 5)
            old = rows(decode(payload, frames, channels, fmt, 0, offset, entry="old")[0], channels, frames + 5)
            assert np.array_equal(new, old), (fmt, channels, frames, offset)


def test_past_the_cap_every_element():
    """S16 big-endian, 2 channels, unit_work + 258 samples (unit_work is even, so unit_work + 257 is no whole number of two-channel
    frames: the least count above it that is): the grid is capped, its threads take a second trip, and every element is compared."""
    import _long as K
    L = _lib()
    rc, unit, wanted, used = K.stream_grid(L.lib(), "pcm_decode_ex", 0, 1 << 30)
    assert rc == 0 and used < wanted and unit == used * 256
    frames = (unit + 257 + 1) // 2
    rc, unit2, wanted, used = K.stream_grid(L.lib(), "pcm_decode_ex", 0, frames * 2)
    assert rc == 0 and used < wanted and unit2 == unit and unit < frames * 2 < 2 * unit
    x = np.random.default_rng(8).integers(-32768, 32768, size=frames * 2, dtype=np.int64).astype(">i2")
    _count(reset=True)
    out, _ = decode(x.tobytes(), frames, 2, S16, BIG, offset=0, ld=frames)
    assert _count(reset=True) == 1
    got = rows(out, 2, frames)
    want = np.ascontiguousarray((x.astype(np.float32) * np.float32(2.0 ** -15)).view(np.uint32).reshape(-1, 2).T)
    assert np.array_equal(got[1:-1], want) and (got[0] == 0xA5A5A5A5).all() and (got[-1] == 0xA5A5A5A5).all()


def test_streams_and_repeats():
    rng = np.random.default_rng(12)
    payload = rng.integers(0, 256, size=5000 * 3 * 3, dtype=np.uint8).tobytes()
    want = reference(payload, 3, S24, BIG)
    first = rows(decode(payload, 5000, 3, S24, BIG, 1)[0], 3, 5005)
    second = rows(decode(payload, 5000, 3, S24, BIG, 1)[0], 3, 5005)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out, keep = decode(payload, 5000, 3, S24, BIG, 1)
    side.synchronize()
    third = rows(out, 3, 5005)
    assert np.array_equal(first, second) and np.array_equal(first, third)
    check_guarded(first, want, 5000, "s24 be")


def test_wrapper_and_counter():
    from pix2pixhdaudiosr_amd.generate import pcm_decode
    rng = np.random.default_rng(13)
    payload = rng.integers(0, 256, size=100 * 2 * 3, dtype=np.uint8).tobytes()
    dev = torch.frombuffer(bytearray(b"\0" + payload), dtype=torch.uint8).to(DEV)[1:]      # storage offset of one byte
    _count(reset=True)
    got = pcm_decode(dev, 100, 2, 1, 24, big_endian=True)
    assert _count(reset=True) == 1
    assert np.array_equal(got.cpu().numpy().view(np.uint32), reference(payload, 2, S24, BIG))
    assert np.array_equal(pcm_decode(dev, 100, 2, 1, 24).cpu().numpy().view(np.uint32), reference(payload, 2, S24, 0))
    assert np.array_equal(pcm_decode(dev, 300, 2, 1, 8, signed8=True).cpu().numpy().view(np.uint32), reference(payload, 2, U8, SIGNED8))
    assert np.array_equal(pcm_decode(dev, 300, 2, 1, 8, big_endian=True, signed8=True).cpu().numpy().view(np.uint32), reference(payload, 2, U8, SIGNED8))
    assert np.array_equal(pcm_decode(dev, 300, 2, 1, 8, big_endian=True).cpu().numpy().view(np.uint32), reference(payload, 2, U8, 0))
    assert np.array_equal(pcm_decode(dev, 75, 2, 3, 32, big_endian=True).cpu().numpy().view(np.uint32), reference(payload, 2, F32, BIG))
    assert _count(reset=True) == 5
    empty = pcm_decode(dev, 0, 2, 1, 16, big_endian=True)                            # frames = 0: nothing launched, nothing counted
    assert tuple(empty.shape) == (2, 0) and _count() == 0
    decode(b"", 0, 3, S32, BIG)
    assert _count() == 0
    with pytest.raises(_lib().P2PHDError, match="SIGNED8"):
        pcm_decode(dev, 100, 2, 1, 24, signed8=True)
    with pytest.raises(ValueError, match="do not hold"):
        pcm_decode(dev, 101, 2, 1, 24, big_endian=True)
    assert _count() == 0


def test_refusals():
    L = _lib()
    src = torch.zeros(256, dtype=torch.uint8, device=DEV)
    out = torch.full((64,), 0xA5, dtype=torch.uint8, device=DEV)
    S, O = src.data_ptr(), out.data_ptr()
    _count(reset=True)
    #        frames, channels, format, flags, ld, bytes, out -> a word of the error text
    cases = [((4, 1, S16, SIGNED8, 4, S, O), b"SIGNED8"), ((4, 1, S24, SIGNED8 | BIG, 4, S, O), b"SIGNED8"), ((4, 1, S32, SIGNED8, 4, S, O), b"SIGNED8"),
             ((4, 1, F32, SIGNED8, 4, S, O), b"SIGNED8"), ((4, 1, F64, SIGNED8, 4, S, O), b"SIGNED8"), ((4, 1, S16, 4, 4, S, O), b"flag"),
             ((4, 1, U8, 8 | SIGNED8, 4, S, O), b"flag"), ((4, 1, S16, -1, 4, S, O), b"flag"), ((4, 1, S16, 1 << 30, 4, S, O), b"flag"),
             ((4, 0, S16, BIG, 4, S, O), b"channels"), ((4, 65536, S16, BIG, 4, S, O), b"channels"), ((-1, 1, S16, BIG, 4, S, O), b"frames"),
             ((4, 1, 6, BIG, 4, S, O), b"format"), ((4, 1, -1, BIG, 4, S, O), b"format"), ((4, 1, S16, BIG, 3, S, O), b"ld"),
             (((1 << 40) // 2 + 1, 2, S16, BIG, 1 << 40, S, O), b"too large"), ((4, 1, S16, BIG, 4, 0, O), b"null"), ((4, 1, S16, BIG, 4, S, 0), b"null"),
             ((4, 1, S16, BIG, 4, S, O + 2), b"aligned"), ((4, 1, U8, SIGNED8, 4, S, O + 1), b"aligned")]
    for (frames, ch, fmt, flags, ld, b, o), word in cases:
        rc = L.lib().p2phd_pcm_decode_ex(ctypes.c_void_p(b), frames, ch, fmt, flags, ctypes.c_void_p(o), ld, L.stream_ptr())
        text = L.lib().p2phd_last_error()
        assert rc != 0 and text.startswith(b"pcm_decode_ex") and word in text, (frames, ch, fmt, flags, ld, text)
    torch.cuda.synchronize()
    assert _count() == 0 and bool((out == 0xA5).all())
    # frames = 0 is checked like any call and passes without pointers
    assert L.lib().p2phd_pcm_decode_ex(None, 0, 2, S16, BIG, None, 0, L.stream_ptr()) == 0 and _count() == 0
    assert L.lib().p2phd_pcm_decode_ex(None, 0, 2, S16, SIGNED8, None, 0, L.stream_ptr()) != 0
