"""The device decoders of coded WAV input (csrc/wavcodec.hip) against the library's host entries, bit for bit as uint32 views, in a
0xA5-filled buffer with ld > frames: the rest of every row and the guards around the rows must be untouched.  The host entries
themselves are held against the restatement and audioop in tests/test_wavcodec_host.py, without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _wavcodec_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                                                  # words in front of and behind the rows
FILL = 0xA5A5A5A5


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib()


def _err():
    return _L().p2phd_last_error().decode()


def _count(reset=False):
    return _L().p2phd_launch_count(b"wavcodec", 1 if reset else 0)


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data if a.size else None)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_payload(payload, offset):
    """The payload on the device at byte `offset` behind a 256-byte aligned address, 0xEE around it -> (keep-alive, address)."""
    n = len(payload)
    host = np.full(offset + n + 64, 0xEE, dtype=np.uint8)
    host[offset:offset + n] = np.frombuffer(bytes(payload), dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 256 == 0
    return dev, dev.data_ptr() + offset


def _guarded(C, ld, skew):
    """A 0xA5-filled buffer; the rows start `skew` words behind a 16-byte boundary -> (tensor of int32 words, address of row 0)."""
    words = GUARD + skew + C * ld + GUARD
    buf = torch.full((words,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * (GUARD + skew)


def _expected(C, ld, skew, frames, rows):
    want = np.full(GUARD + skew + C * ld + GUARD, FILL, dtype=np.uint32)
    body = want[GUARD + skew:GUARD + skew + C * ld].reshape(C, ld)
    body[:, :frames] = np.ascontiguousarray(rows[:, :frames], dtype=np.float32).view(np.uint32)
    return want


def _host_ima(payload, C, align, frames):
    src = np.frombuffer(bytes(payload), dtype=np.uint8)
    out = np.zeros((C, max(frames, 1)), dtype=np.float32)
    assert _L().p2phd_ima_decode_host(_vp(src), src.size, C, align, 0, frames, _vp(out), max(frames, 1)) == 0, _err()
    return out


def _host_g711(payload, C, law, frames):
    src = np.frombuffer(bytes(payload), dtype=np.uint8)
    out = np.zeros((C, max(frames, 1)), dtype=np.float32)
    assert _L().p2phd_g711_decode_host(_vp(src), frames, C, law, _vp(out), max(frames, 1)) == 0, _err()
    return out


def _run_ima(payload, C, align, frames, offset=0, skew=0, pad=5):
    ld = frames + pad
    keep, src = _device_payload(payload, offset)
    buf, dst = _guarded(C, ld, skew)
    rc = _L().p2phd_ima_decode(ctypes.c_void_p(src), len(payload), C, align, frames, ctypes.c_void_p(dst), ld, _stream())
    assert rc == 0, _err()
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32), ld


def _check_ima(payload, C, align, frames, offset=0, skew=0):
    got, ld = _run_ima(payload, C, align, frames, offset, skew)
    want = _expected(C, ld, skew, frames, _host_ima(payload, C, align, frames))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8] - GUARD - skew, got[bad[:8]], want[bad[:8]])


def _random_ima(rng, C, align, blocks, extra=0, any_index=False):
    payload = bytearray(rng.integers(0, 256, blocks * align + extra, dtype=np.uint8).tobytes())
    if not any_index:
        heads = np.arange(blocks)[:, None] * align + 4 * np.arange(C)[None, :] + 2
        idx = rng.integers(0, 89, heads.shape, dtype=np.uint8)
        arr = np.frombuffer(payload, dtype=np.uint8)
        arr[heads.reshape(-1)] = idx.reshape(-1)
    return bytes(payload)


ALIGN_OF_SPB = {9: 8, 505: 256, 2041: 1024}                               # block_align per channel


# ---- G.711 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", [R.ULAW, R.ALAW])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_g711_device_equals_host(law, channels):
    rng = np.random.default_rng(100 * law + channels)
    C = channels
    counts = sorted({max(0, k * C + d) for k in (16, 64, 256) for d in (-1, 0, 1)} | {k + d for k in (16, 64, 256) for d in (-1, 0, 1)} | {1, 5000})
    for i, frames in enumerate(counts):
        # all 256 codes in every channel where they fit, then random bytes
        payload = np.concatenate([np.repeat(np.arange(256, dtype=np.uint8), C), rng.integers(0, 256, frames * C, dtype=np.uint8)])
        payload = (payload if frames >= 256 else payload[256 * C:])[:frames * C]
        for offset in ([i % 16] if frames != 64 * C else range(16)):
            ld, skew = frames + 7, i % 4
            keep, src = _device_payload(payload.tobytes(), offset)
            buf, dst = _guarded(C, ld, skew)
            assert _L().p2phd_g711_decode(ctypes.c_void_p(src), frames, C, law, ctypes.c_void_p(dst), ld, _stream()) == 0, _err()
            torch.cuda.synchronize()
            want = _expected(C, ld, skew, frames, _host_g711(payload.tobytes(), C, law, frames))
            assert np.array_equal(buf.cpu().numpy().view(np.uint32), want), (frames, offset)


@pytest.mark.parametrize("law", [R.ULAW, R.ALAW])
def test_g711_all_codes_are_the_restatement(law):
    from pix2pixhdaudiosr_amd import generate as G
    codes = torch.arange(256, dtype=torch.uint8, device="cuda")
    out = G.g711_decode(codes, 256, 1, 'alaw' if law == R.ALAW else 'ulaw')
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[0], R.scale(R.g711_table(law)).view(np.uint32))
    two = G.g711_decode(codes, 128, 2, 'alaw' if law == R.ALAW else 'ulaw').cpu().numpy()
    assert np.array_equal(two.T.reshape(-1).view(np.uint32), R.scale(R.g711_table(law)).view(np.uint32))


def test_g711_past_the_grid_cap():
    """More 16-byte pieces than the capped grid of 256-lane workgroups takes in one trip: the stride loop's second trip."""
    frames = _L().p2phd_g711_max_workgroups() * 256 * 16 + 16 * 300 + 5
    rng = np.random.default_rng(3)
    payload = rng.integers(0, 256, frames, dtype=np.uint8)
    dev = torch.from_numpy(payload).cuda()
    from pix2pixhdaudiosr_amd import generate as G
    out = G.g711_decode(dev, frames, 1, 'ulaw')
    want = torch.from_numpy(R.scale(R.ULAW_TABLE)).cuda()[dev.long()]
    assert torch.equal(out[0].view(torch.int32), want.view(torch.int32))


# ---- IMA ADPCM -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spb", [9, 505, 2041])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("blocks", [1, 63, 64, 65, 257])
def test_ima_device_equals_host(blocks, channels, spb):
    align = ALIGN_OF_SPB[spb] * channels
    rng = np.random.default_rng(blocks * 1000 + channels * 10 + spb)
    payload = _random_ima(rng, channels, align, blocks)
    k = blocks + channels + spb
    _check_ima(payload, channels, align, blocks * spb, offset=k % 4, skew=(k // 4) % 4)


@pytest.mark.parametrize("channels", [1, 3])
def test_ima_past_the_grid_cap(channels):
    L = _L()
    align = 8 * channels
    bpw, cap = L.p2phd_ima_blocks_per_workgroup(channels, align), L.p2phd_ima_max_workgroups()
    assert bpw >= 1 and cap >= 1
    blocks = bpw * cap + 1                                                  # the last block is the second trip of workgroup 0
    payload = _random_ima(np.random.default_rng(channels), channels, align, blocks)
    _check_ima(payload, channels, align, blocks * 9, offset=0, skew=1)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("skew", [0, 1, 2, 3])
def test_ima_payload_offsets_and_row_alignment(offset, skew):
    """Payload at every byte offset of a word; rows 0, 4, 8 and 12 bytes off a 16-byte boundary (with ld odd the rows differ too)."""
    C, align = 2, 512
    payload = _random_ima(np.random.default_rng(offset * 4 + skew), C, align, 65)
    _check_ima(payload, C, align, 65 * 505, offset, skew)


@pytest.mark.parametrize("channels,spb", [(1, 9), (2, 505), (3, 9), (8, 505)])
def test_ima_partial_last_block_and_fact_cut(channels, spb):
    C, align = channels, ALIGN_OF_SPB[spb] * channels
    rng = np.random.default_rng(7 * C + spb)
    groups = (spb - 1) // 8
    for k in sorted({0, 1, groups - 1}):                                    # a trailing partial block: the headers and k whole groups
        extra = 4 * C * (1 + k)
        for slack in (0, 3):                                                # ... and bytes behind it that make no group
            payload = _random_ima(rng, C, align, 66, extra=0)
            payload = payload[:65 * align + extra + slack]
            frames = _L().p2phd_ima_frames(len(payload), C, align)
            assert frames == 65 * spb + 1 + 8 * k == R.ima_frames(len(payload), C, align)
            _check_ima(payload, C, align, frames, offset=k % 4, skew=slack)
    payload = _random_ima(rng, C, align, 66)
    for frames in [1, 2, 8, 9, 10, spb - 1, spb, spb + 1, spb + 2, 65 * spb + 5, 66 * spb - 1, 66 * spb]:          # `fact` cuts inside a block
        _check_ima(payload, C, align, frames, offset=frames % 4, skew=frames % 3)


@pytest.mark.parametrize("channels", [1, 2, 8])
def test_ima_any_header_index_is_clamped_on_both_sides(channels):
    """Random bytes, header indices 0 .. 255 included: the device clamps on load, and so does the host entry without the scan."""
    align = 36 * channels
    payload = _random_ima(np.random.default_rng(40 + channels), channels, align, 300, any_index=True)
    heads = np.frombuffer(payload, dtype=np.uint8).reshape(300, align)[:, 2:4 * channels:4]
    assert (heads > 88).sum() > 100 and _L().p2phd_ima_scan_host(_vp(np.frombuffer(payload, dtype=np.uint8)), len(payload), channels, align) >= 0
    _check_ima(payload, channels, align, 300 * 65, offset=1, skew=2)


def test_ima_small_case_is_the_restatement():
    from pix2pixhdaudiosr_amd import generate as G
    x = R.speech_like(2, 400, 1)
    payload = R.ima_encode(x, 72)
    ref = R.ima_decode(payload, 2, 72)
    out = G.ima_decode(torch.from_numpy(np.frombuffer(payload, dtype=np.uint8).copy()).cuda(), ref.shape[1], 2, 72)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.scale(ref).view(np.uint32))
    sat = b"".join(np.int16(p).tobytes() + bytes([88, 0]) + bytes([n | (n << 4)]) * 32 for p, n in [(32000, 7), (-32000, 15), (0, 0), (0, 8)])
    ref = R.ima_decode(sat, 1, 36)
    assert ref.max() == 32767 and ref.min() == -32768
    out = G.ima_decode(torch.from_numpy(np.frombuffer(sat, dtype=np.uint8).copy()).cuda(), ref.shape[1], 1, 36)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), R.scale(ref).view(np.uint32))


def test_two_runs_and_two_streams_give_the_same_bits():
    C, align = 3, 36 * 3
    payload = _random_ima(np.random.default_rng(5), C, align, 700)
    a, _ = _run_ima(payload, C, align, 700 * 65)
    b, _ = _run_ima(payload, C, align, 700 * 65)
    with torch.cuda.stream(torch.cuda.Stream()):
        c, _ = _run_ima(payload, C, align, 700 * 65)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    from pix2pixhdaudiosr_amd import generate as G
    g = torch.from_numpy(np.random.default_rng(6).integers(0, 256, 3 * 5001, dtype=np.uint8)).cuda()
    x = G.g711_decode(g, 5001, 3, 'alaw')
    with torch.cuda.stream(torch.cuda.Stream()):
        y = G.g711_decode(g, 5001, 3, 'alaw')
        torch.cuda.current_stream().synchronize()
    assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), G.g711_decode(g, 5001, 3, 'alaw').view(torch.int32))


def test_launch_counter():
    from pix2pixhdaudiosr_amd import generate as G
    ima = torch.from_numpy(np.frombuffer(_random_ima(np.random.default_rng(1), 2, 72, 4), dtype=np.uint8).copy()).cuda()
    g = torch.arange(64, dtype=torch.uint8, device="cuda")
    _count(reset=True)
    G.ima_decode(ima, 4 * 65, 2, 72)
    assert _count() == 1
    G.g711_decode(g, 32, 2, 'ulaw')
    assert _count() == 2
    assert G.ima_decode(ima, 0, 2, 72).shape == (2, 0) and G.g711_decode(g, 0, 2, 'alaw').shape == (2, 0)
    assert _count(reset=True) == 2                                          # frames = 0 launches nothing
    pcm = torch.zeros(64, dtype=torch.uint8, device="cuda")
    G.pcm_decode(pcm, 16, 2, 1, 16)
    assert _count() == 0


def test_c_entry_refusals():
    L = _L()
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.zeros(4096, dtype=torch.float32, device="cuda")
    s, o, st = ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(out.data_ptr()), _stream()
    _count(reset=True)

    def g711(*a):
        assert L.p2phd_g711_decode(*a) != 0
        return _err()

    def ima(*a):
        assert L.p2phd_ima_decode(*a) != 0
        return _err()

    assert "law must be" in g711(s, 16, 1, 2, o, 16, st)
    assert "1 <= channels <= 65535" in g711(s, 16, 0, 0, o, 16, st)
    assert "frames >= 0" in g711(s, -1, 1, 0, o, 16, st)
    assert "ld 15 is shorter" in g711(s, 16, 1, 0, o, 15, st)
    assert "null pointer" in g711(None, 16, 1, 0, o, 16, st) and "null pointer" in g711(s, 16, 1, 0, None, 16, st)
    assert "not aligned to a float" in g711(s, 16, 1, 0, ctypes.c_void_p(out.data_ptr() + 2), 16, st)
    for C, align in [(0, 8), (9, 72), (1, 4), (1, 10), (2, 36), (1, 65536)]:
        assert "block_align a multiple of" in ima(s, 4096, C, align, 1, o, 16, st)
    assert "does not fit a workgroup's LDS" in ima(s, 4096, 1, 65028, 1, o, 16, st)
    assert "frames asked of a payload that holds 4608" in ima(s, 4096, 1, 8, 4609, torch.zeros(4609, device="cuda").data_ptr(), 4609, st)
    assert "frames asked" in ima(s, 4096, 1, 8, -1, o, 4096, st)
    assert "ld 8 is shorter" in ima(s, 4096, 1, 8, 9, o, 8, st)
    assert "null pointer" in ima(None, 4096, 1, 8, 9, o, 9, st) and "null pointer" in ima(s, 4096, 1, 8, 9, None, 9, st)
    assert "not aligned to a float" in ima(s, 4096, 1, 8, 9, ctypes.c_void_p(out.data_ptr() + 1), 9, st)
    assert "nbytes" in ima(s, -1, 1, 8, 0, o, 9, st)
    assert _count() == 0
    from pix2pixhdaudiosr_amd import generate as G
    with pytest.raises(ValueError, match="law must be"):
        G.g711_decode(src, 4, 1, 'mulaw')
    with pytest.raises(ValueError, match="do not hold"):
        G.g711_decode(src, 4097, 1, 'ulaw')
    with pytest.raises(Exception, match="frames asked"):
        G.ima_decode(src, 4609, 1, 8)
