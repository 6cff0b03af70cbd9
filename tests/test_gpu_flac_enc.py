"""The FLAC encoder on the GPU (csrc/flacenc.hip: p2phd_flac_encode; generate.flac_encode) against the host encoder
p2phd_flac_encode_host -- which tests/test_flac_enc_host.py holds to the restatement -- byte for byte, stream and lengths.  Every call
writes its stream between canaries into a buffer filled with a byte pattern (bytes at and beyond the total keep it), takes a
workspace of exactly the planned size poisoned with 0xEE, and lengths between canaries.  Shapes: a sub-matrix of the host matrix,
every decision case (a frame of several windows of the bit stream and a unary run longer than a window among them), the payload at
byte offsets 0 .. 3, frame counts around the scan's step, runs and streams, the launch counter, every refusal, and the round trip
through the device decoder."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import _flac_enc_cases as K
import _flac_enc_ref as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL, POISON, GUARD = 0xA5, 0xEE, 32


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _flacio():
    from pix2pixhdaudiosr_amd.data import flacio
    return flacio


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"flacenc", 1 if reset else 0)


def _call(pay, C, bits, rate, block, offset=0, stream=None, over=None):
    """p2phd_flac_encode -> (rc, the frames' bytes, lengths as a list, everything around them intact)."""
    L_ = _lib()
    total = len(pay) // (C * bits // 8)
    nframes, worst, nwork = _flacio().encode_plan(C, bits, total, block)
    raw = torch.zeros((len(pay) + 8,), dtype=torch.uint8, device=DEV)
    raw[offset:offset + len(pay)] = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
    out = torch.full((GUARD + worst + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((1 + nframes + 1 + 1,), -7, dtype=torch.int64, device=DEV)
    work = torch.full((nwork,), POISON, dtype=torch.uint8, device=DEV)
    a = dict(pay=ctypes.c_void_p(raw.data_ptr() + offset), C=C, bits=bits, L=total, rate=rate, block=block, out=ctypes.c_void_p(out.data_ptr() + GUARD),
             cap=worst, lengths=ctypes.c_void_p(lengths.data_ptr() + 8), work=L_.ptr(work), nwork=nwork)
    a.update(over or {})
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    rc = L_.lib().p2phd_flac_encode(a['pay'], a['C'], a['bits'], a['L'], a['rate'], a['block'], a['out'], a['cap'], a['lengths'], a['work'], a['nwork'],
                                    L_.stream_ptr() if stream is None else ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    got, ln = out.cpu().numpy(), lengths.cpu().numpy()
    intact = bool((got[:GUARD] == FILL).all() and (got[-GUARD:] == FILL).all() and ln[0] == -7 and ln[-1] == -7)
    if rc != 0:
        intact = intact and bool((got == FILL).all() and (ln == -7).all() and (work == POISON).all().item())
        return rc, b"", [], intact
    n = int(ln[-2])
    intact = intact and 0 <= n <= worst and bool((got[GUARD + n:] == FILL).all())
    return rc, got[GUARD:GUARD + n].tobytes(), ln[1:-1].tolist(), intact


def _check(channels, bits, rate, block, **kw):
    C = len(channels)
    pay = E.payload(channels, bits)
    want, lengths = _flacio().encode(pay, C, bits, rate, block)
    rc, got, ln, intact = _call(pay, C, bits, rate, block, **kw)
    assert rc == 0, _lib().lib().p2phd_last_error()
    assert intact
    assert ln == lengths.tolist()
    assert got == want
    return got, lengths


@pytest.mark.parametrize("name", sorted(K.decisions()))
def test_every_decision(name):
    """CONSTANT, VERBATIM, FIXED, the four stereo assignments, the 64-bit sums and the 25-bit side channel, partition orders 0 and 8,
    the three ties, a unary run across several windows; five frames of 4096 x 2 is the largest shape."""
    (channels, bits, rate, block), _ = K.decisions()[name]
    _check(channels, bits, rate, block)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_sub_matrix(C, bits):
    """Blocks 16 (one sample per finest partition), 100 and 1000 (few partitions, lanes sharing one), 576, 4096; a last frame of 1, 5,
    block - 1 and 5 samples; every rate code."""
    i = 0
    for block in (16, 100, 576, 1000, 4096):
        for L in (1, 5, block - 1, block + 1, 3 * block + 5):
            if block == 4096 and L > block + 1 and C == 8:
                L = block + 5                                               # (the largest shape stays five frames of 4096 x 2)
            i += 1
            channels, bits_, rate, block_ = K.matrix_case(C, bits, block, L, i + C)
            _check(channels, bits_, rate, block_)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_payload_at_any_byte_offset(offset):
    _check([K.tone(700, 24, 1), K.tone(700, 24, 2, noise=3)], 24, 48000, 256, offset=offset)
    _check([K.tone(700, 16, 1)], 16, 48000, 256, offset=offset)


def test_frame_counts():
    """1 and 2 frames, and the scan's step (one workgroup walks the frame lengths, p2phd_flac_encode_scan_threads at a time): one
    below, at, one above, and two steps and a frame.  The last frame is short."""
    S = _lib().lib().p2phd_flac_encode_scan_threads()
    assert S >= 64
    for n in (1, 2, S - 1, S, S + 1, 2 * S + 1):
        x = K.tone(16 * n - 3, 16, n % 5, amp=0.05, noise=2)
        got, lengths = _check([x], 16, 44100, 16)
        assert len(lengths) == n + 1


@pytest.mark.parametrize("kind", ["verbatim", "fixed"])
def test_blocks_around_the_writers_step(kind):
    """The frame kernel writes a subframe in steps of p2phd_flac_encode_threads samples (VERBATIM) or residuals (FIXED: the first step
    starts behind the warm-up samples): blocks of one step less one, one step, one more, and the same around two steps, each with a
    shorter last frame; both sample sizes."""
    T = _lib().lib().p2phd_flac_encode_threads()
    assert T >= 64
    for block in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 4):
        for bits in (16, 24):
            L = 2 * block + T // 2
            x = K.full_noise(L, bits, block) if kind == "verbatim" else K.tone(L, bits, block % 5, noise=2)
            _check([x, x[::-1].copy()], bits, 48000, block)


def test_a_step_that_ends_on_the_windows_edge():
    """The frame kernel keeps p2phd_flac_encode_window_words words of the frame's bit stream in LDS and stores them when a step ends
    beyond them.  From frame 128 on a frame of 16-bit noise has a header of 9 bytes (a two-byte frame number, the 16-bit block-size
    trailer), so its VERBATIM subframe starts at bit 80 and ends at 80 + 16 * block: with block = (window - 80) / 16 the first
    channel's last step ends exactly on the window's last bit and the second channel's first step starts exactly behind it.  One
    sample more and one less put the edge inside a sample."""
    W = 32 * _lib().lib().p2phd_flac_encode_window_words()
    assert (W - 80) % 16 == 0 and (W - 80) // 16 > 256 and (W - 80) // 16 not in (576, 1152, 2304, 4608, 512, 1024, 2048, 4096, 8192, 16384, 32768)
    for block in ((W - 80) // 16 - 1, (W - 80) // 16, (W - 80) // 16 + 1):
        L = 130 * block + 7
        got, lengths = _check([K.full_noise(L, 16, 1), K.full_noise(L, 16, 2)], 16, 48000, block)
        assert lengths[129] == 9 + 2 * (1 + 2 * block) + 2             # header, two VERBATIM subframes, CRC-16


def test_runs_and_streams_repeat_the_bytes():
    channels = [K.tone(3000, 24, 1), K.tone(3000, 24, 2, noise=40)]
    side = torch.cuda.Stream()
    a = _check(channels, 24, 96000, 1000)[0]
    b = _check(channels, 24, 96000, 1000)[0]
    c = _check(channels, 24, 96000, 1000, stream=side)[0]
    assert a == b == c


def test_launch_counter_and_refusals():
    channels = [K.tone(100, 16, 1)]
    pay = E.payload(channels, 16)
    _count(reset=True)
    _check(channels, 16, 48000, 64)
    assert _count() == 3                                                    # the frame kernel, the scan, the gather
    null = ctypes.c_void_p(None)
    nframes, worst, nwork = _flacio().encode_plan(1, 16, 100, 64)
    odd = torch.zeros((nwork + 16,), dtype=torch.uint8, device=DEV)
    for over, text in ((dict(C=0), b"channels"), (dict(C=9), b"channels"), (dict(bits=20), b"bits per sample"), (dict(bits=32), b"bits per sample"),
                       (dict(L=0), b"L"), (dict(rate=0), b"rate"), (dict(rate=1048576), b"rate"), (dict(block=15), b"block"), (dict(block=65536), b"block"),
                       (dict(cap=worst - 1), b"worst case"), (dict(nwork=nwork - 1), b"workspace"), (dict(pay=null), b"null"), (dict(out=null), b"null"),
                       (dict(lengths=null), b"null"), (dict(work=null), b"null"), (dict(work=ctypes.c_void_p(odd.data_ptr() + 4)), b"aligned")):
        rc, got, ln, intact = _call(pay, 1, 16, 48000, 64, over=over)
        assert rc != 0 and intact and _count() == 3, over
        assert text in _lib().lib().p2phd_last_error(), (over, _lib().lib().p2phd_last_error())
    assert _count(reset=True) == 3 and _count() == 0


def test_round_trip_on_the_device():
    """The encoder's stream behind flacio's header, through flacio.index_bytes and generate.flac_decode: the input samples."""
    from pix2pixhdaudiosr_amd.generate import flac_decode, flac_encode
    f = _flacio()
    for channels, bits, block in (([K.tone(5000, 16, 1), K.tone(5000, 16, 2, noise=9)], 16, 1024), ([K.tone(900, 24, c, noise=c) for c in range(3)], 24, 192)):
        C, L = len(channels), len(channels[0])
        pay = E.payload(channels, bits)
        dev = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
        stream, lengths = flac_encode(dev, C, bits, 48000, block)
        nframes, worst, _ = f.encode_plan(C, bits, L, block)
        assert stream.numel() == worst and lengths.numel() == nframes + 1
        ln = lengths.cpu().numpy()
        want, hl = f.encode(pay, C, bits, 48000, block)
        assert ln.tolist() == hl.tolist() and stream[:int(ln[-1])].cpu().numpy().tobytes() == want
        data = f.stream_header(ln, 48000, C, bits, L, block, hashlib.md5(pay).digest()) + want
        meta, table = f.index_bytes(data)
        out = flac_decode(torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV), table, meta)
        assert torch.equal(out.cpu(), torch.from_numpy(np.array(channels).astype(np.float32) * np.float32(2.0 ** -(bits - 1))))


def test_op_refusals():
    from pix2pixhdaudiosr_amd.generate import flac_encode
    dev = torch.zeros((240,), dtype=torch.uint8, device=DEV)
    for args, text in (((dev, 9, 16, 48000), "channels"), ((dev, 1, 32, 48000), "float32"), ((dev, 1, 16, 1048576), "rate"), ((dev, 1, 16, 48000, 15), "block"),
                       ((dev, 1, 16, 48000, 65536), "block"), ((dev, 7, 16, 48000), "whole frames"), ((dev[:0], 1, 16, 48000), "whole frames")):
        with pytest.raises(ValueError, match=text):
            flac_encode(*args)
    with pytest.raises(Exception, match="GPU"):
        flac_encode(dev.cpu(), 1, 16, 48000)


def test_stage_entry():
    """The measurement entry: the frame kernel alone (1) or without its CRC-16 (2) counts one launch and leaves the stream and the
    lengths alone; any other stage is refused."""
    L_ = _lib()
    pay = E.payload([K.tone(300, 16, 1)], 16)
    nframes, worst, nwork = _flacio().encode_plan(1, 16, 300, 64)
    raw = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
    out = torch.full((worst,), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((nframes + 1,), -7, dtype=torch.int64, device=DEV)
    work = torch.full((nwork,), POISON, dtype=torch.uint8, device=DEV)
    _count(reset=True)
    for stage, ok in ((1, True), (2, True), (0, False), (3, False)):
        rc = L_.lib().p2phd_flac_encode_stage(stage, L_.ptr(raw), 1, 16, 300, 48000, 64, L_.ptr(out), worst, L_.ptr(lengths), L_.ptr(work), nwork, L_.stream_ptr())
        torch.cuda.synchronize()
        assert (rc == 0) == ok and bool((out == FILL).all()) and bool((lengths == -7).all())
    assert b"stage must be" in L_.lib().p2phd_last_error() and _count(reset=True) == 2
    # the frame lengths the frame kernel left in the workspace are the host encoder's
    assert work[:8 * nframes].cpu().numpy().view(np.int64).tolist() == _flacio().encode(pay, 1, 16, 48000, 64)[1][:-1].tolist()
