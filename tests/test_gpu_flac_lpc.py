"""The LPC option of the FLAC encoder on the GPU (csrc/flacenc.hip: p2phd_flac_encode_lpc, the frame kernel's LPC instantiation;
generate.flac_encode(lpc_order=M)) against the host encoder p2phd_flac_encode_lpc_host -- which tests/test_flac_lpc_host.py holds to the
restatement -- byte for byte, stream and lengths.  The set-up is tests/test_gpu_flac_enc.py's: every call runs between canaries, in a
poisoned workspace of exactly the planned size, and the payload sits at byte offsets 0 .. 3."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import _flac_enc_cases as K
import _flac_enc_ref as E
import _flac_lpc_cases as C

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


def _call(pay, Cn, bits, rate, block, M, offset=0, stream=None, over=None, entry="lpc"):
    """p2phd_flac_encode_lpc (entry 'plain': p2phd_flac_encode) -> (rc, the frames' bytes, lengths as a list, everything around them intact)."""
    L_ = _lib()
    total = len(pay) // (Cn * bits // 8)
    nframes, worst, nwork = _flacio().encode_plan(Cn, bits, total, min(block, 65535))
    raw = torch.zeros((len(pay) + 8,), dtype=torch.uint8, device=DEV)
    raw[offset:offset + len(pay)] = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
    out = torch.full((GUARD + worst + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((1 + nframes + 1 + 1,), -7, dtype=torch.int64, device=DEV)
    work = torch.full((nwork,), POISON, dtype=torch.uint8, device=DEV)
    a = dict(pay=ctypes.c_void_p(raw.data_ptr() + offset), C=Cn, bits=bits, L=total, rate=rate, block=block, M=M, out=ctypes.c_void_p(out.data_ptr() + GUARD),
             cap=worst, lengths=ctypes.c_void_p(lengths.data_ptr() + 8), work=L_.ptr(work), nwork=nwork)
    a.update(over or {})
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    st = L_.stream_ptr() if stream is None else ctypes.c_void_p(stream.cuda_stream)
    if entry == "plain":
        rc = L_.lib().p2phd_flac_encode(a['pay'], a['C'], a['bits'], a['L'], a['rate'], a['block'], a['out'], a['cap'], a['lengths'], a['work'], a['nwork'], st)
    else:
        rc = L_.lib().p2phd_flac_encode_lpc(a['pay'], a['C'], a['bits'], a['L'], a['rate'], a['block'], a['M'], a['out'], a['cap'], a['lengths'], a['work'],
                                            a['nwork'], st)
    torch.cuda.synchronize()
    got, ln = out.cpu().numpy(), lengths.cpu().numpy()
    intact = bool((got[:GUARD] == FILL).all() and (got[-GUARD:] == FILL).all() and ln[0] == -7 and ln[-1] == -7)
    if rc != 0:
        intact = intact and bool((got == FILL).all() and (ln == -7).all() and (work == POISON).all().item())
        return rc, b"", [], intact
    n = int(ln[-2])
    intact = intact and 0 <= n <= worst and bool((got[GUARD + n:] == FILL).all())
    return rc, got[GUARD:GUARD + n].tobytes(), ln[1:-1].tolist(), intact


def _check(channels, bits, rate, block, M, **kw):
    Cn = len(channels)
    pay = E.payload(channels, bits)
    want, lengths = _flacio().encode(pay, Cn, bits, rate, block, lpc_order=M)
    rc, got, ln, intact = _call(pay, Cn, bits, rate, block, M, **kw)
    assert rc == 0, _lib().lib().p2phd_last_error()
    assert intact
    assert ln == lengths.tolist()
    assert got == want
    return got, lengths


@pytest.mark.parametrize("name", sorted(C.decisions()))
def test_every_decision(name):
    """The decision fixtures of the host tests: LPC chosen, a last frame shorter than the order, the silent analysis signal, an order
    without a coefficient, the 25-bit side channel, orders the residual bound rejects (its LDS maximum and the pass that is
    skipped), the clamped shift, the three ties, stereo, 24 bit."""
    (channels, bits, rate, block, M), _ = C.decisions()[name]
    _check(channels, bits, rate, block, M)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("Cn", [1, 2, 3, 8])
def test_sub_matrix(Cn, bits):
    """Blocks 16, 17, 255, 256, 257 and 512 (from one sample per finest partition to lanes sharing the only one), lengths around the
    block, M = 1 and 12."""
    for i, block in enumerate((16, 17, 255, 256, 257, 512)):
        for j, L in enumerate((1, 5, block - 1, block + 1, 2 * block + 13)):
            _check(C.signal(Cn, bits, L, i + j + Cn), bits, K.RATES[(i + j) % 5], block, 12 if (i + j) % 2 else 1)
            if L > block and Cn < 3:
                _check(C.signal(Cn, bits, L, i + j + Cn), bits, 48000, block, 1 if (i + j) % 2 else 12)


@pytest.mark.parametrize("block,Cn,bits,M", [(4096, 2, 16, 12), (4096, 3, 24, 1), (15360, 1, 16, 12), (16384, 1, 16, 12), (16384, 2, 24, 12), (16384, 8, 24, 1)])
def test_large_blocks(block, Cn, bits, M):
    """4096, 15360 (the largest 16-bit block whose analysis signal fits the Rice sums' LDS) and 16384: the largest block of the option, the int32
    image at 64 KiB; two frames, the second short."""
    _check(C.signal(Cn, bits, block + 37, block + Cn), bits, 48000, block, M)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_payload_at_any_byte_offset(offset):
    _check([C.resonant(700, 1, 24), C.resonant(700, 2, 24)], 24, 48000, 256, 12, offset=offset)
    _check([C.resonant(700, 1, 16)], 16, 48000, 256, 12, offset=offset)


def test_blocks_around_the_writers_step():
    """The frame kernel writes a subframe's residuals in steps of p2phd_flac_encode_threads, the first behind the warm-up samples: blocks
    around one and two steps, LPC chosen (a resonance), orders 1 and 12, both sample sizes."""
    T = _lib().lib().p2phd_flac_encode_threads()
    for block in (T - 1, T, T + 1, T + 12, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 12):
        for bits, M in ((16, 12), (24, 1)):
            L = 2 * block + T // 2
            x = np.array(C.resonant(L, block, bits))
            _check([x, x[::-1].copy()], bits, 48000, block, M)


def test_order_zero_is_the_existing_entry():
    """M = 0 through the new entry: p2phd_flac_encode's bytes, byte for byte, and its three launches."""
    for channels, bits, block in (([K.tone(3000, 16, 1), C.resonant(3000, 2)], 16, 1000), ([C.resonant(700, c, 24) for c in range(3)], 24, 192),
                                  ([K.tone(70000, 16, 3)], 16, 65535)):
        pay = E.payload(channels, bits)
        _count(reset=True)
        a = _call(pay, len(channels), bits, 48000, block, 0)
        assert _count(reset=True) == 3
        b = _call(pay, len(channels), bits, 48000, block, 0, entry="plain")
        assert a[0] == 0 and a == b and a[3]
        assert a[1] == _flacio().encode(pay, len(channels), bits, 48000, block)[0]


def test_runs_and_streams_repeat_the_bytes():
    channels = [C.resonant(3000, 1, 24), C.resonant(3000, 2, 24)]
    side = torch.cuda.Stream()
    a = _check(channels, 24, 96000, 1000, 12)[0]
    b = _check(channels, 24, 96000, 1000, 12)[0]
    c = _check(channels, 24, 96000, 1000, 12, stream=side)[0]
    assert a == b == c


def test_launch_counter_and_refusals():
    channels = [C.resonant(100, 1)]
    pay = E.payload(channels, 16)
    _count(reset=True)
    _check(channels, 16, 48000, 64, 12)
    assert _count() == 3                                                    # the frame kernel, the scan, the gather
    null = ctypes.c_void_p(None)
    nframes, worst, nwork = _flacio().encode_plan(1, 16, 100, 64)
    odd = torch.zeros((nwork + 16,), dtype=torch.uint8, device=DEV)
    for over, text in ((dict(M=13), b"lpc_order"), (dict(M=-1), b"lpc_order"), (dict(block=16385), b"at most 16384"), (dict(block=65535), b"at most 16384"),
                       (dict(C=0), b"channels"), (dict(C=9), b"channels"), (dict(bits=20), b"bits per sample"), (dict(L=0), b"L"), (dict(rate=0), b"rate"),
                       (dict(block=15), b"block"), (dict(block=65536), b"block"), (dict(cap=worst - 1), b"worst case"), (dict(nwork=nwork - 1), b"workspace"),
                       (dict(pay=null), b"null"), (dict(out=null), b"null"), (dict(lengths=null), b"null"), (dict(work=null), b"null"),
                       (dict(work=ctypes.c_void_p(odd.data_ptr() + 4)), b"aligned")):
        rc, got, ln, intact = _call(pay, 1, 16, 48000, 64, 12, over=over)
        assert rc != 0 and intact and _count() == 3, over
        assert text in _lib().lib().p2phd_last_error(), (over, _lib().lib().p2phd_last_error())
    assert _count(reset=True) == 3 and _count() == 0


def test_round_trip_on_the_device():
    """generate.flac_encode(lpc_order=M): the host encoder's bytes; behind flacio's header, through flacio.index_bytes and
    generate.flac_decode: the input samples."""
    from pix2pixhdaudiosr_amd.generate import flac_decode, flac_encode
    f = _flacio()
    for channels, bits, block, M in (([C.resonant(5000, 1), C.resonant(5000, 2)], 16, 1024, 12), ([C.resonant(900, c, 24) for c in range(3)], 24, 192, 8)):
        Cn, L = len(channels), len(channels[0])
        pay = E.payload(channels, bits)
        dev = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
        stream, lengths = flac_encode(dev, Cn, bits, 48000, block, lpc_order=M)
        nframes, worst, _ = f.encode_plan(Cn, bits, L, block)
        assert stream.numel() == worst and lengths.numel() == nframes + 1
        ln = lengths.cpu().numpy()
        want, hl = f.encode(pay, Cn, bits, 48000, block, lpc_order=M)
        assert ln.tolist() == hl.tolist() and stream[:int(ln[-1])].cpu().numpy().tobytes() == want
        assert len(want) < len(f.encode(pay, Cn, bits, 48000, block)[0])     # (LPC is in it)
        data = f.stream_header(ln, 48000, Cn, bits, L, block, hashlib.md5(pay).digest()) + want
        meta, table = f.index_bytes(data)
        out = flac_decode(torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV), table, meta)
        assert torch.equal(out.cpu(), torch.from_numpy(np.array(channels).astype(np.float32) * np.float32(2.0 ** -(bits - 1))))


def test_op_refusals():
    from pix2pixhdaudiosr_amd.generate import flac_encode
    dev = torch.zeros((240,), dtype=torch.uint8, device=DEV)
    _count(reset=True)
    for args, kw, text in (((dev, 1, 16, 48000), dict(lpc_order=13), "LPC order"), ((dev, 1, 16, 48000), dict(lpc_order=-1), "LPC order"),
                           ((dev, 1, 16, 48000), dict(lpc_order=True), "LPC order"), ((dev, 1, 16, 48000, 16385), dict(lpc_order=1), "at most 16384"),
                           ((dev, 9, 16, 48000), dict(lpc_order=4), "channels"), ((dev, 7, 16, 48000), dict(lpc_order=4), "whole frames")):
        with pytest.raises(ValueError, match=text):
            flac_encode(*args, **kw)
    assert _count() == 0


def test_stage_entry():
    """The measurement entry with the option: the frame kernel alone (1) or without its CRC-16 (2) counts one launch and leaves the stream
    and the lengths alone; the frame lengths it leaves in the workspace are the host encoder's."""
    L_ = _lib()
    pay = E.payload([C.resonant(300, 1)], 16)
    nframes, worst, nwork = _flacio().encode_plan(1, 16, 300, 64)
    raw = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
    out = torch.full((worst,), FILL, dtype=torch.uint8, device=DEV)
    lengths = torch.full((nframes + 1,), -7, dtype=torch.int64, device=DEV)
    work = torch.full((nwork,), POISON, dtype=torch.uint8, device=DEV)
    _count(reset=True)
    for stage, ok in ((1, True), (2, True), (0, False), (3, False)):
        rc = L_.lib().p2phd_flac_encode_lpc_stage(stage, L_.ptr(raw), 1, 16, 300, 48000, 64, 12, L_.ptr(out), worst, L_.ptr(lengths), L_.ptr(work), nwork,
                                                  L_.stream_ptr())
        torch.cuda.synchronize()
        assert (rc == 0) == ok and bool((out == FILL).all()) and bool((lengths == -7).all())
    assert b"stage must be" in L_.lib().p2phd_last_error() and _count(reset=True) == 2
    assert work[:8 * nframes].cpu().numpy().view(np.int64).tolist() == _flacio().encode(pay, 1, 16, 48000, 64, lpc_order=12)[1][:-1].tolist()
