"""The FLAC encoder on the host (csrc/flacenc.hip: p2phd_flac_encode_plan / p2phd_flac_encode_host; data/flacio.py: encode,
stream_header, write_stream, save) against the restatement tests/_flac_enc_ref.py, byte for byte: no tolerance anywhere.  Every
stream is also put through code this encoder did not write: the index (every CRC, the chaining), the host decoder and the
restatement's decoder of the FLAC reader."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import _flac_enc_cases as K
import _flac_enc_ref as E
import _flac_ref as R


def _flacio():
    from pix2pixhdaudiosr_amd.data import flacio
    return flacio


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L.lib()


def _check_stream(channels, bits, rate, block):
    """Host encoder == restatement, and the stream stands: -> (frames of the restatement, its decisions)."""
    f = _flacio()
    C, L = len(channels), len(channels[0])
    want, decisions = E.encode_frames(channels, bits, rate, block)
    pay = E.payload(channels, bits)
    got, lengths = f.encode(pay, C, bits, rate, block)
    assert lengths.tolist() == [len(x) for x in want] + [sum(map(len, want))]
    assert got == b"".join(want)
    nframes, worst, _ = f.encode_plan(C, bits, L, block)
    assert nframes == len(want) == -(-L // block) and len(got) <= worst
    head = f.stream_header(lengths, rate, C, bits, L, block, hashlib.md5(pay).digest())
    assert head == E.header(want, channels, bits, rate, block, md5=True)
    data = head + got
    meta, table = f.index_bytes(data)                                       # p2phd_flac_info / p2phd_flac_index: every CRC, the chaining
    assert (meta.sample_rate, meta.num_frames, meta.num_channels, meta.bits_per_sample, meta.min_block, meta.max_block, meta.num_flac_frames) == \
           (rate, L, C, bits, block, block, nframes)
    assert meta.md5 == R.md5_of([[int(v) for v in c] for c in channels], bits)
    assert table[:, 1].tolist() == lengths[:-1].tolist() and table[:, 3].tolist() == [min(block, L - a) for a in range(0, L, block)]
    assert np.array_equal(f.decode_frames(data, table, 0, nframes, C), np.array(channels))
    info, out = R.decode_stream(data)                                       # the restatement's decoder of the FLAC reader, every stream
    assert out == [[int(v) for v in c] for c in channels]
    assert (info["rate"], info["channels"], info["bits"], info["total"]) == (rate, C, bits, L)
    return want, decisions


def test_restatement_uses_the_readers_writer():
    R.self_check()
    assert E.trailing_zeros(4096) == 12 and E.trailing_zeros(100) == 2 and E.trailing_zeros(65535) == 0


@pytest.mark.parametrize("rate", K.RATES)
@pytest.mark.parametrize("block", K.BLOCKS)
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_matrix(C, bits, block, rate):
    """The whole product: every L of the matrix (a last frame of 1 .. 4 samples, where the order is bounded by bs - 1, included) at
    every (C, bits, block, rate) -- 2560 streams.  The signal of a case does not depend on its rate."""
    for i, L in enumerate(K.lengths_of(block)):
        channels, bits_, rate_, block_ = K.matrix_case(C, bits, block, L, i + 8 * (K.BLOCKS.index(block) + C + bits), rate)
        _check_stream(channels, bits_, rate_, block_)


@pytest.mark.parametrize("rate", K.RATES + (1, 65535, 65536, 655350, 655360, 1000000, 1048575))
def test_rate_codes(rate):
    """Every way a frame header states the rate, the edges of the 16-bit trailers included."""
    _check_stream([K.tone(40, 16, 1)], 16, rate, 16)


@pytest.mark.parametrize("block", [17, 255, 257, 65535])
def test_block_trailers(block):
    """Block sizes with the 8- and the 16-bit trailer; 65535 is the largest block there is."""
    _check_stream([K.tone(block + 3, 16, 2, noise=2)], 16, 48000, block)


@pytest.mark.parametrize("name", sorted(K.decisions()))
def test_decisions(name):
    """Each decision is asserted on the restatement first, then the host encoder's bytes are the restatement's."""
    (channels, bits, rate, block), expect = K.decisions()[name]
    want, decisions = E.encode_frames(channels, bits, rate, block)
    assert expect(decisions), decisions
    _check_stream(channels, bits, rate, block)
    size, pcm = sum(map(len, want)), len(E.payload(channels, bits))
    if name == "noise-verbatim":
        assert size == 6 + 1 + pcm + 2                                      # header, type byte, the samples as they are, CRC-16
        assert E.candidates(channels[0], 16, 16)[(0, 0)][0] > 8 + 1024 * 16
    if name == "tone-fixed":
        assert size < pcm // 2
    if name == "alternating-24bit":
        assert decisions[0][0] in (1, R.LEFT_SIDE, R.SIDE_RIGHT, R.MID_SIDE)
        side = E.candidates(channels[0] - channels[1], 25, 24)
        assert max(max(ks) for _, ks, _ in side.values()) >= 24
    if name == "alternating-24bit-mono":                                    # nothing beats VERBATIM; the candidates' sums pass 2^32, their k the twenties
        c = E.candidates(channels[0], 24, 24)
        assert min(t for t, _, _ in c.values()) > 8 + 512 * 24 and max(max(ks) for _, ks, _ in c.values()) >= 24
        assert int(np.abs(np.diff(channels[0])).sum()) * 2 > 1 << 32


def test_ties_are_ties():
    """The tie cases hold what they are named for: the pairs listed have equal bits, fewer than every other pair and than VERBATIM,
    and the restatement keeps the first; the k case has two equally cheap parameters in its only partition."""
    for name, pairs in K.TIES.items():
        (channels, bits, rate, block), _ = K.decisions()[name]
        c = E.candidates(channels[0], bits, bits)
        low = min(t for t, _, _ in c.values())
        assert sorted(op for op, (t, _, _) in c.items() if t == low) == pairs and low < 8 + block * bits
        assert E.choose(channels[0], bits, bits)[2][1:3] == min(pairs, key=lambda op: (op[1], op[0]))     # the smaller p, then the smaller o
    (channels, bits, rate, block), _ = K.decisions()["tie-k"]
    assert E.candidates(channels[0], bits, bits)[(0, 0)][2]


def test_plan():
    f = _flacio()
    # stereo full-scale noise: every subframe VERBATIM, independent -- within the bound, which also counts a side channel's extra bit
    ch = [K.full_noise(1000, 24, 1), K.full_noise(1000, 24, 2)]
    got, lengths = f.encode(E.payload(ch, 24), 2, 24, 48000, 256)
    nframes, worst, work = f.encode_plan(2, 24, 1000, 256)
    assert nframes == 4 and lengths[-1] <= worst
    per = lambda bs: 16 + -(-(2 * (8 + bs * 24) + bs) // 8) + 2                 # noqa: E731
    assert worst == 3 * per(256) + per(1000 - 768)
    assert work >= nframes * per(256) and work % 8 == 0
    out = (ctypes.c_int64 * 3)()
    a = ctypes.addressof(out)
    for args, text in (((0, 16, 10, 4096), b"channels"), ((9, 16, 10, 4096), b"channels"), ((1, 20, 10, 4096), b"bits"), ((1, 32, 10, 4096), b"bits"),
                       ((1, 16, 0, 4096), b"L"), ((1, 16, 10, 15), b"block"), ((1, 16, 10, 65536), b"block")):
        assert _lib().p2phd_flac_encode_plan(*args, ctypes.c_void_p(a), ctypes.c_void_p(a + 8), ctypes.c_void_p(a + 16)) != 0
        assert text in _lib().p2phd_last_error()
    assert _lib().p2phd_flac_encode_plan(1, 16, 10, 4096, None, None, None) != 0


def test_encode_refusals():
    f = _flacio()
    pay = E.payload([K.tone(40, 16, 1)], 16)
    for kw, text in ((dict(channels=9), "channels"), (dict(channels=0), "channels"), (dict(bits=20), "pcm16 or pcm24"), (dict(bits=32), "float32"),
                     (dict(block=15), "block"), (dict(block=65536), "block"), (dict(rate=0), "rate"), (dict(rate=1048576), "rate"),
                     (dict(channels=3), "whole frames")):
        args = dict(channels=1, bits=16, rate=48000, block=16)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            f.encode(pay, **args)
    with pytest.raises(ValueError, match="whole frames"):
        f.encode(b"", 1, 16, 48000, 16)
    with pytest.raises(ValueError, match="channel count"):
        f.encode(pay)
    with pytest.raises(ValueError, match="outside 16 bits"):
        f.encode(np.array([[40000]]), bits=16)
    # the C entry itself: a stream buffer below the plan's worst case, null pointers
    lengths = np.zeros(4, dtype=np.int64)
    out = np.zeros(8, dtype=np.uint8)
    p = np.frombuffer(pay, dtype=np.uint8)
    rc = _lib().p2phd_flac_encode_host(ctypes.c_void_p(p.ctypes.data), 1, 16, 40, 48000, 16, ctypes.c_void_p(out.ctypes.data), 8, ctypes.c_void_p(lengths.ctypes.data))
    assert rc != 0 and b"worst case" in _lib().p2phd_last_error() and not out.any() and not lengths.any()
    rc = _lib().p2phd_flac_encode_host(None, 1, 16, 40, 48000, 16, ctypes.c_void_p(out.ctypes.data), 1 << 20, ctypes.c_void_p(lengths.ctypes.data))
    assert rc != 0 and b"null" in _lib().p2phd_last_error()


def test_encode_takes_samples_or_payload():
    f = _flacio()
    ch = [K.tone(100, 24, 1), K.tone(100, 24, 2)]
    a = f.encode(np.array(ch), bits=24, rate=44100, block=64)
    b = f.encode(E.payload(ch, 24), 2, 24, 44100, 64)
    assert a[0] == b[0] and a[1].tolist() == b[1].tolist()
    assert f.encode(np.array(ch[0]), bits=24, rate=44100, block=64)[0] == f.encode(E.payload(ch[:1], 24), 1, 24, 44100, 64)[0]


@pytest.mark.parametrize("encoding", ["pcm16", "pcm24"])
def test_save_is_the_twin_of_wavio_save(tmp_path, encoding):
    """flacio.save then flacio.load == wavio.save then wavio.load, values beyond full scale and half-way cases included; the MD5 is the
    payload's, and the file is the restatement's."""
    from pix2pixhdaudiosr_amd.data import wavio
    f = _flacio()
    g = torch.Generator().manual_seed(3)
    w = torch.randn(2, 1000, generator=g) * 0.6
    w[0, :4] = torch.tensor([1.5, -1.5, 1.0, -1.0])
    w[1, :4] = torch.tensor([0.5 / 32768, 1.5 / 32768, -0.5 / 32768, 2.5 / 32768])
    for wave, name in ((w, "stereo"), (w[0], "mono")):
        pw, pf = str(tmp_path / (name + ".wav")), str(tmp_path / (name + ".flac"))
        wavio.save(pw, wave, 22050, encoding)
        n = f.save(pf, wave, 22050, encoding, block=192)
        a, ra = wavio.load(pw)
        b, rb = f.load(pf)
        assert ra == rb == 22050 and torch.equal(a, b)
        assert f.verify(pf) is True
        data = open(pf, "rb").read()
        assert len(data) == n
        pay, C = wavio.payload_of(wave, encoding)
        bits = f.ENCODINGS[encoding]
        q = np.frombuffer(pay, dtype=np.uint8).reshape(-1, bits // 8)
        ints = np.zeros((len(q), 4), dtype=np.uint8)
        ints[:, :bits // 8] = q
        ints = (ints.view("<i4").reshape(-1, C).T << (32 - bits)) >> (32 - bits)
        assert data == E.stream(list(ints.astype(np.int64)), bits, 22050, 192, md5=True)
        assert f.info(pf).md5 == hashlib.md5(pay).digest()


def test_save_and_write_stream_refusals(tmp_path):
    f = _flacio()
    p = str(tmp_path / "never.flac")
    w = torch.zeros(2, 64)
    for kw, text in ((dict(encoding="float32"), "float32"), (dict(encoding="pcm8"), "encoding"), (dict(block=15), "block"), (dict(block=65536), "block"),
                     (dict(sample_rate=1048576), "rate"), (dict(waveform=torch.zeros(9, 64)), "channels")):
        args = dict(waveform=w, sample_rate=48000, encoding="pcm16", block=4096)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            f.save(p, **args)
        assert not (tmp_path / "never.flac").exists()                       # refused before a file is opened
    frames, lengths = f.encode(E.payload([K.tone(40, 16, 1)], 16), 1, 16, 48000, 16)
    with pytest.raises(ValueError, match="16 bytes"):
        f.write_stream(p, frames, lengths, 48000, 1, 16, 40, 16, md5=b"short")
    with pytest.raises(ValueError, match="bytes of frames"):
        f.write_stream(p, frames[:-1], lengths, 48000, 1, 16, 40, 16)
    assert not (tmp_path / "never.flac").exists()
    # a longer buffer than the total (the device encoder's stream at its worst-case size): cut at the total
    n = f.write_stream(p, frames + b"\xAA" * 9, lengths, 48000, 1, 16, 40, 16)
    assert n == 42 + len(frames) and open(p, "rb").read()[42:] == frames and f.verify(p) is None
