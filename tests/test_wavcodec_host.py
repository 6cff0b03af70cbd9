"""Coded WAV input on the host (no GPU): the library's host decoders (csrc/wavcodec.hip) == the plain-Python restatement
(tests/_wavcodec_ref.py) == Python's audioop (tests/golden/wavcodec_audioop.npz, and audioop itself where it imports), bit for bit;
data/wavio.py on coded files == the same calls on their PCM16 twins; every refusal of the contract."""
import ctypes
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest

import _wavcodec_ref as R
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "wavcodec_audioop.npz")


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib()


def _err():
    return _L().p2phd_last_error().decode()


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data if a.size else None)


def host_g711(payload, frames, channels, law, ld=None):
    ld = frames if ld is None else ld
    src = np.frombuffer(bytes(payload), dtype=np.uint8)
    out = np.zeros((channels, ld), dtype=np.float32)
    rc = _L().p2phd_g711_decode_host(_vp(src), frames, channels, law, _vp(out), ld)
    return rc, out


def host_ima(payload, channels, block_align, first, count, ld=None):
    ld = count if ld is None else ld
    src = np.frombuffer(bytes(payload), dtype=np.uint8)
    out = np.zeros((channels, ld), dtype=np.float32)
    rc = _L().p2phd_ima_decode_host(_vp(src), src.size, channels, block_align, first, count, _vp(out), ld)
    return rc, out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the restatement against audioop -------------------------------------------------------------------------------------------------
def test_restatement_is_audioop_golden():
    g = np.load(GOLDEN)
    assert g["ulaw"].shape == (256,) and g["alaw"].shape == (256,) and g["ima_out"].shape == (200, 64)
    assert np.array_equal(R.ULAW_TABLE, g["ulaw"].astype(np.int32))
    assert np.array_equal(R.ALAW_TABLE, g["alaw"].astype(np.int32))
    assert (int(R.ULAW_TABLE.min()), int(R.ULAW_TABLE.max())) == (-32124, 32124)
    assert (int(R.ALAW_TABLE.min()), int(R.ALAW_TABLE.max())) == (-32256, 32256)
    for k in range(200):
        got = R.ima_chain(int(g["ima_pred"][k]), int(g["ima_index"][k]), [int(n) for n in g["ima_nibbles"][k]])
        assert got == [int(v) for v in g["ima_out"][k]], k
    # the fixture does reach both clamps of the predictor
    assert int(g["ima_out"].min()) == -32768 and int(g["ima_out"].max()) == 32767


def test_restatement_is_audioop_itself():
    audioop = pytest.importorskip("audioop")
    codes = bytes(range(256))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2"), R.ULAW_TABLE)
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2"), R.ALAW_TABLE)
    rng = np.random.default_rng(5)
    for _ in range(50):
        pred, index = int(rng.integers(-32768, 32768)), int(rng.integers(0, 89))
        nib = [int(n) for n in rng.integers(0, 16, size=64)]
        packed = bytes((a << 4) | b for a, b in zip(nib[0::2], nib[1::2]))         # audioop: high nibble first
        ref = np.frombuffer(audioop.adpcm2lin(packed, 2, (pred, index))[0], dtype="<i2")
        assert R.ima_chain(pred, index, nib) == [int(v) for v in ref]


def test_host_chains_are_audioop_golden():
    """The library's host decoder on the golden chains: every chain as one mono block of 1 + 64 samples."""
    g = np.load(GOLDEN)
    align = 4 + 32
    payload = bytearray()
    for k in range(200):
        nib = g["ima_nibbles"][k].astype(np.uint32)
        body = bytes(int(nib[2 * i]) | (int(nib[2 * i + 1]) << 4) for i in range(32))       # WAVE: low nibble first
        payload += struct.pack("<hBB", int(g["ima_pred"][k]), int(g["ima_index"][k]), 0) + body
    rc, out = host_ima(payload, 1, align, 0, 200 * 65)
    assert rc == 0, _err()
    want = np.concatenate([g["ima_pred"][:, None], g["ima_out"]], axis=1).reshape(1, -1)
    assert np.array_equal(bits(out), bits(R.scale(want)))


# ---- G.711 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("law", [R.ULAW, R.ALAW])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_g711_host_all_codes(law, channels):
    rng = np.random.default_rng(channels)
    frames = 256 + 37
    payload = np.concatenate([np.repeat(np.arange(256, dtype=np.uint8), channels), rng.integers(0, 256, 37 * channels).astype(np.uint8)])
    rc, out = host_g711(payload, frames, channels, law, ld=frames + 5)
    assert rc == 0, _err()
    want = R.scale(R.g711_decode(payload, frames, channels, law))
    assert np.array_equal(bits(out[:, :frames]), bits(want))
    assert not out[:, frames:].any()
    assert host_g711(b"", 0, channels, law)[0] == 0


def test_g711_encode_round_trip():
    for law in (R.ULAW, R.ALAW):
        t = R.g711_table(law)
        codes = np.frombuffer(R.g711_encode(t[None, :], law), dtype=np.uint8)
        assert np.array_equal(t[codes], t)                              # every value of the table encodes to a code of that value


# ---- IMA: host decoder == restatement -------------------------------------------------------------------------------------------------
ALIGN_OF_SPB = {9: 8, 505: 256, 2041: 1024}                               # block_align per channel


def _frame_counts(spb):
    return [0, 1, spb - 1, spb, spb + 1, 3 * spb + 3]


@pytest.mark.parametrize("spb", [9, 505, 2041])
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_ima_host_matches_restatement(channels, spb):
    align = ALIGN_OF_SPB[spb] * channels
    assert R.ima_spb(channels, align) == spb
    rng = np.random.default_rng(spb * 10 + channels)
    payload = bytearray(rng.integers(0, 256, 4 * align, dtype=np.uint8).tobytes())     # random bytes: valid apart from the header index
    for B in range(4):
        for c in range(channels):
            payload[B * align + 4 * c + 2] = int(rng.integers(0, 89))
    assert _L().p2phd_ima_frames(len(payload), channels, align) == 4 * spb == R.ima_frames(len(payload), channels, align)
    ref = R.scale(R.ima_decode(payload, channels, align))
    for n in _frame_counts(spb):
        rc, out = host_ima(payload, channels, align, 0, n, ld=n + 3)
        assert rc == 0, _err()
        assert np.array_equal(bits(out[:, :n]), bits(ref[:, :n])), n
        assert not out[:, n:].any()
    for first, count in [(1, spb), (spb - 1, 2), (spb, spb), (spb + 1, 2 * spb), (4 * spb - 1, 1), (4 * spb, 0), (2 * spb - 3, 7)]:
        rc, out = host_ima(payload, channels, align, first, count)
        assert rc == 0, _err()
        assert np.array_equal(bits(out), bits(ref[:, first:first + count])), (first, count)


def test_ima_host_many_blocks_cost_one_pass():
    """More blocks than the device decoder's grid takes in one trip (tests/test_gpu_wavcodec.py compares with this entry there): a
    block is decoded from its own bytes alone, so windows of the payload are slices of the whole and a window costs its blocks."""
    L = _L()
    blocks = L.p2phd_ima_blocks_per_workgroup(1, 8) * L.p2phd_ima_max_workgroups() + 1
    rng = np.random.default_rng(1)
    payload = rng.integers(0, 256, (blocks, 8), dtype=np.uint8)
    payload[:, 2] = rng.integers(0, 89, blocks, dtype=np.uint8)
    rc, whole = host_ima(payload.tobytes(), 1, 8, 0, blocks * 9)
    assert rc == 0, _err()
    assert np.array_equal(bits(whole[0, 0::9]), bits(R.scale(payload[:, :2].copy().view("<i2")[:, 0])))      # every block's first sample: its header's
    for B in (0, 1, 70000, blocks - 2, blocks - 1):
        assert np.array_equal(bits(whole[:, B * 9:B * 9 + 9]), bits(R.scale(R.ima_decode(payload[B].tobytes(), 1, 8)))), B
        rc, part = host_ima(payload.tobytes(), 1, 8, B * 9 + 2, 9 if B < blocks - 1 else 7)
        assert rc == 0 and np.array_equal(bits(part), bits(whole[:, B * 9 + 2:B * 9 + 11]))


def test_ima_host_saturation_and_pinned_index():
    """Chains that run into +-32767 / -32768, and the index pinned at 0 and at 88."""
    def block(pred, index, nibble, groups=8):
        return struct.pack("<hBB", pred, index, 0) + bytes([nibble | (nibble << 4)]) * (4 * groups)
    cases = [block(32000, 88, 7), block(-32000, 88, 15), block(32767, 88, 7), block(-32768, 88, 15),
             block(0, 0, 0), block(0, 0, 8), block(100, 88, 7), block(-5, 3, 3), block(32767, 0, 0), block(-32768, 0, 8)]
    payload = b"".join(cases)
    ref = R.ima_decode(payload, 1, 36)
    assert ref.max() == 32767 and ref.min() == -32768
    rc, out = host_ima(payload, 1, 36, 0, ref.shape[1])
    assert rc == 0, _err()
    assert np.array_equal(bits(out), bits(R.scale(ref)))
    # index pinned: nibble 0 at index 0 keeps adding STEP[0] >> 3 = 0; nibble 7 at 88 adds 32767 + 16383 + 8191 + 4095
    assert ref[0, 65 * 4 + 1] == 0 and ref[0, 65 * 6 + 1] == 32767


def test_ima_host_clamps_header_index_and_scan_finds_it():
    rng = np.random.default_rng(9)
    C, align = 2, 2 * 36
    payload = bytearray(rng.integers(0, 256, 6 * align, dtype=np.uint8).tobytes())
    for B in range(6):
        for c in range(C):
            payload[B * align + 4 * c + 2] = int(rng.integers(0, 89))
    L = _L()
    src = np.frombuffer(bytes(payload), dtype=np.uint8)
    assert L.p2phd_ima_scan_host(_vp(src), src.size, C, align) == -1
    payload[4 * align + 4 + 2] = 89
    payload[5 * align + 2] = 255
    src = np.frombuffer(bytes(payload), dtype=np.uint8)
    assert L.p2phd_ima_scan_host(_vp(src), src.size, C, align) == 4
    assert L.p2phd_ima_scan_host(_vp(src), 4 * align + 7, C, align) == -1          # block 4 without its headers holds no sample
    assert L.p2phd_ima_scan_host(_vp(src), 4 * align + 8, C, align) == 4
    rc, out = host_ima(payload, C, align, 0, 6 * 65)                                # the decoder without the scan clamps to 88
    assert rc == 0, _err()
    assert np.array_equal(bits(out), bits(R.scale(R.ima_decode(payload, C, align))))
    fixed = bytearray(payload)
    fixed[4 * align + 4 + 2] = fixed[5 * align + 2] = 88
    assert np.array_equal(R.ima_decode(payload, C, align), R.ima_decode(fixed, C, align))


def test_ima_host_partial_last_block():
    rng = np.random.default_rng(2)
    C, align = 2, 2 * 36
    full = bytearray(rng.integers(0, 256, 3 * align, dtype=np.uint8).tobytes())
    for B in range(3):
        for c in range(C):
            full[B * align + 4 * c + 2] = 40
    for cut, frames in [(2 * align + 7, 130), (2 * align + 8, 131), (2 * align + 15, 131), (2 * align + 16, 139), (2 * align + 8 * 4, 155)]:
        payload = bytes(full[:cut])
        assert _L().p2phd_ima_frames(cut, C, align) == frames == R.ima_frames(cut, C, align)
        rc, out = host_ima(payload, C, align, 0, frames)
        assert rc == 0, _err()
        assert np.array_equal(bits(out), bits(R.scale(R.ima_decode(payload, C, align)))), cut
        assert host_ima(payload, C, align, 0, frames + 1)[0] != 0 and "payload holds" in _err()


def test_host_entry_refusals():
    L = _L()
    buf = np.zeros(64, dtype=np.uint8)
    out = np.zeros(64, dtype=np.float32)
    assert L.p2phd_g711_decode_host(_vp(buf), 4, 1, 2, _vp(out), 4) != 0 and "law" in _err()
    assert L.p2phd_g711_decode_host(_vp(buf), 4, 0, 0, _vp(out), 4) != 0 and "channels" in _err()
    assert L.p2phd_g711_decode_host(_vp(buf), 4, 1, 0, _vp(out), 3) != 0 and "ld" in _err()
    assert L.p2phd_g711_decode_host(None, 4, 1, 0, _vp(out), 4) != 0 and "null" in _err()
    for C, align in [(0, 8), (9, 72), (1, 4), (1, 10), (2, 24 + 4), (1, 65536)]:
        assert L.p2phd_ima_frames(64, C, align) == -1 and "block_align" in _err()
        assert L.p2phd_ima_decode_host(_vp(buf), 64, C, align, 0, 1, _vp(out), 1) != 0 and "block_align" in _err()
        assert L.p2phd_ima_scan_host(_vp(buf), 64, C, align) == -2
        assert L.p2phd_ima_blocks_per_workgroup(C, align) == 0
    assert L.p2phd_ima_decode_host(_vp(buf), 64, 1, 8, 0, 9 * 8 + 1, _vp(out), 80) != 0 and "payload holds" in _err()
    assert L.p2phd_ima_decode_host(_vp(buf), 64, 1, 8, -1, 1, _vp(out), 8) != 0
    assert L.p2phd_ima_decode_host(_vp(buf), 64, 1, 8, 0, 9, _vp(out), 8) != 0 and "ld" in _err()
    assert L.p2phd_ima_decode_host(None, 64, 1, 8, 0, 9, _vp(out), 9) != 0 and "null" in _err()
    assert L.p2phd_ima_blocks_per_workgroup(1, 8) >= 1 and L.p2phd_ima_max_workgroups() >= 1


# ---- data/wavio.py ---------------------------------------------------------------------------------------------------------------------
def _twin(tmp_path, name, kind, channels, frames, seed=0, **kw):
    """Writes a coded file and its PCM16 twin -> (coded path, twin path, ints [channels, frames'])."""
    x = R.speech_like(channels, frames, seed)
    coded, twin = str(tmp_path / (name + ".wav")), str(tmp_path / (name + "_pcm.wav"))
    if kind == "ima":
        align = kw.pop("block_align", 36 * channels)
        payload = R.ima_encode(x, align, partial=kw.pop("partial", True))
        ints = R.ima_decode(payload, channels, align)
        fact = kw.pop("fact", "own")
        fact = ints.shape[1] if fact == "own" else fact
        if fact is not None:
            ints = ints[:, :fact]
        R.write_coded_wav(coded, R.TAG_IMA, payload, 8000, channels, block_align=align, fact=fact, **kw)
    else:
        law = R.ULAW if kind == "ulaw" else R.ALAW
        payload = R.g711_encode(x, law)
        ints = R.g711_decode(payload, frames, channels, law)
        R.write_coded_wav(coded, R.TAG_ULAW if kind == "ulaw" else R.TAG_ALAW, payload, 8000, channels, **kw)
    R.write_pcm16_wav(twin, ints, 8000)
    return coded, twin, ints


@pytest.mark.parametrize("kind,channels", [("ulaw", 1), ("alaw", 2), ("ulaw", 3), ("ima", 1), ("ima", 2), ("ima", 8)])
def test_wavio_load_equals_pcm16_twin(tmp_path, kind, channels):
    from pix2pixhdaudiosr_amd.data import audiofile, wavio
    frames = 65 * 5 + 20
    coded, twin, ints = _twin(tmp_path, "a", kind, channels, frames, seed=channels)
    m, t = wavio.info(coded), wavio.info(twin)
    assert isinstance(m, wavio.WavInfo) and len(m) == 7
    assert m[:3] == t[:3] and m.num_frames == ints.shape[1]
    assert m.bits_per_sample == (4 if kind == "ima" else 8) and m.format_tag == {"ulaw": 7, "alaw": 6, "ima": 0x11}[kind]
    assert m.block_align == (36 * channels if kind == "ima" else channels)
    a, sr = wavio.load(coded)
    b, _ = wavio.load(twin)
    assert sr == 8000 and a.dtype == b.dtype and a.shape == b.shape
    assert np.array_equal(bits(a.numpy()), bits(b.numpy()))
    assert audiofile.kind(coded) == "wav"
    assert np.array_equal(bits(audiofile.load(coded, 3, 100)[0].numpy()), bits(b.numpy()[:, 3:103]))
    payload, meta = wavio.read_payload(coded)
    assert meta == m and wavio.coded_frames(m.format_tag, channels, m.block_align, len(payload)) == m.num_frames
    assert bytes(payload) == open(coded, "rb").read()[m.data_offset:m.data_offset + len(payload)]


@pytest.mark.parametrize("channels", [1, 2])
def test_wavio_windows_around_block_boundaries(tmp_path, channels):
    from pix2pixhdaudiosr_amd.data import wavio
    spb = 65
    coded, twin, ints = _twin(tmp_path, "w", "ima", channels, spb * 4 + 30, seed=7)
    whole = wavio.load(coded)[0].numpy()
    assert np.array_equal(bits(whole), bits(R.scale(ints)))
    n = whole.shape[1]
    for off in [0, 1, spb - 1, spb, spb + 1, 2 * spb - 1, 2 * spb, 4 * spb, n - 1, n, n + 5]:
        for cnt in [0, 1, 2, spb - 1, spb, spb + 1, 2 * spb + 3, -1]:
            got = wavio.load(coded, off, cnt)[0].numpy()
            lo = min(off, n)
            hi = n if cnt < 0 else min(n, lo + cnt)
            assert got.shape == (channels, hi - lo), (off, cnt)
            assert np.array_equal(bits(got), bits(whole[:, lo:hi])), (off, cnt)
    coded, twin, ints = _twin(tmp_path, "g", "ulaw", channels, 300, seed=8)
    whole = wavio.load(coded)[0].numpy()
    for off, cnt in [(0, 0), (0, 1), (17, 100), (299, 5), (300, 1), (400, -1)]:
        got = wavio.load(coded, off, cnt)[0].numpy()
        lo = min(off, 300)
        assert np.array_equal(bits(got), bits(whole[:, lo:300 if cnt < 0 else min(300, lo + cnt)]))


def test_wavio_fact_absent_shorter_longer_and_partial_blocks(tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    C, align, spb = 2, 72, 65
    x = R.speech_like(C, 3 * spb, 3)
    payload = R.ima_encode(x, align)
    full = R.ima_decode(payload, C, align)
    p = str(tmp_path / "f.wav")
    for fact, want in [(None, 3 * spb), (3 * spb - 10, 3 * spb - 10), (2 * spb, 2 * spb), (1, 1), (0, 0), (3 * spb + 100, 3 * spb)]:
        R.write_coded_wav(p, R.TAG_IMA, payload, 8000, C, block_align=align, fact=fact)
        assert wavio.info(p).num_frames == want, fact
        got = wavio.load(p)[0].numpy()
        assert np.array_equal(bits(got), bits(R.scale(full[:, :want]))), fact
    # a trailing partial block: headers and k whole groups (k = 0 and k > 0); anything shorter is ignored
    for cut, want in [(2 * align + 8, 2 * spb + 1), (2 * align + 8 + 8 * 3, 2 * spb + 25), (2 * align + 5, 2 * spb), (2 * align + 8 + 11, 2 * spb + 9)]:
        R.write_coded_wav(p, R.TAG_IMA, payload[:cut], 8000, C, block_align=align, fact=None)
        assert wavio.info(p).num_frames == want, cut
        got = wavio.load(p)[0].numpy()
        assert np.array_equal(bits(got), bits(R.scale(full[:, :want]))), cut
        assert np.array_equal(bits(wavio.load(p, 2 * spb - 2, 40)[0].numpy()), bits(R.scale(full[:, 2 * spb - 2:min(want, 2 * spb + 38)])))
        raw, meta = wavio.read_payload(p)
        assert bytes(raw) == payload[:cut] and meta.num_frames == want
    # a data chunk that promises more than the file holds
    R.write_coded_wav(p, R.TAG_IMA, payload[:2 * align], 8000, C, block_align=align, fact=3 * spb, data_size=3 * align)
    assert wavio.info(p).num_frames == 2 * spb
    assert np.array_equal(bits(wavio.load(p)[0].numpy()), bits(R.scale(full[:, :2 * spb])))
    # G.711: fact and no fact
    g = R.g711_encode(x, R.ALAW)
    for fact, want in [(None, 3 * spb), (100, 100), (10 ** 6, 3 * spb)]:
        R.write_coded_wav(p, R.TAG_ALAW, g, 8000, C, fact=fact)
        assert wavio.info(p).num_frames == want
        assert np.array_equal(bits(wavio.load(p)[0].numpy()), bits(R.scale(R.g711_decode(g, want, C, R.ALAW))))


def test_wavio_extensible_and_chosen_block_align(tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    p = str(tmp_path / "e.wav")
    x = R.speech_like(1, 1200, 4)
    for align in (8, 256, 1024):
        payload = R.ima_encode(x, align, partial=False)
        R.write_coded_wav(p, R.TAG_IMA, payload, 8000, 1, block_align=align, fact=1200, extensible=True)
        m = wavio.info(p)
        assert (m.format_tag, m.block_align, m.num_frames, m.bits_per_sample) == (0x11, align, 1200, 4)
        assert np.array_equal(bits(wavio.load(p)[0].numpy()), bits(R.scale(R.ima_decode(payload, 1, align, 1200))))
    g = R.g711_encode(x, R.ULAW)
    R.write_coded_wav(p, R.TAG_ULAW, g, 8000, 1, extensible=True)
    assert wavio.info(p).format_tag == 7
    assert np.array_equal(bits(wavio.load(p)[0].numpy()), bits(R.scale(R.g711_decode(g, 1200, 1, R.ULAW))))


def test_wavio_refusals(tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    p = str(tmp_path / "r.wav")
    x = R.speech_like(1, 200, 5)
    g, ima = R.g711_encode(x, R.ULAW), R.ima_encode(x, 36)

    def refused(match, *a, **kw):
        R.write_coded_wav(p, *a, **kw)
        with pytest.raises(ValueError, match=match) as e:
            wavio.info(p)
        assert p in str(e.value)
        with pytest.raises(ValueError):
            wavio.load(p)
        with pytest.raises(ValueError):
            wavio.read_payload(p)

    refused("8 bits per sample", R.TAG_ULAW, g, 8000, 1, bits=16)
    refused("8 bits per sample", R.TAG_ALAW, g, 8000, 1, bits=4)
    refused("4 bits per sample", R.TAG_IMA, ima, 8000, 1, block_align=36, bits=8)
    refused("1 to 8 channels", R.TAG_ULAW, g[:198], 8000, 9, block_align=9)
    refused("1 to 8 channels", R.TAG_IMA, ima, 8000, 9, block_align=72, samples_per_block=False)
    refused("block_align", R.TAG_IMA, ima, 8000, 1, block_align=4, samples_per_block=False)
    refused("block_align", R.TAG_IMA, ima, 8000, 1, block_align=38, samples_per_block=False)
    refused("block_align", R.TAG_IMA, ima, 8000, 2, block_align=36, samples_per_block=False)
    refused("block_align", R.TAG_ULAW, g, 8000, 1, block_align=2)
    refused("samples per block", R.TAG_IMA, ima, 8000, 1, block_align=36, samples_per_block=64)
    # a block header whose step index is above 88: load names file and block (info reads no block)
    bad = bytearray(ima)
    bad[2 * 36 + 2] = 89
    R.write_coded_wav(p, R.TAG_IMA, bytes(bad), 8000, 1, block_align=36, fact=200)
    assert wavio.info(p).num_frames == 200
    with pytest.raises(ValueError, match="block 2") as e:
        wavio.load(p)
    assert p in str(e.value)
    with pytest.raises(ValueError, match="block 2"):
        wavio.load(p, 65 * 2 + 3, 4)
    assert wavio.load(p, 0, 130)[0].shape == (1, 130)                       # a window in front of it reads


def test_wavio_other_tags_still_refused_with_todays_text(tmp_path):
    from pix2pixhdaudiosr_amd.data import wavio
    p = str(tmp_path / "t.wav")
    for tag, bits_ in [(2, 4), (0x31, 0), (0x45, 4), (0x55, 0)]:
        R.write_coded_wav(p, tag, b"\0" * 512, 8000, 1, block_align=256, bits=bits_)
        with pytest.raises(ValueError) as e:
            wavio.info(p)
        assert str(e.value) == f"{p}: unsupported WAVE format (tag {tag}, {bits_} bit, 1 ch)"


def test_wavio_pcm_unchanged_beside_a_fact_chunk(tmp_path):
    """A PCM file, with and without a fact chunk in front of its data: the fields and samples of before."""
    from pix2pixhdaudiosr_amd.data import wavio
    x = R.speech_like(2, 50, 6)
    p, q = str(tmp_path / "p.wav"), str(tmp_path / "q.wav")
    R.write_pcm16_wav(p, x, 16000)
    raw = open(p, "rb").read()
    open(q, "wb").write(raw[:36] + b"fact" + struct.pack("<II", 4, 7) + raw[36:])
    assert wavio.info(p) == wavio.WavInfo(16000, 50, 2, 16, 1, 44, 4)
    assert wavio.info(q) == wavio.WavInfo(16000, 50, 2, 16, 1, 56, 4)
    assert np.array_equal(bits(wavio.load(q)[0].numpy()), bits(R.scale(x)))
    assert bytes(wavio.read_payload(q)[0]) == raw[44:]


@pytest.mark.parametrize("kind", ["ulaw", "ima"])
def test_audio_dataset_item_equals_twin(tmp_path, kind):
    """The datasets need nothing beyond what wavio gives them: an item from a coded file is the item from its PCM16 twin."""
    import torch
    from pix2pixhdaudiosr_amd.data import audio_dataset
    (tmp_path / "coded").mkdir()
    (tmp_path / "twin").mkdir()
    coded, twin, ints = _twin(tmp_path, "d", kind, 1, 8000 * 2, seed=11, **({"block_align": 256, "partial": False} if kind == "ima" else {}))
    os.replace(coded, str(tmp_path / "coded" / "d.wav"))
    os.replace(twin, str(tmp_path / "twin" / "d.wav"))
    items = []
    for sub in ("coded", "twin"):
        opt = SimpleNamespace(dataroot=str(tmp_path / sub), lr_sampling_rate=4000, hr_sampling_rate=8000, segment_length=2048, n_fft=64,
                              hop_length=32, win_length=64, center=True, seed=3)
        ds = audio_dataset.AudioDataset(opt)                             # (seeds torch: both draw the same offsets)
        assert len(ds) == 1
        items.append([ds[0], ds[0], ds[0]])
    for a, b in zip(*items):
        assert a["raw_len"] == b["raw_len"] == 2048 and a["rate"] == b["rate"] == 8000
        assert torch.equal(a["raw"].view(torch.int32), b["raw"].view(torch.int32))
    assert not torch.equal(items[0][0]["raw"], items[0][1]["raw"])           # (the three items are different windows)
