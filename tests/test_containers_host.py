"""AIFF / AIFF-C, AU and NIST SPHERE input on the host (data/containers.py; no device): every file decodes to exactly the float32
samples wavio.load returns for its WAV twin.  Anchors: files written by Python's aifc / sunau with what their readers return
(tests/golden/containers_stdlib.npz always, the live modules where they import), and for what the stdlib cannot make the struct / numpy
restatement of the specifications in tests/_containers_ref.py."""
import os
import struct
import wave
from types import SimpleNamespace

import numpy as np
import pytest

import _containers_ref as R
import _wavcodec_ref as W
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "containers_stdlib.npz")
CODINGS = R.codings()
bits = R.bits


def _C():
    from pix2pixhdaudiosr_amd.data import containers
    return containers


def _put(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _golden():
    g = np.load(GOLDEN)
    return {k[5:]: (g[k].tobytes(), g["ints_" + k[5:]]) for k in g.files if k.startswith("file_")}


def _width_of(name):
    """Bytes per decoded sample of a golden file: the G.711 ones decode to 16-bit values."""
    return {"none1": 1, "none2": 2, "none3": 3, "none4": 4, "2": 1, "3": 2, "4": 3, "5": 4}.get(name.split("_")[1], 2)


# ---- the readers against the stdlib ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(_golden()))
def test_golden_file_equals_stdlib_reader_and_wav_twin(tmp_path, name):
    from pix2pixhdaudiosr_amd.data import audiofile, wavio
    data, ints = _golden()[name]
    width = _width_of(name)
    p = _put(tmp_path, name + ".bin", data)
    got, sr = _C().load(p)
    want = np.ascontiguousarray(ints.T).astype(np.float32) * np.float32(2.0 ** -(8 * width - 1))
    assert got.dtype.is_floating_point and tuple(got.shape) == want.shape and sr == (16000 if name.startswith("aifc") else 8000)
    assert np.array_equal(bits(got.numpy()), bits(want))
    # the twin, written by the wave module: little-endian, 8-bit samples unsigned
    twin = str(tmp_path / "twin.wav")
    w = wave.open(twin, "wb")
    w.setnchannels(ints.shape[1]), w.setsampwidth(width), w.setframerate(sr)
    w.writeframes(R.int_bytes(ints.T + (128 if width == 1 else 0), width, big=False))
    w.close()
    ref, sr2 = wavio.load(twin)
    assert sr2 == sr and np.array_equal(bits(got.numpy()), bits(ref.numpy()))
    assert np.array_equal(bits(audiofile.load(p)[0].numpy()), bits(ref.numpy()))
    meta = _C().info(p)
    assert meta[:3] == wavio.info(twin)[:3] and meta.container == ("aiff" if name.startswith("aifc") else "au")
    payload, meta2 = _C().read_payload(p)
    assert meta2 == meta and bytes(payload) == data[meta.data_offset:meta.data_offset + meta.num_frames * meta.block_align]


def test_golden_fixture_is_what_the_live_modules_give(tmp_path):
    """Where aifc and sunau still import: their readers return today what the fixture recorded."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        aifc, sunau, audioop = pytest.importorskip("aifc"), pytest.importorskip("sunau"), pytest.importorskip("audioop")
    for name, (data, ints) in _golden().items():
        p = _put(tmp_path, name, data)
        r = (aifc if name.startswith("aifc") else sunau).open(p, "rb")
        raw, C = r.readframes(r.getnframes()), r.getnchannels()
        r.close()
        if name == "sunau_27":
            raw = audioop.alaw2lin(raw, 2)
        width = _width_of(name)
        if name.split("_")[1] in ("ulaw", "alaw", "1", "27"):
            live = np.frombuffer(raw, dtype="<i2").astype(np.int64)
        else:
            b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width).astype(np.int64)
            live = sum(b[:, k] << (8 * (width - 1 - k)) for k in range(width))
            live = live - ((live >> (8 * width - 1)) << (8 * width))
        assert np.array_equal(live.reshape(-1, C), ints), name


# ---- every coding against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("name", sorted(CODINGS))
def test_coding_equals_restatement_and_twin(tmp_path, name, channels):
    from pix2pixhdaudiosr_amd.data import audiofile, wavio
    frames = 67
    data, want, twin = CODINGS[name](np.random.default_rng(7 * channels + len(name)), channels, frames)
    p = _put(tmp_path, "x.bin", data)
    got, sr = audiofile.load(p)
    assert tuple(got.shape) == (channels, frames) and np.array_equal(bits(got.numpy()), bits(want)), name
    q = str(tmp_path / "twin.wav")
    R.write_twin(q, twin, sr, channels)
    ref, sr2 = wavio.load(q)
    assert sr2 == sr and np.array_equal(bits(got.numpy()), bits(ref.numpy()))
    meta = audiofile.info(p)
    assert meta.container == name.split("-")[0].replace("aifc", "aiff") and (meta.sample_rate, meta.num_frames, meta.num_channels) == (sr, frames, channels)
    g711 = "law" in name.lower() or name in ("au-1", "au-27")
    assert meta.format_tag == ((6 if name in ("au-27", "aifc-alaw", "aifc-ALAW", "sphere-alaw") else 7) if g711 else twin[0])
    assert meta.block_align == channels * meta.bits_per_sample // 8
    payload, _ = _C().read_payload(p)
    assert bytes(payload) == data[meta.data_offset:meta.data_offset + frames * meta.block_align] and len(data) >= meta.data_offset + len(payload)


def test_info_fields():
    C = _C()
    assert C.AudioInfo._fields[:7] == ("sample_rate", "num_frames", "num_channels", "bits_per_sample", "format_tag", "data_offset", "block_align")
    assert C.AudioInfo._fields[7:] == ("big_endian", "signed8", "container", "coding")
    assert [C.kind_of(h) for h in (b"FORM", b".snd", b"NIST_1A", b"RIFF", b"fLaC", b"", b"dns.")] == ["aiff", "au", "sphere", None, None, None, None]


def test_info_flags(tmp_path):
    rng = np.random.default_rng(1)
    want = {"aiff-8": (True, False, True), "aiff-16": (False, True, False), "aifc-sowt": (False, False, False), "aifc-raw": (False, False, False),
            "au-2": (True, False, True), "au-4": (False, True, False), "au-6": (False, True, False), "sphere-pcm-01": (False, False, False),
            "sphere-pcm-10": (False, True, False), "au-1": (False, False, False)}
    for name, (signed8, big, _) in want.items():
        meta = _C().info(_put(tmp_path, "f.bin", CODINGS[name](rng, 2, 5)[0]))
        assert (meta.signed8, meta.big_endian) == (signed8, big), name
    assert _C().info(_put(tmp_path, "f.bin", CODINGS["aifc-ulaw"](rng, 2, 5)[0])).coding == "ulaw"
    assert _C().info(_put(tmp_path, "f.bin", CODINGS["au-27"](rng, 2, 5)[0])).coding == "27"
    assert _C().info(_put(tmp_path, "f.bin", CODINGS["sphere-mu-law"](rng, 2, 5)[0])).coding == "mu-law"


# ---- windows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aiff-24", "aifc-ulaw", "au-3", "au-7", "sphere-pcm-10", "sphere-alaw"])
def test_windows_are_slices_of_the_whole(tmp_path, name):
    frames = 200
    p = _put(tmp_path, "w.bin", CODINGS[name](np.random.default_rng(3), 3, frames)[0])
    whole = _C().load(p)[0]
    assert whole.shape[1] == frames
    for start, count in ((0, 0), (0, 1), (1, 1), (0, 7), (1, 64), (99, 3), (100, -1), (199, 1), (199, 5), (200, 4), (250, 1), (-3, 2), (0, 500)):
        got = _C().load(p, start, count)[0]
        a = min(max(start, 0), frames)
        b = frames if count < 0 else min(frames, a + count)
        assert np.array_equal(bits(got.numpy()), bits(whole[:, a:b].numpy())), (start, count)


# ---- chunk layout ------------------------------------------------------------------------------------------------------------------
def test_aiff_chunk_layout(tmp_path):
    rng = np.random.default_rng(5)
    x = R.int_samples(rng, 2, 2, 33)
    pay, want = R.int_bytes(x, 2), R.int_scale(x, 2)
    odd = [(b"NAME", b"abc"), (b"ANNO", b"an odd annotation"), (b"MARK", struct.pack(">H", 0)), (b"ID3 ", b"ID3\x03" + bytes(7))]
    for label, data in (
            ("comm behind ssnd", R.aiff(pay, 2, 33, 16, comm_last=True)),
            ("odd chunks everywhere", R.aiff(pay, 2, 33, 16, before=odd[:2], between=odd[2:], after=[(b"INST", bytes(20)), (b"(c) ", b"x")])),
            ("odd chunks, comm last", R.aiff(pay, 2, 33, 16, comm_last=True, before=odd, between=odd[:1])),
            ("ssnd offset 3", R.aiff(pay, 2, 33, 16, offset=3)),
            ("ssnd offset 3, aifc, comm last", R.aiff(pay, 2, 33, 16, ctype=b"twos", offset=3, comm_last=True, between=odd[:1]))):
        got = _C().load(_put(tmp_path, "l.aif", data))[0]
        assert np.array_equal(bits(got.numpy()), bits(want)), label
    # an odd number of sound bytes: the pad byte behind SSND is not a sample, and the chunk behind it is found
    x8 = R.int_samples(rng, 1, 1, 33)
    data = R.aiff(R.int_bytes(x8, 1), 1, 33, 8, comm_last=True)
    meta = _C().info(_put(tmp_path, "o.aif", data))
    assert (meta.num_frames, meta.signed8) == (33, True)
    assert np.array_equal(bits(_C().load(str(tmp_path / "o.aif"))[0].numpy()), bits(R.int_scale(x8, 1)))
    # a 12-bit sampleSize: left-justified in two bytes, decoded at the container width (as aifc does); bits_per_sample says 16
    x12 = (R.int_samples(rng, 2, 1, 20) >> 4) << 4
    meta = _C().info(_put(tmp_path, "t.aif", R.aiff(R.int_bytes(x12, 2), 1, 20, 12)))
    assert meta.bits_per_sample == 16 and meta.block_align == 2
    assert np.array_equal(bits(_C().load(str(tmp_path / "t.aif"))[0].numpy()), bits(R.int_scale(x12, 2)))
    for size, width in ((1, 1), (8, 1), (9, 2), (17, 3), (24, 3), (25, 4), (32, 4)):
        assert _C().info(_put(tmp_path, "s.aif", R.aiff(bytes(width * 4), 1, 4, size))).bits_per_sample == 8 * width
    # no frames and no SSND: an empty clip; COMM that states more frames than the file holds is cut to the whole frames there
    empty = _put(tmp_path, "e.aif", R.aiff(b"", 2, 0, 16, ssnd=False))
    assert _C().info(empty).num_frames == 0 and tuple(_C().load(empty)[0].shape) == (2, 0) and len(_C().read_payload(empty)[0]) == 0
    cut = R.aiff(pay, 2, 33, 16)[:-7]
    assert _C().info(_put(tmp_path, "c.aif", cut)).num_frames == 31
    assert np.array_equal(bits(_C().load(str(tmp_path / "c.aif"))[0].numpy()), bits(want[:, :31]))
    # G.711 in AIFF-C: one byte per sample whatever sampleSize says
    for size in (8, 16):
        data = R.aiff(bytes(12), 3, 4, size, ctype=b"ulaw", cname=b"x")
        meta = _C().info(_put(tmp_path, "u.aifc", data))
        assert (meta.block_align, meta.bits_per_sample, meta.format_tag, meta.num_frames) == (3, 8, 7, 4)


# ---- 80-bit rates -------------------------------------------------------------------------------------------------------------------
def test_extended_rates(tmp_path):
    from fractions import Fraction
    for rate in (8000, 11025, 44100, 48000, 96000, 2 ** 31 - 1, 1, 3):
        assert _C().info(_put(tmp_path, "r.aif", R.aiff(bytes(4), 1, 2, 16, rate=rate))).sample_rate == rate
    assert _C().extended_rate("x", bytes.fromhex("400EAC44000000000000")) == 44100     # (the bytes every AIFF of a CD holds)
    for rate, word in ((Fraction(244800, 11), "not an integer"), (0, "zero"), (-1, "negative"), (-44100, "negative"), (float("inf"), "infinite"),
                       (float("-inf"), "infinite"), (float("nan"), "NaN"), (2 ** 31, "int32"), (2 ** 40, "int32"), (Fraction(1, 2), "not an integer"),
                       (2.0 ** 200, "int32")):
        p = _put(tmp_path, "r.aif", R.aiff(bytes(4), 1, 2, 16, rate=rate))
        with pytest.raises(ValueError, match=word) as e:
            _C().info(p)
        assert str(e.value).startswith(p)
    with pytest.raises(ValueError, match="not an integer"):                          # a denormal
        _C().info(_put(tmp_path, "r.aif", R.aiff(bytes(4), 1, 2, 16, rate_bytes=struct.pack(">HQ", 0, 1))))


# ---- AU lengths ----------------------------------------------------------------------------------------------------------------------
def test_au_lengths(tmp_path):
    rng = np.random.default_rng(9)
    x = R.int_samples(rng, 2, 2, 40)
    pay, want = R.int_bytes(x, 2), R.int_scale(x, 2)
    for label, data, frames in (("size unknown", R.au(pay, 3, 16000, 2, size=0xFFFFFFFF), 40),
                                ("size beyond the file", R.au(pay, 3, 16000, 2, size=len(pay) + 1000), 40),
                                ("size short of the file", R.au(pay, 3, 16000, 2, size=42), 10),
                                ("a 1 KiB annotation", R.au(pay, 3, 16000, 2, annotation=b"n" * 1024), 40),
                                ("a cut last frame", R.au(pay, 3, 16000, 2, size=0xFFFFFFFF)[:-1], 39),
                                ("no data", R.au(b"", 3, 16000, 2), 0)):
        p = _put(tmp_path, "l.au", data)
        meta = _C().info(p)
        assert meta.num_frames == frames, label
        assert np.array_equal(bits(_C().load(p)[0].numpy()), bits(want[:, :frames])), label
        assert bytes(_C().read_payload(p)[0]) == pay[:frames * 4]
    assert _C().info(_put(tmp_path, "l.au", R.au(pay, 3, 16000, 2, annotation=b"n" * 1024))).data_offset == 24 + 1024


# ---- SPHERE --------------------------------------------------------------------------------------------------------------------------
def test_sphere_headers(tmp_path):
    rng = np.random.default_rng(10)
    x = R.int_samples(rng, 2, 2, 30)
    want = R.int_scale(x, 2)
    be, le = R.int_bytes(x, 2), R.int_bytes(x, 2, big=False)
    for label, data, frames in (("10", R.sphere(be, R.sphere_fields(2, 16000, 2, 30, "pcm", "10")), 30),
                                ("01", R.sphere(le, R.sphere_fields(2, 16000, 2, 30, "pcm", "01")), 30),
                                ("no sample_count", R.sphere(be, R.sphere_fields(2, 16000, 2, None, "pcm", "10")), 30),
                                ("header of 2048", R.sphere(be, R.sphere_fields(2, 16000, 2, 30, "pcm", "10"), hsize=2048), 30),
                                ("count short of the file", R.sphere(be, R.sphere_fields(2, 16000, 2, 12, "pcm", "10")), 12),
                                ("count beyond the file", R.sphere(be[:-3], R.sphere_fields(2, 16000, 2, 30, "pcm", "10")), 29),
                                ("a real rate", R.sphere(be, [("channel_count", "i", 2), ("sample_rate", "r", "16000.0"), ("sample_n_bytes", "i", 2),
                                                              ("sample_byte_format", "s", "10")]), 30)):
        p = _put(tmp_path, "s.sph", data)
        meta = _C().info(p)
        assert (meta.num_frames, meta.sample_rate, meta.container) == (frames, 16000, "sphere"), label
        assert np.array_equal(bits(_C().load(p)[0].numpy()), bits(want[:, :frames])), label
    assert _C().info(_put(tmp_path, "s.sph", R.sphere(be, R.sphere_fields(2, 16000, 2, 30, "pcm", "10"), hsize=2048))).data_offset == 2048
    codes, want8, _ = R.g711_case(rng, 2, 30, W.ULAW)
    for coding in ("ulaw", "mu-law"):
        p = _put(tmp_path, "u.sph", R.sphere(codes, R.sphere_fields(2, 8000, 1, 30, coding)))
        assert _C().info(p).format_tag == 7 and np.array_equal(bits(_C().load(p)[0].numpy()), bits(want8))
    # a TIMIT file: SPHERE under the name .WAV -- the first bytes decide
    from pix2pixhdaudiosr_amd.data import audiofile
    p = _put(tmp_path, "SA1.WAV", R.sphere(le, R.sphere_fields(2, 16000, 2, 30, "pcm", "01")))
    assert audiofile.kind(p) == "sphere" and np.array_equal(bits(audiofile.load(p)[0].numpy()), bits(want))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refused(tmp_path, data, *words):
    from pix2pixhdaudiosr_amd.data import audiofile
    p = _put(tmp_path, "bad.bin", data)
    for call in (_C().info, _C().load, _C().read_payload, audiofile.info, audiofile.load):
        with pytest.raises(ValueError) as e:
            call(p)
        assert str(e.value).startswith(p), str(e.value)
        for w in words:
            assert w in str(e.value), (w, str(e.value))


def test_aiff_refusals(tmp_path):
    names = {b"ima4": b"IMA 4:1", b"MAC3": b"MACE 3-to-1", b"MAC6": b"MACE 6-to-1", b"G722": b"CCITT G.722", b"GSM ": b"GSM 6.10",
             b"Qclp": b"Qualcomm PureVoice", b"QDMC": b"QDesign Music", b"zzzz": b"something new"}
    for ctype, cname in names.items():
        _refused(tmp_path, R.aiff(bytes(68), 2, 64, 16, ctype=ctype, cname=cname), repr(ctype.decode()), cname.decode(), "is not read")
    _refused(tmp_path, R.aiff(bytes(68), 2, 64, 16, ctype=b"ima4", cname=b"IMA 4:1"), "predictor", "no PCM twin")
    _refused(tmp_path, R.aiff(bytes(8), 1, 4, 16, ctype=b"raw ", cname=b""), "'raw '", "sampleSize of 16")
    _refused(tmp_path, R.aiff(bytes(12), 1, 4, 16, ctype=b"in24", cname=b""), "'in24'", "sampleSize of 16")
    _refused(tmp_path, R.aiff(bytes(12), 1, 4, 24, ctype=b"in32", cname=b""), "'in32'", "sampleSize of 24")
    _refused(tmp_path, R.aiff(bytes(8), 1, 4, 0), "sampleSize of 0")
    _refused(tmp_path, R.aiff(bytes(8), 1, 4, 33), "sampleSize of 33")
    _refused(tmp_path, R.aiff(bytes(8), 0, 4, 16), "1 to 65535 channels", "states 0")
    _refused(tmp_path, R.aiff(bytes(8), -2, 4, 16), "1 to 65535 channels")
    _refused(tmp_path, R.aiff(bytes(18), 9, 2, 8, ctype=b"ulaw", cname=b""), "1 to 8 channels", "states 9")
    _refused(tmp_path, R.aiff(bytes(18), 9, 2, 8, ctype=b"ALAW", cname=b""), "1 to 8 channels")
    _refused(tmp_path, R.aiff(b"", 1, 4, 16, ssnd=False), "no SSND chunk", "4 frames")
    _refused(tmp_path, b"FORM" + struct.pack(">I", 4) + b"8SVX", "neither AIFF nor AIFF-C")
    _refused(tmp_path, b"FORM" + struct.pack(">I", 4 + 16) + b"AIFF" + R.chunk(b"SSND", bytes(8)), "no COMM chunk")
    _refused(tmp_path, b"FORM" + struct.pack(">I", 4 + 12) + b"AIFF" + R.chunk(b"COMM", bytes(4)), "COMM chunk of 4 bytes")
    data = R.aiff(bytes(8), 1, 4, 16)
    at = data.index(b"SSND")
    _refused(tmp_path, data[:at + 8] + struct.pack(">I", 9) + data[at + 12:], "data offset of 9")


def test_au_refusals(tmp_path):
    for enc, word in ((23, "G.721"), (24, "G.722"), (25, "G.723"), (26, "G.723")):
        _refused(tmp_path, R.au(bytes(16), enc, 8000, 1), "AU encoding %d" % enc, word, "G.72x")
    for enc in (0, 8, 9, 10, 11, 12, 13, 17, 18, 19, 20, 21, 22, 28, 99):
        _refused(tmp_path, R.au(bytes(16), enc, 8000, 1), "AU encoding %d" % enc, "not read")
    p = _put(tmp_path, "swapped.au", R.au(bytes(16), 3, 8000, 1, magic=b"dns."))     # (audiofile sends it to wavio: not '.snd')
    for call in (_C().info, _C().load, _C().read_payload):
        with pytest.raises(ValueError, match="byte-swapped magic 'dns.'") as e:
            call(p)
        assert str(e.value).startswith(p)
    _refused(tmp_path, R.au(bytes(16), 3, 8000, 1, offset=23), "data offset of 23", "at least 24")
    _refused(tmp_path, R.au(bytes(16), 3, 8000, 1, offset=16), "data offset of 16")
    _refused(tmp_path, R.au(bytes(16), 3, 8000, 1, offset=41), "data offset of 41", "inside the file")
    _refused(tmp_path, R.au(bytes(16), 3, 0, 1), "sample rate")
    _refused(tmp_path, R.au(bytes(16), 3, 2 ** 31, 1), "sample rate")
    _refused(tmp_path, R.au(bytes(16), 3, 8000, 0), "1 to 65535 channels")
    _refused(tmp_path, R.au(bytes(16), 3, 8000, 65536), "1 to 65535 channels")
    _refused(tmp_path, R.au(bytes(18), 1, 8000, 9), "1 to 8 channels")
    _refused(tmp_path, R.au(bytes(18), 27, 8000, 9), "1 to 8 channels")
    assert _C().info(_put(tmp_path, "ok.au", R.au(bytes(65535 * 2), 3, 8000, 65535))).num_frames == 1


def test_sphere_refusals(tmp_path):
    F = R.sphere_fields
    for coding, suffix in (("pcm,embedded-shorten-v2.00", "embedded-shorten-v2.00"), ("ulaw,embedded-shorten-v2.00", "embedded-shorten-v2.00"),
                           ("pcm,embedded-wavpack-4.60", "embedded-wavpack-4.60")):
        _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 2, 8, coding, "01")), repr(suffix), "no decoder")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 2, 8, "adpcm", "01")), "'adpcm'", "is not read")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 1, 8, "pcm", "1")), "sample_n_bytes of 1")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 4, 4, "pcm", "0123")), "sample_n_bytes of 4")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 3, 4, "pcm", "012")), "sample_n_bytes of 3")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 8000, 2, 8, "ulaw", "01")), "ulaw", "sample_n_bytes of 2")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 2, 8, "pcm", None)), "sample_byte_format")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 2, 8, "pcm", "1")), "sample_byte_format", "'1'")
    _refused(tmp_path, R.sphere(bytes(16), F(0, 16000, 2, 8, "pcm", "01")), "1 to 65535 channels")
    _refused(tmp_path, R.sphere(bytes(18), F(9, 8000, 1, 2, "alaw")), "1 to 8 channels")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 16000, 2, -1, "pcm", "01")), "sample_count", "negative")
    _refused(tmp_path, R.sphere(bytes(16), F(1, 0, 2, 8, "pcm", "01")), "sample rate")
    for missing in ("channel_count", "sample_rate", "sample_n_bytes"):
        _refused(tmp_path, R.sphere(bytes(16), [f for f in F(1, 16000, 2, 8, "pcm", "01") if f[0] != missing]), "no " + missing)
    real = [("channel_count", "i", 1), ("sample_rate", "r", "11025.5"), ("sample_n_bytes", "i", 2), ("sample_byte_format", "s", "01")]
    _refused(tmp_path, R.sphere(bytes(16), real), "sample_rate", "must be an integer", "11025.5")
    _refused(tmp_path, R.sphere(bytes(16), [("channel_count", "i", "two")] + real[1:]), "channel_count", "must be an integer")
    ok = R.sphere(bytes(16), F(1, 16000, 2, 8, "pcm", "01"))
    _refused(tmp_path, ok.replace(b"end_head\n", b" " * 9), "no end_head line")
    _refused(tmp_path, ok.replace(b"   1024\n", b"   abcd\n"), "header size")
    _refused(tmp_path, ok.replace(b"   1024\n", b"      8\n"), "header size of 8")
    _refused(tmp_path, ok.replace(b"   1024\n", b"9999999\n"), "header size of 9999999")
    _refused(tmp_path, ok.replace(b"NIST_1A\n", b"NIST_2B\n"), "not a NIST SPHERE file")
    _refused(tmp_path, ok.replace(b"sample_rate -i 16000", b"sample_rate 16000   "), "key -type value")


def test_other_files_keep_wavios_refusal(tmp_path):
    from pix2pixhdaudiosr_amd.data import audiofile
    for data in (b"", b"OggS" + bytes(40), b"RIFX" + bytes(40), b"caff" + bytes(40)):
        p = _put(tmp_path, "x.bin", data)
        assert audiofile.kind(p) == "wav"
        with pytest.raises(ValueError, match="not a RIFF/WAVE file"):
            audiofile.info(p)
        with pytest.raises(ValueError, match="not an AIFF, AU or NIST SPHERE file"):
            _C().info(p)


# ---- truncation ----------------------------------------------------------------------------------------------------------------------
def _header_length(kind, data):
    if kind == "aiff":
        return R.aiff_header_length(data)
    if kind == "au":
        return struct.unpack(">I", data[4:8])[0]
    return int(data[8:16])


def _truncation_cases():
    cases = [(k.split("_")[0].replace("aifc", "aiff").replace("sunau", "au"), k, v[0]) for k, v in sorted(_golden().items())]
    rng = np.random.default_rng(4)
    for name in ("aiff-16", "aifc-sowt", "aifc-fl64", "aifc-ulaw", "au-3", "au-7", "sphere-pcm-10", "sphere-ulaw"):
        cases.append((name.split("-")[0].replace("aifc", "aiff"), name, CODINGS[name](rng, 2, 9)[0]))
    x = R.int_bytes(R.int_samples(rng, 2, 2, 9), 2)
    cases.append(("aiff", "chunks in front", R.aiff(x, 2, 9, 16, before=[(b"NAME", b"abc"), (b"ANNO", b"note")], between=[(b"MARK", bytes(2))], offset=3)))
    cases.append(("au", "annotated", R.au(x, 3, 16000, 2, annotation=b"words " * 20)))
    return cases


@pytest.mark.parametrize("kind,name,data", _truncation_cases(), ids=[c[1] for c in _truncation_cases()])
def test_every_cut_of_the_header_is_a_value_error(tmp_path, kind, name, data):
    """A file cut at any byte of its header: a ValueError that starts with the path, from info, load and read_payload alike -- no other
    exception type, and an answer every time."""
    from pix2pixhdaudiosr_amd.data import audiofile
    n = _header_length(kind, data)
    assert 12 <= n <= len(data)
    assert _C().info(_put(tmp_path, "whole.bin", data[:n])).num_frames == 0        # the whole header and not one sample: an empty clip
    p = str(tmp_path / "cut.bin")
    for cut in range(4, n):                                                        # (below 4 bytes nothing says which container it is)
        with open(p, "wb") as f:
            f.write(data[:cut])
        for call in (_C().info, _C().load, _C().read_payload, audiofile.load):
            with pytest.raises(ValueError) as e:
                call(p)
            assert str(e.value).startswith(p), (cut, str(e.value))
    for cut in range(0, 4):
        with open(p, "wb") as f:
            f.write(data[:cut])
        with pytest.raises(ValueError):
            _C().info(p)
        with pytest.raises(ValueError):
            audiofile.info(p)


# ---- dispatch, datasets, folder planning ---------------------------------------------------------------------------------------------
def test_audiofile_kind_on_all_five(tmp_path):
    from pix2pixhdaudiosr_amd.data import audiofile
    rng = np.random.default_rng(2)
    x = W.speech_like(1, 40, 1)
    W.write_pcm16_wav(str(tmp_path / "a.wav"), x, 16000)
    assert audiofile.kind(str(tmp_path / "a.wav")) == "wav"
    for data, want in ((b"fLaC" + bytes(40), "flac"), (b"ID3\x03" + bytes(40), "flac"), (CODINGS["aiff-16"](rng, 1, 4)[0], "aiff"),
                       (CODINGS["aifc-sowt"](rng, 1, 4)[0], "aiff"), (CODINGS["au-3"](rng, 1, 4)[0], "au"), (CODINGS["sphere-pcm-01"](rng, 1, 4)[0], "sphere"),
                       (b"RIFF" + bytes(40), "wav"), (b"", "wav"), (b"dns." + bytes(40), "wav")):
        assert audiofile.kind(_put(tmp_path, "k.wav", data)) == want              # (the name says nothing)
    from pix2pixhdaudiosr_amd.data import wavio
    assert type(audiofile.info(str(tmp_path / "a.wav"))) is wavio.WavInfo
    assert type(audiofile.info(_put(tmp_path, "k.wav", CODINGS["au-3"](rng, 1, 4)[0]))) is _C().AudioInfo


def _opt(root, **more):
    return SimpleNamespace(lr_sampling_rate=8000, hr_sampling_rate=16000, segment_length=100, n_fft=64, hop_length=32, win_length=64,
                           center=True, dataroot=str(root), seed=3, **more)


def test_dataset_reads_container_twins(tmp_path, capsys):
    import torch
    from pix2pixhdaudiosr_amd.data.audio_dataset import AudioDataset
    wav, mixed = tmp_path / "wav", tmp_path / "mixed"
    for d in (wav / "sub", mixed / "sub"):
        d.mkdir(parents=True)
    makers = {"a.aif": lambda x: R.aiff(R.int_bytes(x, 2), 2, x.shape[1], 16),
              "b.sph": lambda x: R.sphere(R.int_bytes(x, 2, big=False), R.sphere_fields(2, 16000, 2, x.shape[1], "pcm", "01")),
              "sub/c.AIFC": lambda x: R.aiff(R.int_bytes(x, 2, big=False), 2, x.shape[1], 16, ctype=b"sowt", cname=b""),
              "short.sph": lambda x: R.sphere(R.int_bytes(x, 2), R.sphere_fields(2, 16000, 2, None, "pcm", "10"))}
    for i, (name, make) in enumerate(makers.items()):
        x = W.speech_like(2, 30 if name.startswith("short") else 400 + 37 * i, i)
        _put(mixed, name, make(x))
        W.write_pcm16_wav(str(wav / (os.path.splitext(name)[0] + ".wav")), x, 16000)
    _put(mixed, "d.au", R.au(bytes(80), 3, 16000, 2))                              # (not asked for below: not listed)
    assert len(AudioDataset(_opt(mixed))) == 0                                     # the default scan lists .wav alone
    assert len(AudioDataset(_opt(mixed, audio_formats="wav,aif"))) == 1
    dw, dm = AudioDataset(_opt(wav)), AudioDataset(_opt(mixed, audio_formats="wav,aif,aifc,sph"))
    assert len(dw) == len(dm) == 4
    stem = lambda p: os.path.splitext(os.path.relpath(p, str(tmp_path)).split(os.sep, 1)[1])[0]
    where = {stem(p): i for i, p in enumerate(dm.audio_file)}
    capsys.readouterr()
    for i, p in enumerate(dw.audio_file):
        torch.manual_seed(11 + i)
        a = dw[i]
        torch.manual_seed(11 + i)
        b = dm[where[stem(p)]]
        assert torch.equal(a["raw"].view(torch.int32), b["raw"].view(torch.int32)) and (a["raw_len"], a["rate"]) == (b["raw_len"], b["rate"])
    assert "Load failed!" not in capsys.readouterr().out
    assert len(AudioDataset(_opt(mixed, audio_formats="au,snd"))) == 1
    with pytest.raises(ValueError, match="audio_formats"):
        AudioDataset(_opt(mixed, audio_formats="wav,aif,mp3"))


def test_plan_folder_with_the_new_extensions(tmp_path):
    from pix2pixhdaudiosr_amd.generate import INPUT_FORMATS, check_input_formats, plan_folder
    src, dst = tmp_path / "in", tmp_path / "out"
    for rel in ("b.wav", "a.AIF", "c.aiff", "d.aifc", "e.au", "f.snd", "sub/g.sph", "sub/y.wav", "h.flac", "notes.txt", "aif", "i.mp3"):
        p = src / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    j = os.path.join
    assert INPUT_FORMATS == ("wav", "flac", "aif", "aiff", "aifc", "au", "snd", "sph")
    assert [r for r, _, _ in plan_folder(str(src), str(dst))] == ["b.wav", j("sub", "y.wav")]           # a default scan: .wav alone, as before
    plan = plan_folder(str(src), str(dst), formats="wav,aif,aiff,aifc,au,snd,sph")
    assert [(r, os.path.relpath(o, str(dst))) for r, _, o in plan] == [
        ("a.AIF", "a.wav"), ("b.wav", "b.wav"), ("c.aiff", "c.wav"), ("d.aifc", "d.wav"), ("e.au", "e.wav"), ("f.snd", "f.wav"),
        (j("sub", "g.sph"), j("sub", "g.wav")), (j("sub", "y.wav"), j("sub", "y.wav"))]
    plan = plan_folder(str(src), str(dst), formats=("aif", "sph"), ext=".flac")
    assert [(r, os.path.relpath(o, str(dst))) for r, _, o in plan] == [("a.AIF", "a.flac"), (j("sub", "g.sph"), j("sub", "g.flac"))]
    for twin, formats in (("a.wav", "wav,aif"), ("e.snd", "au,snd"), ("sub/g.aiff", "sph,aiff")):
        (src / twin).write_bytes(b"")
        with pytest.raises(ValueError, match="both be written"):
            plan_folder(str(src), str(dst), formats=formats)
        os.remove(str(src / twin))
    assert check_input_formats("wav, .AIF,sph") == ("wav", "aif", "sph")
    for bad in ("mp3", "wav,mp3", "aif,ogg", "", ("aif", 3), ()):
        with pytest.raises(ValueError):
            check_input_formats(bad)
