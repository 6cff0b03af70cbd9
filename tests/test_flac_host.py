"""The FLAC reader on the host (csrc/flac.hip: p2phd_flac_info / p2phd_flac_index / p2phd_flac_decode_host; data/flacio.py,
data/audiofile.py) against the restatement tests/_flac_ref.py, bit for bit, and the places it is wired into: the feeder's datasets,
plan_folder and the command line.  No GPU."""
import os
import struct
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _flac_cases as K
import _flac_ref as R

CASES = K.all_cases()


def _flacio():
    from pix2pixhdaudiosr_amd.data import flacio
    return flacio


def _decode(data, name="case"):
    f = _flacio()
    meta, table = f.index_bytes(data, name)
    return meta, table, f.decode_frames(data, table, 0, len(table), meta.num_channels, name)


def test_restatement():
    """The restatement's own anchors: the two CRCs, the RFC's example frame, encode -> decode identity."""
    R.self_check()
    for name in ("matrix-2ch-16bit", "wide-sums", "rice-edges", "escapes-12bit", "wasted-20bit", "stereo-24bit-10", "variable-small", "metadata-id3"):
        data, chs = CASES[name]()
        info, out = R.decode_stream(data)
        assert out == chs, name
        assert info["md5"] == R.md5_of(chs, info["bits"])


def test_rfc_frame():
    data = R.encode_stream([R.RFC_FRAME], 44100, 2, 16, 1, 16, 16)
    meta, table, pcm = _decode(data)
    assert (meta.sample_rate, meta.num_frames, meta.num_channels, meta.bits_per_sample, meta.num_flac_frames) == (44100, 1, 2, 16, 1)
    assert table.tolist() == [[42, len(R.RFC_FRAME), 0, 1, 1, 16]]
    assert pcm.tolist() == [[25588], [10416]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_decoder_bit_for_bit(name):
    data, chs = CASES[name]()
    meta, table, pcm = _decode(data, name)
    assert meta.num_channels == len(chs) and meta.num_frames == len(chs[0])
    assert np.array_equal(pcm, np.array(chs, dtype=np.int64))
    # frames chain from the first frame to the end of the file; the columns are consecutive
    assert table[0, 0] == meta.first_frame_offset and table[-1, 0] + table[-1, 1] == len(data)
    assert np.array_equal(table[1:, 0], table[:-1, 0] + table[:-1, 1])
    assert np.array_equal(table[1:, 2], table[:-1, 2] + table[:-1, 3])


def test_info_fields():
    data, chs = CASES["metadata-id3-footer"]()
    meta, table, _ = _decode(data)
    assert meta[:4] == (44100, 70, 2, 16)                                      # WavInfo's leading fields
    assert meta.seek_points == 3 and meta.md5 == R.md5_of(chs, 16) and (meta.min_block, meta.max_block) == (32, 32)
    assert data[meta.first_frame_offset:meta.first_frame_offset + 2] == b"\xff\xf8"
    data, chs = CASES["block-codes"]()
    meta, table, _ = _decode(data)
    assert table[:, 3].tolist() == K.BLOCK_SIZES
    for (rate, code) in K.RATES:
        assert _decode(CASES["rate-%d-%s" % (rate, code)]()[0])[0].sample_rate == rate
    for variable, first in K.NUMBERS:
        t = _decode(CASES["number-%s-%d" % ("v" if variable else "f", first)]()[0])[1]
        assert t[0, 2] == (first if variable else first * 16)


def test_total_zero_is_counted():
    ch = K.signal(40, 16, 1)
    data, _ = R.make_stream([ch], 16, 16, total=0)
    meta, _, pcm = _decode(data)
    assert meta.num_frames == 40 and pcm[0].tolist() == ch


def test_partial_decode_and_bounds():
    """Frames of a window alone; a table row that points outside the bytes, or a column outside the rows, is refused."""
    f = _flacio()
    data, chs = CASES["matrix-2ch-16bit"]()
    meta, table = f.index_bytes(data)
    pcm = f.decode_frames(data, table, 3, 4, 2)
    assert np.array_equal(pcm, np.array(chs)[:, 3 * 48:7 * 48])
    bad = table.copy()
    bad[5, 1] += len(data)
    with pytest.raises(ValueError, match="frame 5"):
        f.decode_frames(data, bad, 0, len(bad), 2)
    bad = table.copy()
    bad[5, 1] -= 3                                                             # the bits run out inside the row's range: an error, not an overrun
    with pytest.raises(ValueError, match="frame 5"):
        f.decode_frames(data, bad, 0, len(bad), 2)


def _small():
    ch = K.signal(5 * 16, 16, 77)
    return R.make_stream([ch], 16, 16, specs=[dict(kind="fixed", order=2)])


def test_false_header_does_not_split_a_frame():
    """The header of the frame that follows, CRC-8 and number right, planted in a VERBATIM frame's samples."""
    ch = K.signal(4 * 16, 16, 3)
    for k in range(3):
        fake = R.frame_header(16, 44100, 0, 16, k + 1)
        fake += b"\0" * (len(fake) % 2)
        for i in range(len(fake) // 2):
            ch[16 * k + 4 + i] = struct.unpack(">h", fake[2 * i:2 * i + 2])[0]
    data, frames = R.make_stream([ch], 16, 16)
    assert all(R.frame_header(16, 44100, 0, 16, k + 1) in frames[k][9:] for k in range(3))
    meta, table, pcm = _decode(data)
    assert table[:, 1].tolist() == [len(f) for f in frames] and pcm[0].tolist() == ch


def test_closed_crc_in_front_of_a_sync_code_inside_a_frame():
    """Valid and rare (once in 2^27 bytes of audio): inside a VERBATIM frame sample 5 is the CRC-16 of the frame's bytes in front of
    it, so the running CRC closes behind it, and sample 6 is 0xFFF8, a sync code.  The frame does not end there: its subframe does
    not decode to that bit.  Also with the sync code one bit off."""
    for fake in (0xFFF8, 0xFFF9, 0xFFFA, 0xFFF0, 0x7FF8):
        ch = K.signal(32, 16, 6)
        ch[6] = fake - 0x10000 if fake & 0x8000 else fake
        frame = R.encode_frame([ch[:16]], 16, 0)
        at = len(R.frame_header(16, 44100, 0, 16, 0)) + 1                      # sample 0: behind the header and the subframe's byte
        crc = R.crc16(frame[:at + 10])
        ch[5] = crc - 0x10000 if crc & 0x8000 else crc
        data, frames = R.make_stream([ch], 16, 16)
        assert R.crc16(frames[0][:at + 12]) == 0 and frames[0][at + 12:at + 14] == fake.to_bytes(2, "big")
        assert R.decode_stream(data)[1] == [ch]
        meta, table, pcm = _decode(data)
        assert table[:, 1].tolist() == [len(f) for f in frames] and pcm[0].tolist() == ch


def test_decode_frames_refuses_another_channel_count():
    f = _flacio()
    data, chs = CASES["matrix-2ch-16bit"]()
    meta, table = f.index_bytes(data)
    with pytest.raises(ValueError, match="frame 0.*assignment 1 is not one of 1 channels"):
        f.decode_frames(data, table, 0, len(table), 1)
    bad = table.copy()
    bad[4, 4] = 2                                                              # a row that claims three channels: nothing is written past the two rows
    with pytest.raises(ValueError, match="frame 4.*assignment 2 is not one of 2 channels"):
        f.decode_frames(data, bad, 0, len(bad), 2)


def test_flipped_bit_names_its_frame():
    data, frames = _small()
    f = _flacio()
    at = len(data) - sum(len(x) for x in frames)
    for k, frame in enumerate(frames):
        for bit in range(8 * len(frame)):
            bad = bytearray(data)
            bad[at + bit // 8] ^= 0x80 >> (bit % 8)
            with pytest.raises(ValueError, match=r"case: flac_index: frame %d at byte %d:" % (k, at)):
                f.index_bytes(bytes(bad), "case")
        at += len(frame)


def _refused(data, match):
    with pytest.raises(ValueError, match=match):
        _decode(data, "named.flac")


def test_index_refusals():
    data, frames = _small()
    head = data[:len(data) - sum(len(x) for x in frames)]
    _refused(data[:-5], r"named.flac.*frame 4 at byte \d+")                    # truncated inside the last frame
    _refused(data[:-len(frames[-1])], "named.flac.*truncated")                 # ... and at a frame boundary
    _refused(head + b"".join(frames[:2] + frames[3:]), "named.flac.*frame 2 at byte.*gap")
    _refused(data + b"\0" * 7, "named.flac.*frame 4")                          # bytes behind the last frame
    ch = K.signal(32, 16, 2)

    def second(**header):                                                      # a stream whose second frame has this header
        a = R.encode_frame([ch[:16]], 16, 0)
        b = R.encode_frame([ch[16:]], 16, 1, **header)
        return R.encode_stream([a, b], 44100, 1, 16, 32, 16, 16)
    _refused(second(bs_code=0), "frame 1 at byte.*reserved block-size code")
    _refused(second(rate_code=15), "frame 1 at byte.*reserved sample-rate code")
    _refused(second(bits_code=3), "frame 1 at byte.*reserved sample-size code")
    _refused(second(bits_code=7), "frame 1 at byte.*32-bit")
    _refused(second(reserved1=1), "frame 1 at byte.*reserved bit")
    _refused(second(reserved2=1), "frame 1 at byte.*reserved bit")
    _refused(second(rate=48000), "frame 1 at byte.*sample rate changes")
    _refused(second(bits_code=5), "frame 1 at byte.*sample size changes")
    for assign in range(11, 16):
        a = R.encode_frame([ch[:16]], 16, 0)
        b = R.frame_header(16, 44100, assign, 16, 1) + bytes(35)
        _refused(R.encode_stream([a, b + struct.pack(">H", R.crc16(b))], 44100, 1, 16, 32, 16, 16), "frame 1 at byte.*reserved channel assignment")
    a = R.encode_frame([ch[:16]], 16, 0)
    b = R.encode_frame([ch[16:], ch[16:]], 16, 1)
    _refused(R.encode_stream([a, b], 44100, 1, 16, 32, 16, 16), "frame 1 at byte.*channel count changes")
    _refused(R.encode_stream([a], 44100, 1, 32, 16, 16, 16), "named.flac.*32-bit")
    _refused(b"OggS" + data, "named.flac.*Ogg")
    _refused(R.encode_stream([a], 44100, 1, 16, 16, 16, 16, marker=b"RIFF"), "named.flac.*not a FLAC stream")
    _refused(data[:30], "named.flac.*ends inside the metadata")


@pytest.mark.parametrize("spec,why", [(dict(type_bits=2), "reserved"), (dict(type_bits=13), "reserved"), (dict(type_bits=16), "reserved"),
                                      (dict(pad_bit=1), "reserved"), (dict(method_field=2), "reserved"), (dict(method_field=3), "reserved"),
                                      (dict(kind="lpc", coefs=[3, -1], precision=4, shift=-1), "reserved"),
                                      (dict(kind="lpc", coefs=[3, -1], precision=16), "reserved")])
def test_subframe_refusals(spec, why):
    """Reserved subframe types, the padding bit, reserved residual methods, a negative LPC shift, the reserved precision: frames the
    index passes (their CRCs are right) and the decoder refuses by number."""
    ch = K.signal(32, 16, 4)
    base = dict(kind="fixed", order=2)
    base.update(spec)
    if base.get("precision") == 16:
        w = dict(base, precision=15)
        good = R.encode_frame([ch[16:]], 16, 1, specs=[w])
        # the precision field is the 4 bits behind the subframe header (8 bits) and the two 16-bit warm-up samples
        body = bytearray(good[:-2])
        hdr = len(R.frame_header(16, 44100, 0, 16, 1))
        assert body[hdr + 5] >> 4 == 14
        body[hdr + 5] |= 0xF0
        frame = bytes(body) + struct.pack(">H", R.crc16(body))
    else:
        frame = R.encode_frame([ch[16:]], 16, 1, specs=[base])
    data = R.encode_stream([R.encode_frame([ch[:16]], 16, 0), frame], 44100, 1, 16, 32, 16, 16)
    f = _flacio()
    meta, table = f.index_bytes(data, "named.flac")
    with pytest.raises(ValueError, match="named.flac.*frame 1 at byte.*" + why):
        f.decode_frames(data, table, 0, 2, 1, "named.flac")


def _write_wav(path, chs, bits, rate=44100):
    a = np.array(chs, dtype=np.int64).T
    if bits == 8:
        payload = (a + 128).astype(np.uint8).tobytes()
    elif bits == 16:
        payload = a.astype("<i2").tobytes()
    else:
        payload = np.ascontiguousarray(a.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()
    align = len(chs) * bits // 8
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, len(chs), rate, rate * align, align, bits))
        f.write(b"data" + struct.pack("<I", len(payload)) + payload)


@pytest.mark.parametrize("bits", [8, 16, 24])
def test_load_equals_wavio_load(tmp_path, bits):
    from pix2pixhdaudiosr_amd.data import audiofile, wavio
    f = _flacio()
    data, chs = CASES["matrix-2ch-%dbit" % bits]()
    pf, pw = str(tmp_path / "x.flac"), str(tmp_path / "x.wav")
    open(pf, "wb").write(data)
    _write_wav(pw, chs, bits)
    builds = f.STATS["index_builds"]
    T = len(chs[0])
    assert f.info(pf)[:4] == wavio.info(pw)[:4] == audiofile.info(pf)[:4]
    windows = [(0, -1), (0, 0), (T, 5), (T + 9, -1)]
    windows += [(a, b - a) for a in (0, 47, 48, 49, 95, 96, 97) for b in (a + 1, 143, 144, 145, T - 1, T, T + 7) if b > a]
    for off, n in windows:
        a, ra = f.load(pf, off, n)
        b, rb = wavio.load(pw, off, n)
        assert ra == rb == 44100 and a.dtype == b.dtype == torch.float32 and a.shape == b.shape, (off, n)
        assert torch.equal(a, b), (off, n)
    assert torch.equal(audiofile.load(pf, 5, 60)[0], wavio.load(pw, 5, 60)[0]) and torch.equal(audiofile.load(pw)[0], wavio.load(pw)[0])
    assert f.STATS["index_builds"] == builds + 1 and f.STATS["index_hits"] >= len(windows)      # one index, re-used by every call
    os.utime(pf, ns=(1, 1))                                                                      # another mtime: another key
    f.load(pf, 0, 1)
    assert f.STATS["index_builds"] == builds + 2


def test_load_reads_covering_frames_only(tmp_path, monkeypatch):
    f = _flacio()
    data, chs = CASES["matrix-1ch-16bit"]()
    p = str(tmp_path / "x.flac")
    open(p, "wb").write(data)
    meta, table = f.index_bytes(data)
    f.info(p)
    seen = []
    real = f.decode_frames
    monkeypatch.setattr(f, "decode_frames", lambda buf, t, first, count, ch, name="": seen.append((len(buf), count)) or real(buf, t, first, count, ch, name))
    f.load(p, 50, 48)                                                          # samples 50 .. 97: frames 1 and 2 of 48
    assert seen == [(int(table[1, 1] + table[2, 1]), 2)]


def test_read_file_into(tmp_path):
    f = _flacio()
    data, chs = CASES["stereo-16bit-10"]()
    p = str(tmp_path / "x.flac")
    open(p, "wb").write(data)
    got, meta, table = f.read_file(p)
    assert bytes(got) == data and meta.num_frames == len(chs[0]) and len(table) == meta.num_flac_frames
    buf = np.zeros(len(data) + 100, dtype=np.uint8)
    asked = []
    got, _, _ = f.read_file(p, into=lambda n: asked.append(n) or buf)
    assert asked == [len(data)] and bytes(buf[:len(data)]) == data and len(got) == len(data)
    with pytest.raises(ValueError, match="buffer"):
        f.read_file(p, into=bytearray(10))


def test_verify(tmp_path):
    f = _flacio()
    data, chs = CASES["matrix-3ch-24bit"]()
    p = str(tmp_path / "x.flac")
    open(p, "wb").write(data)
    assert f.verify(p) is True
    md5 = R.md5_of(chs, 24)
    at = data.index(md5)
    open(p, "wb").write(data[:at] + bytes([md5[0] ^ 1]) + data[at + 1:])
    assert f.verify(p) is False
    open(p, "wb").write(data[:at] + bytes(16) + data[at + 16:])
    assert f.verify(p) is None
    for bits in (8, 12, 20):
        open(p, "wb").write(CASES["matrix-2ch-%dbit" % bits]()[0])
        assert f.verify(p) is True


def _opt(root, **more):
    return SimpleNamespace(lr_sampling_rate=8000, hr_sampling_rate=16000, segment_length=100, n_fft=64, hop_length=32, win_length=64,
                           center=True, dataroot=str(root), seed=3, **more)


def test_dataset_reads_flac_twins(tmp_path, capsys):
    from pix2pixhdaudiosr_amd.data.audio_dataset import AudioDataset
    wav, flac = tmp_path / "wav", tmp_path / "flac"
    for d in (wav, flac / "sub"):
        d.mkdir(parents=True)
    (wav / "sub").mkdir()
    for i, name in enumerate(("a", "b", "sub/c")):
        chs = [K.signal(400 + 37 * i, 16, i), K.signal(400 + 37 * i, 16, i + 9)]
        data, _ = R.make_stream(chs, 16, 64, rate=16000, assign=R.MID_SIDE, specs=[dict(kind="fixed", order=2), dict(kind="fixed", order=1)])
        open(str(flac / (name + ".flac")), "wb").write(data)
        _write_wav(str(wav / (name + ".wav")), chs, 16, 16000)
    short = [K.signal(30, 16, 5)]
    open(str(flac / "short.flac"), "wb").write(R.make_stream(short, 16, 16, rate=16000)[0])
    _write_wav(str(wav / "short.wav"), short, 16, 16000)
    assert len(AudioDataset(_opt(flac))) == 0                                  # the default scan lists no .flac
    assert len(AudioDataset(_opt(flac, audio_formats="wav"))) == 0
    dw, df = AudioDataset(_opt(wav)), AudioDataset(_opt(flac, audio_formats="wav,flac"))
    assert len(dw) == len(df) == 4
    stem = lambda p: os.path.splitext(os.path.relpath(p, str(tmp_path)).split(os.sep, 1)[1])[0]
    where = {stem(p): i for i, p in enumerate(df.audio_file)}
    for i, p in enumerate(dw.audio_file):
        torch.manual_seed(11 + i)
        a = dw[i]
        torch.manual_seed(11 + i)
        b = df[where[stem(p)]]
        assert torch.equal(a["raw"], b["raw"]) and (a["raw_len"], a["rate"]) == (b["raw_len"], b["rate"])
    with pytest.raises(ValueError, match="audio_formats"):
        AudioDataset(_opt(flac, audio_formats="wav,mp3"))
    # a csv list is taken as it stands: a listed FLAC loads
    (tmp_path / "list.csv").write_text("flac/a.flac,wav/b.wav\n")
    dc = AudioDataset(_opt(tmp_path / "list.csv"))
    capsys.readouterr()
    torch.manual_seed(11)
    a = dc[0]
    torch.manual_seed(11)
    assert torch.equal(a["raw"], dw[[stem(p) for p in dw.audio_file].index("a")]["raw"])
    assert "Load failed!" not in capsys.readouterr().out


def test_plan_folder_formats(tmp_path):
    from pix2pixhdaudiosr_amd.generate import check_input_formats, plan_folder
    src, dst = tmp_path / "in", tmp_path / "out"
    for rel in ("b.wav", "a.FLAC", "sub/x.flac", "sub/y.wav", "notes.txt", "flac"):
        p = src / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    j = os.path.join
    assert [r for r, _, _ in plan_folder(str(src), str(dst))] == ["b.wav", j("sub", "y.wav")]
    assert plan_folder(str(src), str(dst), formats=("wav",)) == plan_folder(str(src), str(dst))
    plan = plan_folder(str(src), str(dst), formats=("wav", "flac"))
    assert [(r, os.path.relpath(o, str(dst))) for r, _, o in plan] == [("a.FLAC", "a.wav"), ("b.wav", "b.wav"), (j("sub", "x.flac"), j("sub", "x.wav")),
                                                                       (j("sub", "y.wav"), j("sub", "y.wav"))]
    assert [r for r, _, _ in plan_folder(str(src), str(dst), formats="flac")] == ["a.FLAC", j("sub", "x.flac")]
    (src / "sub" / "x.wav").write_bytes(b"")
    with pytest.raises(ValueError, match="both be written"):
        plan_folder(str(src), str(dst), formats=("wav", "flac"))
    assert len(plan_folder(str(src), str(dst))) == 3                           # the default does not see the collision
    assert check_input_formats("wav, .FLAC") == ("wav", "flac")
    for bad in ("mp3", "", ("wav", 3), ()):
        with pytest.raises(ValueError):
            check_input_formats(bad)


def test_command_line_flags():
    from pix2pixhdaudiosr_amd.generate import _parser
    base = ["--input", "in", "--output", "out", "--load_pretrain", "ckpt"]
    a = _parser().parse_args(base)
    assert a.input_formats is None and a.verify_input is False
    a = _parser().parse_args(base + ["--input_formats", "wav,flac", "--verify_input"])
    assert a.input_formats == "wav,flac" and a.verify_input is True
    for old in (["--channels", "all", "--encoding", "pcm24"], ["--dither", "shaped", "--dither_curve", "e5", "--dither_chunk", "512"],
                ["--output_rate", "44100", "--clip", "guard", "--ceiling_dbfs", "-1", "--true_peak", "--limiter"],
                ["--loudness", "-23", "--loudness_scope", "folder", "--norm_scope", "clip", "--stereo", "ms"],
                ["--crossover", "input", "--crossover_hz", "auto", "--bandwidth", "--stereo_report", "--metrics_ext", "--fp16"]):
        _parser().parse_args(base + old)
