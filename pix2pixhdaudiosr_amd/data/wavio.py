"""RIFF/WAVE reader for the feeder (stands in for torchaudio.info / torchaudio.load of data/audio_dataset.py:31-38,99):
header parse + a seek to the requested frame window, so a random training segment costs one read of segment_length
frames, not the file.  PCM 8/16/24/32-bit and IEEE float, WAVE_FORMAT_EXTENSIBLE included; samples are scaled the way
`torchaudio.load(normalize=True)` documents (signed PCM / 2^(bits-1)).  Host I/O only -- no arithmetic of the hot path.

Coded data chunks -- G.711 mu-law (tag 7), A-law (tag 6) and 4-bit IMA ADPCM (tag 0x11), the formats of telephone archives -- are
decoded by the library's host entries (csrc/wavcodec.hip, plain C++) to exactly the samples the file's PCM16 twin holds, scaled as 16-bit
PCM is; a window of an IMA file costs one read of the blocks that cover it.  MS ADPCM (tag 2), GSM 6.10, G.726 and MP3-in-WAV stay
refused: no second decoder stands beside them to hold this one against."""
import os
import struct
from collections import namedtuple

import numpy as np
import torch

WavInfo = namedtuple("WavInfo", "sample_rate num_frames num_channels bits_per_sample format_tag data_offset block_align")


# Coded data chunks (include/p2phd.h, "Coded WAV input"): format tag -> (name, bits per sample).  Decoded by csrc/wavcodec.hip to the
# samples of the file's PCM16 twin: on the host here (`load`), on the device in whole-file generation (generate.g711_decode / ima_decode).
CODED_TAGS = {6: ("A-law", 8), 7: ("mu-law", 8), 0x11: ("IMA ADPCM", 4)}
CODED_MAX_CHANNELS = 8


def ima_samples_per_block(channels, block_align):
    """Samples per block and channel of IMA ADPCM in WAV, 1 + 8 * (block_align - 4C) / 4C; None for a block_align the layout does not
    admit (below 8C, or not a whole number of 4C-byte groups behind the C headers)."""
    c4 = 4 * int(channels)
    if channels < 1 or block_align < 2 * c4 or (block_align - c4) % c4:
        return None
    return 1 + 8 * ((block_align - c4) // c4)


def coded_frames(tag, channels, block_align, nbytes):
    """The frames `nbytes` of a coded data chunk hold: G.711 one per `channels` bytes; IMA spb per whole block, plus 1 + 8k for a
    trailing partial block that holds its headers and k >= 0 whole groups (anything shorter is ignored)."""
    if tag != 0x11:
        return nbytes // channels
    spb, c4 = ima_samples_per_block(channels, block_align), 4 * channels
    full, rest = divmod(nbytes, block_align)
    return full * spb + (1 + 8 * (rest // c4 - 1) if rest >= c4 else 0)


def _coded_info(path, tag, ch, rate, align, bits, fmt, extensible, fact, offset, there):
    name, want = CODED_TAGS[tag]
    if bits != want:
        raise ValueError(f"{path}: {name} (tag {tag}) holds {want} bits per sample, the fmt chunk states {bits}")
    if not 1 <= ch <= CODED_MAX_CHANNELS:
        raise ValueError(f"{path}: {name} (tag {tag}) is read with 1 to {CODED_MAX_CHANNELS} channels, the fmt chunk states {ch}")
    if tag == 0x11:
        spb = ima_samples_per_block(ch, align)
        if spb is None:
            raise ValueError(f"{path}: IMA ADPCM needs a block_align of 4 * channels * (1 + groups) with groups >= 1, "
                             f"the fmt chunk states {align} for {ch} ch")
        if len(fmt) >= 20 and struct.unpack("<H", fmt[16:18])[0] >= 2:
            stated = struct.unpack("<H", fmt[18:20])[0]
            if stated != spb and not (extensible and stated == 0):
                raise ValueError(f"{path}: the fmt chunk states {stated} samples per block, a block_align of {align} with {ch} ch holds {spb}")
    elif align != ch:
        raise ValueError(f"{path}: {name} (tag {tag}) needs a block_align of one byte per channel, the fmt chunk states {align} for {ch} ch")
    frames = coded_frames(tag, ch, align, there)
    if fact is not None:
        frames = min(frames, fact)                                          # a fact chunk that claims more is cut to what is there
    return WavInfo(rate, frames, ch, bits, tag, offset, align)


def _parse(path):
    """-> (WavInfo, the bytes of the data chunk that are in the file)."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file")
        fmt = fact = None
        while True:
            hdr = f.read(8)
            if len(hdr) < 8:
                raise ValueError(f"{path}: no data chunk")
            cid, size = hdr[:4], struct.unpack("<I", hdr[4:])[0]
            if cid == b"fmt ":
                fmt = f.read(size)
                if size & 1:
                    f.seek(1, 1)
            elif cid == b"fact" and size >= 4:
                word = f.read(4)                                          # dwSampleLength: frames per channel (coded formats)
                fact = struct.unpack("<I", word)[0] if len(word) == 4 else None
                f.seek(size - 4 + (size & 1), 1)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: data chunk before fmt chunk")
                tag, ch, rate, _, align, bits = struct.unpack("<HHIIHH", fmt[:16])
                extensible = tag == 0xFFFE and len(fmt) >= 26
                if extensible:
                    tag = struct.unpack("<H", fmt[24:26])[0]
                there = min(size, max(os.fstat(f.fileno()).st_size - f.tell(), 0))
                if tag in CODED_TAGS:
                    return _coded_info(path, tag, ch, rate, align, bits, fmt, extensible, fact, f.tell(), there), there
                if tag not in (1, 3) or bits not in (8, 16, 24, 32, 64) or ch < 1 or align != ch * bits // 8:
                    raise ValueError(f"{path}: unsupported WAVE format (tag {tag}, {bits} bit, {ch} ch)")
                return WavInfo(rate, size // align, ch, bits, tag, f.tell(), align), there
            else:
                f.seek(size + (size & 1), 1)


def info(path):
    """-> WavInfo.  PCM and IEEE float: num_frames as the data chunk states them.  A coded file (CODED_TAGS): bits_per_sample 8 or 4,
    the file's own block_align, num_frames the decoded frame count -- the `fact` chunk's where there is one, cut to what the data
    chunk holds."""
    return _parse(path)[0]


def _lib():
    from .. import _lib as L
    return L.lib()


def _load_coded(path, meta, there, start, stop):
    """Frames [start, stop) of a coded data chunk, decoded on the host (p2phd_g711_decode_host / p2phd_ima_decode_host: plain C++, no
    device): one seek and one read of the bytes -- for IMA the blocks -- that cover the window."""
    import ctypes
    C, n = meta.num_channels, stop - start
    out = np.zeros((C, n), dtype=np.float32)
    if n == 0:
        return out
    lib = _lib()
    if meta.format_tag == 0x11:
        spb = ima_samples_per_block(C, meta.block_align)
        b0, b1 = start // spb, -(-stop // spb)
        byte0, byte1 = b0 * meta.block_align, min(b1 * meta.block_align, there)
    else:
        b0, byte0, byte1 = 0, start * C, stop * C
    with open(path, "rb") as f:
        f.seek(meta.data_offset + byte0)
        raw = np.frombuffer(f.read(byte1 - byte0), dtype=np.uint8)
    if raw.size != byte1 - byte0:
        raise ValueError(f"{path}: short read of the data chunk")
    src, dst = ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    if meta.format_tag == 0x11:
        bad = lib.p2phd_ima_scan_host(src, raw.size, C, meta.block_align)
        if bad >= 0:
            raise ValueError(f"{path}: block {b0 + bad}: a step index above 88 in its header")
        rc = -1 if bad != -1 else lib.p2phd_ima_decode_host(src, raw.size, C, meta.block_align, start - b0 * spb, n, dst, n)
    else:
        rc = lib.p2phd_g711_decode_host(src, n, C, 1 if meta.format_tag == 6 else 0, dst, n)
    if rc != 0:
        raise ValueError("%s: %s" % (path, lib.p2phd_last_error().decode("utf-8", "replace")))
    return out


def ima_scan(payload, channels, block_align, name="<bytes>"):
    """The block headers of an IMA ADPCM payload (a bytes-like object), checked on the host (p2phd_ima_scan_host): a step index above
    88 is a ValueError that names `name` and the block."""
    import ctypes
    a = np.frombuffer(payload, dtype=np.uint8)
    lib = _lib()
    bad = lib.p2phd_ima_scan_host(ctypes.c_void_p(a.ctypes.data if a.size else None), a.size, int(channels), int(block_align))
    if bad >= 0:
        raise ValueError(f"{name}: block {bad}: a step index above 88 in its header")
    if bad != -1:
        raise ValueError("%s: %s" % (name, lib.p2phd_last_error().decode("utf-8", "replace")))


def load(path, frame_offset=0, num_frames=-1):
    """-> (float32 tensor [channels, frames], sample_rate), like torchaudio.load."""
    meta, there = _parse(path)
    start = min(max(int(frame_offset), 0), meta.num_frames)
    stop = meta.num_frames if num_frames < 0 else min(meta.num_frames, start + int(num_frames))
    if meta.format_tag in CODED_TAGS:
        return torch.from_numpy(_load_coded(path, meta, there, start, max(stop, start))), meta.sample_rate
    with open(path, "rb") as f:
        f.seek(meta.data_offset + start * meta.block_align)
        raw = f.read((stop - start) * meta.block_align)
    bits = meta.bits_per_sample
    if meta.format_tag == 3:
        a = np.frombuffer(raw, dtype="<f4" if bits == 32 else "<f8").astype(np.float32)
    elif bits == 8:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) * (1.0 / 128.0)
    elif bits == 16:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) * (1.0 / 32768.0)
    elif bits == 24:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = (b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) << 8                 # sign bit into bit 31
        a = (v >> 8).astype(np.float32) * (1.0 / 8388608.0)
    else:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float32) * (1.0 / 2147483648.0)
    return torch.from_numpy(np.ascontiguousarray(a.reshape(-1, meta.num_channels).T)), meta.sample_rate


def read_payload(path, into=None):
    """-> (payload, WavInfo): the bytes of the data chunk, `num_frames * block_align` of them, undecoded (the device decodes
    them, generate.pcm_decode).  `into`: a writable buffer at least that long, or a callable that is given the byte count
    and returns one (a pinned host tensor's memory); the payload is a view of it, cut to size.  Default: a bytearray.  A
    data chunk that promises more than the file holds is cut to the whole frames that are there, as `load` reads it.  A coded file
    (CODED_TAGS): the data chunk's bytes as they stand -- every byte of it that is in the file; the WavInfo's num_frames says how many
    frames the device decoder (generate.g711_decode / ima_decode) is to take from them."""
    meta, held = _parse(path)
    with open(path, "rb") as f:
        if meta.format_tag in CODED_TAGS:
            n = held
            buf = bytearray(n) if into is None else into(n) if callable(into) else into
            buf = memoryview(buf).cast("B")
            if len(buf) < n:
                raise ValueError(f"{path}: the buffer holds {len(buf)} bytes, the data chunk {n}")
            f.seek(meta.data_offset)
            if f.readinto(buf[:n]) != n:
                raise ValueError(f"{path}: short read of the data chunk")
            return buf[:n], meta
        there = max(os.fstat(f.fileno()).st_size - meta.data_offset, 0) // meta.block_align
        if there < meta.num_frames:
            meta = meta._replace(num_frames=there)
        n = meta.num_frames * meta.block_align
        buf = bytearray(n) if into is None else into(n) if callable(into) else into
        buf = memoryview(buf).cast("B")
        if len(buf) < n:
            raise ValueError(f"{path}: the buffer holds {len(buf)} bytes, the data chunk {n}")
        f.seek(meta.data_offset)
        if f.readinto(buf[:n]) != n:
            raise ValueError(f"{path}: short read of the data chunk")
    return buf[:n], meta


def read_frames(path, meta, start, stop, into=None):
    """-> the bytes of frames [start, stop) of a file whose coding has a fixed size per frame (PCM, IEEE float, G.711: `meta` is the
    file's WavInfo, or the AudioInfo of an AIFF, AU or SPHERE file, whose sound data is laid out the same way), undecoded: one seek
    and one read.  `into`: as read_payload's.  The header is not parsed again; an IMA ADPCM file, whose frames share blocks, is a
    ValueError, and so is a range outside the file's frames."""
    if meta.format_tag == 0x11:
        raise ValueError(f"{path}: IMA ADPCM has no fixed size per frame: a frame range of it is not read")
    start, stop = int(start), int(stop)
    if not 0 <= start <= stop <= meta.num_frames:
        raise ValueError(f"{path}: frames {start}..{stop} are not inside the file's {meta.num_frames}")
    n = (stop - start) * meta.block_align
    buf = bytearray(n) if into is None else into(n) if callable(into) else into
    buf = memoryview(buf).cast("B")
    if len(buf) < n:
        raise ValueError(f"{path}: the buffer holds {len(buf)} bytes, the frames {n}")
    with open(path, "rb") as f:
        f.seek(meta.data_offset + start * meta.block_align)
        if n and f.readinto(buf[:n]) != n:
            raise ValueError(f"{path}: short read of the data chunk")
    return buf[:n]


def frame_info(path):
    """-> WavInfo with num_frames cut to the whole frames the file holds, as read_payload returns it: what read_frames is given."""
    meta, held = _parse(path)
    if meta.format_tag not in CODED_TAGS:
        meta = meta._replace(num_frames=min(meta.num_frames, held // meta.block_align))
    return meta


# encoding -> (format tag, bits per sample)
ENCODINGS ={"pcm16": (1, 16), "pcm24": (1, 24), "float32": (3, 32)}


def write_payload(path, payload, sample_rate, channels, encoding="pcm16"):
    """A 44-byte header (format tag 1 for the PCM encodings, 3 for float32) and `payload`, the interleaved little-endian
    samples as they stand."""
    if encoding not in ENCODINGS:
        raise ValueError(f"wavio: encoding must be one of {sorted(ENCODINGS)}, got {encoding!r}")
    tag, bits = ENCODINGS[encoding]
    align = int(channels) * bits // 8
    payload = memoryview(payload).cast("B")
    if channels < 1 or len(payload) % align:
        raise ValueError(f"wavio: {len(payload)} bytes are not whole frames of {channels} x {bits} bit")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(payload) + (len(payload) & 1)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, tag, int(channels), int(sample_rate), int(sample_rate) * align, align, bits))
        f.write(b"data" + struct.pack("<I", len(payload)))
        f.write(payload)
        if len(payload) & 1:
            f.write(b"\0")                                            # RIFF chunks are word-aligned


def payload_of(waveform, encoding="pcm16"):
    """waveform [channels, frames] or [frames] -> (the interleaved little-endian payload, channels): the clamping and rounding of
    `save`, shared with flacio.save."""
    if encoding not in ENCODINGS:
        raise ValueError(f"wavio: encoding must be one of {sorted(ENCODINGS)}, got {encoding!r}")
    w = torch.as_tensor(waveform).detach().cpu().float()
    if w.dim() == 1:
        w = w.unsqueeze(0)
    if encoding == "pcm16":
        pcm = (w.clamp(-1.0, 32767.0 / 32768.0) * 32768.0).round().to(torch.int16).T.contiguous().numpy().tobytes()
    elif encoding == "pcm24":
        q = (w.clamp(-1.0, 8388607.0 / 8388608.0) * 8388608.0).round().to(torch.int32).T.contiguous().numpy()
        pcm = np.ascontiguousarray(q.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()
    else:
        pcm = w.T.contiguous().numpy().astype("<f4").tobytes()
    return pcm, w.shape[0]


def save(path, waveform, sample_rate, encoding="pcm16"):
    """Writer (torchaudio.save's default for float input is float32; the reference's outputs are listened to, not re-read,
    generate_audio.py:65): waveform [channels, frames] or [frames].  `encoding`: 'pcm16' (default) and 'pcm24' clamp to
    [-1, 1 - 2^-(bits-1)], scale by 2^(bits-1) and round half to even; 'float32' writes the values as they are."""
    pcm, channels = payload_of(waveform, encoding)
    write_payload(path, pcm, sample_rate, channels, encoding)
