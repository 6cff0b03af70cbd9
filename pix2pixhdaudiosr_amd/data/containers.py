"""Readers of the three big-endian containers -- AIFF / AIFF-C, Sun/NeXT AU (.snd) and NIST SPHERE -- for the feeder and for
whole-file generation (stand in for torchaudio.info / torchaudio.load of these files, data/audio_dataset.py:31-38,99).  Host I/O
only, wavio's shapes: `info`, `load` (a seek to the frame window), `read_payload` (the bytes as they stand, for the device decoder).

The contract (include/p2phd.h, "Big-endian containers"): a file decodes to exactly the float32 samples wavio.load returns for its WAV
twin, the RIFF file that holds the same samples -- integer PCM of the same width scaled by 2^-(8 * bytes - 1), a signed 8-bit sample s
as s / 128 (its twin holds s + 128), float32 as a bit copy after the byte swap, float64 rounded to nearest even, G.711 as the same
bytes under format tags 6 / 7.  Here the PCM is decoded with numpy and G.711 with the library's host entry (p2phd_g711_decode_host);
in whole-file generation by generate.pcm_decode(..., big_endian=, signed8=) and generate.g711_decode.

Not read, each refused with its name: AIFF-C ima4 / MAC3 / MAC6 / G722 / GSM / Qclp / QDMC (QuickTime decoders disagree on whether an
ima4 packet's header or the running state holds the predictor, so no PCM twin is defined for it), AU's G.72x codes 23 - 26 and the
byte-swapped magic 'dns.', shorten- or wavpack-coded SPHERE, non-integer sample rates.  Every refusal is a ValueError that starts with
the path, a file cut inside its header included."""
import os
import struct
from collections import namedtuple

import numpy as np
import torch

from . import wavio

# WavInfo's seven fields lead, so whatever reads those reads an AudioInfo.  format_tag: WAVE's codes (1 integer PCM, 3 IEEE float,
# 6 A-law, 7 mu-law); bits_per_sample: the container width of a sample; container: 'aiff' | 'au' | 'sphere'; coding: the file's own
# word for what it holds (AIFF-C's four characters, AU's encoding number, SPHERE's sample_coding).
AudioInfo = namedtuple("AudioInfo", wavio.WavInfo._fields + ("big_endian", "signed8", "container", "coding"))

PCM_MAX_CHANNELS = 65535
_HEADER_LIMIT = 1 << 20                                                    # a SPHERE header that claims more bytes than this is refused


def kind_of(head):
    """The first bytes of a file (4 are enough) -> 'aiff', 'au', 'sphere' or None."""
    head = bytes(head[:4])
    return {b"FORM": "aiff", b".snd": "au", b"NIST": "sphere"}.get(head)


def _meta(path, container, coding, tag, rate, channels, nbytes, offset, there, frames=None, big_endian=True, signed8=False):
    """The checks every container shares -> (AudioInfo, bytes of payload in the file).  `there`: payload bytes the file holds;
    `frames`: what the header states (None: what the file holds), cut to the whole frames that are there (wavio's rule)."""
    what = "G.711" if tag in (6, 7) else "PCM"
    most = wavio.CODED_MAX_CHANNELS if tag in (6, 7) else PCM_MAX_CHANNELS
    if not 1 <= channels <= most:
        raise ValueError(f"{path}: {what} ({coding}) is read with 1 to {most} channels, the header states {channels}")
    if not 1 <= rate <= 0x7FFFFFFF:
        raise ValueError(f"{path}: the sample rate must be a positive integer that int32 holds, the header states {rate}")
    align = channels * nbytes
    held = max(there, 0) // align
    frames = held if frames is None else min(int(frames), held)
    return AudioInfo(int(rate), frames, channels, 8 * nbytes, tag, offset, align, bool(big_endian) and nbytes > 1, bool(signed8),
                     container, coding), frames * align


def _need(path, data, n, what):
    if len(data) < n:
        raise ValueError(f"{path}: the file ends inside {what}")
    return data


# ---- AIFF / AIFF-C ---------------------------------------------------------------------------------------------------------------
def extended_rate(path, ten):
    """The 80-bit IEEE 754 extended of a COMM chunk -> its value as a Python int, exactly.  Zero, negative, non-integral, infinite
    and NaN rates are refused by name."""
    se, mant = struct.unpack(">HQ", ten)
    exp = se & 0x7FFF
    if exp == 0x7FFF:
        raise ValueError(f"{path}: the sample rate of the COMM chunk is " + ("NaN" if mant & 0x7FFFFFFFFFFFFFFF else "infinite"))
    if mant == 0:
        raise ValueError(f"{path}: the sample rate of the COMM chunk is zero")
    if se & 0x8000:
        raise ValueError(f"{path}: the sample rate of the COMM chunk is negative")
    shift = exp - 16383 - 63                                               # value = mant * 2^shift
    if shift >= 0:
        value = mant << min(shift, 64)                                     # (far beyond int32 either way)
    else:
        if -shift >= 64 or mant & ((1 << -shift) - 1):
            raise ValueError(f"{path}: the sample rate of the COMM chunk is not an integer ({mant * 2.0 ** shift!r} Hz)")
        value = mant >> -shift
    if value > 0x7FFFFFFF:
        raise ValueError(f"{path}: the sample rate of the COMM chunk, {value} Hz, is more than int32 holds")
    return value


# compression type -> (format tag, bytes per sample or None for "ceil(sampleSize / 8)", big-endian)
_AIFC_TYPES = {b"NONE": (1, None, True), b"twos": (1, None, True), b"in24": (1, 3, True), b"in32": (1, 4, True),
               b"sowt": (1, None, False), b"raw ": (1, 1, True),
               b"fl32": (3, 4, True), b"FL32": (3, 4, True), b"fl64": (3, 8, True), b"FL64": (3, 8, True),
               b"ulaw": (7, 1, True), b"ULAW": (7, 1, True), b"alaw": (6, 1, True), b"ALAW": (6, 1, True)}
_AIFC_REFUSED = {b"ima4": "IMA 4:1 (QuickTime decoders disagree on where a packet's predictor comes from: no PCM twin is defined)",
                 b"MAC3": "MACE 3:1", b"MAC6": "MACE 6:1", b"G722": "G.722", b"GSM ": "GSM 6.10", b"Qclp": "Qualcomm PureVoice",
                 b"QDMC": "QDesign Music"}


def _parse_aiff(path, f, size):
    head = _need(path, f.read(12), 12, "the FORM header")
    if head[:4] != b"FORM" or head[8:12] not in (b"AIFF", b"AIFC"):
        raise ValueError(f"{path}: a FORM file that is neither AIFF nor AIFF-C (form type {head[8:12]!r})")
    aifc = head[8:12] == b"AIFC"
    comm = ssnd = None
    pos = 12
    while pos < size and (comm is None or ssnd is None):
        f.seek(pos)
        hdr = f.read(8)
        if len(hdr) < 8:
            if comm is None:
                raise ValueError(f"{path}: the file ends inside a chunk header")
            break
        cid, csize = hdr[:4], struct.unpack(">I", hdr[4:])[0]
        if cid == b"COMM":
            need = 22 if aifc else 18
            if csize < need:
                raise ValueError(f"{path}: a COMM chunk of {csize} bytes is too short")
            comm = _need(path, f.read(min(csize, 512)), min(csize, 512), "the COMM chunk")
        elif cid == b"SSND":
            word = _need(path, f.read(8), 8, "the SSND chunk")
            offset = struct.unpack(">I", word[:4])[0]
            if csize < 8 or offset > csize - 8:
                raise ValueError(f"{path}: an SSND chunk of {csize} bytes with a data offset of {offset}")
            ssnd = (pos + 16 + offset, csize - 8 - offset)
        pos += 8 + csize + (csize & 1)                                      # chunks are padded to even sizes
    if comm is None:
        raise ValueError(f"{path}: no COMM chunk")
    channels, frames, bits = struct.unpack(">hIh", comm[:8])
    rate = extended_rate(path, comm[8:18])
    ctype = comm[18:22] if aifc else b"NONE"
    if ctype not in _AIFC_TYPES:
        n = comm[22] if len(comm) > 22 else 0
        name = comm[23:23 + n].decode("latin-1") or "no name given"
        why = ": " + _AIFC_REFUSED[ctype] if ctype in _AIFC_REFUSED else ""
        raise ValueError(f"{path}: AIFF-C compression type {ctype.decode('latin-1')!r} ({name}) is not read{why}")
    tag, nbytes, big = _AIFC_TYPES[ctype]
    coding = ctype.decode("latin-1")
    if tag in (6, 7):
        nbytes = 1                                                         # one byte per sample, whatever sampleSize says (usually 16)
    else:
        if not 1 <= bits <= 32 and tag == 1:
            raise ValueError(f"{path}: a sampleSize of {bits} bits; 1 .. 32 are read")
        stated = (bits + 7) // 8                                           # left-justified in ceil(bits / 8) bytes
        if nbytes is None:
            nbytes = stated
        elif tag == 1 and stated != nbytes:
            raise ValueError(f"{path}: AIFF-C compression type {coding!r} holds {8 * nbytes}-bit samples, the COMM chunk states a sampleSize of {bits}")
    if ssnd is None:
        if frames != 0:
            raise ValueError(f"{path}: no SSND chunk, and the COMM chunk states {frames} frames")
        ssnd = (size, 0)
    start, length = ssnd
    there = min(length, max(size - start, 0))
    signed8 = tag == 1 and nbytes == 1 and ctype != b"raw "
    return _meta(path, "aiff", coding, tag, rate, channels, nbytes, start, there, frames, big_endian=big, signed8=signed8)


# ---- AU ----------------------------------------------------------------------------------------------------------------------------
# encoding -> (format tag, bytes per sample, signed 8-bit)
_AU_ENCODINGS = {1: (7, 1, False), 2: (1, 1, True), 3: (1, 2, False), 4: (1, 3, False), 5: (1, 4, False), 6: (3, 4, False),
                 7: (3, 8, False), 27: (6, 1, False)}
_AU_REFUSED = {23: "G.721 4-bit ADPCM", 24: "G.722", 25: "G.723 3-bit ADPCM", 26: "G.723 5-bit ADPCM"}


def _parse_au(path, f, size):
    head = _need(path, f.read(24), 24, "the AU header")
    magic, offset, length, enc, rate, channels = struct.unpack(">4sIIIII", head)
    if magic != b".snd":
        raise ValueError(f"{path}: not an AU file")
    if offset < 24 or offset > size:
        raise ValueError(f"{path}: the AU header states a data offset of {offset}; it must be at least 24 and inside the file ({size} bytes)")
    if enc not in _AU_ENCODINGS:
        why = f"{_AU_REFUSED[enc]}: there is no decoder for the G.72x family here" if enc in _AU_REFUSED else "an encoding that is not read"
        raise ValueError(f"{path}: AU encoding {enc} ({why})")
    tag, nbytes, signed8 = _AU_ENCODINGS[enc]
    there = size - offset
    if length != 0xFFFFFFFF:                                               # (which means: to the end of the file)
        there = min(there, length)
    return _meta(path, "au", str(enc), tag, rate, channels, nbytes, offset, there, None, big_endian=True, signed8=signed8)


# ---- NIST SPHERE -----------------------------------------------------------------------------------------------------------------
def _parse_sphere(path, f, size):
    first = _need(path, f.read(16), 16, "the SPHERE header")            # 'NIST_1A\n' and the header size, right-justified in 8 bytes
    if first[:8] != b"NIST_1A\n":
        raise ValueError(f"{path}: not a NIST SPHERE file")
    try:
        hsize = int(first[8:].decode("ascii").strip())
    except ValueError:
        raise ValueError(f"{path}: the second line of the SPHERE header does not hold the header size ({first[8:]!r})") from None
    if not 16 <= hsize <= _HEADER_LIMIT:
        raise ValueError(f"{path}: a SPHERE header size of {hsize} bytes")
    f.seek(0)
    header = _need(path, f.read(hsize), hsize, "the SPHERE header")
    fields, ended = {}, False
    for line in header[16:].split(b"\n"):
        line = line.decode("latin-1").strip()
        if line == "end_head":
            ended = True
            break
        if not line or line[0] == ";":
            continue
        parts = line.split(None, 2)
        if len(parts) < 3 or parts[1][:2] not in ("-i", "-r", "-s"):
            raise ValueError(f"{path}: a SPHERE header line that is not 'key -type value': {line!r}")
        fields[parts[0]] = (parts[1][1], parts[2].strip())
    if not ended:
        raise ValueError(f"{path}: the SPHERE header has no end_head line")

    def number(key, needed=True):
        if key not in fields:
            if needed:
                raise ValueError(f"{path}: the SPHERE header has no {key}")
            return None
        kind, text = fields[key]
        try:
            if kind == "r":
                value = float(text)
                if value != value or value in (float("inf"), float("-inf")) or value != int(value):
                    raise ValueError
                return int(value)
            return int(text)
        except ValueError:
            raise ValueError(f"{path}: the SPHERE header's {key} must be an integer, it states {text!r}") from None

    channels, rate, nbytes = number("channel_count"), number("sample_rate"), number("sample_n_bytes")
    frames = number("sample_count", needed=False)
    coding = fields.get("sample_coding", ("s", "pcm"))[1]
    base, comma, suffix = coding.partition(",")
    if comma:
        raise ValueError(f"{path}: SPHERE sample_coding {coding!r}: there is no decoder for the compressed part {suffix!r} (shorten, wavpack)")
    big = True
    if base == "pcm":
        if nbytes != 2:
            raise ValueError(f"{path}: SPHERE pcm with a sample_n_bytes of {nbytes}; 2 is read")
        order = fields.get("sample_byte_format", (None, None))[1]
        if order not in ("01", "10"):
            raise ValueError(f"{path}: SPHERE pcm needs a sample_byte_format of 01 or 10, the header states {order!r}")
        tag, big = 1, order == "10"
    elif base in ("ulaw", "mu-law", "alaw"):
        if nbytes != 1:
            raise ValueError(f"{path}: SPHERE {base} with a sample_n_bytes of {nbytes}; 1 is read")
        tag = 6 if base == "alaw" else 7
    else:
        raise ValueError(f"{path}: SPHERE sample_coding {coding!r} is not read (pcm, ulaw, mu-law, alaw are)")
    if frames is not None and frames < 0:
        raise ValueError(f"{path}: the SPHERE header's sample_count is negative ({frames})")
    return _meta(path, "sphere", coding, tag, rate, channels, nbytes, hsize, size - hsize, frames, big_endian=big)


_PARSERS = {"aiff": _parse_aiff, "au": _parse_au, "sphere": _parse_sphere}


def _parse(path):
    """-> (AudioInfo, the bytes of payload that num_frames stands for)."""
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        head = f.read(4)
        if head == b"dns.":
            raise ValueError(f"{path}: an AU file with the byte-swapped magic 'dns.' (little-endian header) is not read")
        kind = kind_of(head)
        if kind is None:
            raise ValueError(f"{path}: not an AIFF, AU or NIST SPHERE file")
        f.seek(0)
        try:
            return _PARSERS[kind](path, f, size)
        except struct.error as e:                                          # (a header cut where a fixed-size record was expected)
            raise ValueError(f"{path}: the file ends inside its header ({e})") from None


def info(path):
    """-> AudioInfo: num_frames as the header states them, cut to the whole frames the file holds."""
    return _parse(path)[0]


def decode_host(raw, meta):
    """The interleaved bytes of whole frames, as they stand in the file -> float32 [channels, frames] (numpy): the samples of the
    WAV twin.  G.711 goes through the library's host decoder."""
    C = meta.num_channels
    nbytes = meta.bits_per_sample // 8
    n = len(raw) // meta.block_align
    if meta.format_tag in (6, 7):
        import ctypes
        from .. import _lib as L
        out = np.zeros((C, n), dtype=np.float32)
        if n:
            src = np.frombuffer(raw, dtype=np.uint8)
            rc = L.lib().p2phd_g711_decode_host(ctypes.c_void_p(src.ctypes.data), n, C, 1 if meta.format_tag == 6 else 0,
                                                ctypes.c_void_p(out.ctypes.data), n)
            if rc != 0:
                raise ValueError("g711_decode_host: %s" % L.lib().p2phd_last_error().decode("utf-8", "replace"))
        return out
    order = ">" if meta.big_endian else "<"
    if meta.format_tag == 3:
        if nbytes == 4:                                                    # a bit copy behind the swap: a NaN keeps its payload
            a = np.frombuffer(raw, dtype=order + "u4").astype(np.uint32).view(np.float32)
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                a = np.frombuffer(raw, dtype=order + "f8").astype(np.float32)
    elif nbytes == 1:
        b = np.frombuffer(raw, dtype=np.int8 if meta.signed8 else np.uint8).astype(np.float32)
        a = (b if meta.signed8 else b - 128.0) * np.float32(1.0 / 128.0)
    elif nbytes == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        hi, lo = (0, 2) if meta.big_endian else (2, 0)
        v = (b[:, lo] | (b[:, 1] << 8) | (b[:, hi] << 16)) << 8           # sign bit into bit 31
        a = (v >> 8).astype(np.float32) * np.float32(1.0 / 8388608.0)
    else:
        a = np.frombuffer(raw, dtype=order + ("i2" if nbytes == 2 else "i4")).astype(np.float32) * np.float32(2.0 ** -(8 * nbytes - 1))
    return np.ascontiguousarray(a.reshape(-1, C).T)


def load(path, frame_offset=0, num_frames=-1):
    """-> (float32 tensor [channels, frames], sample_rate), like wavio.load: one seek to the window, one read of it."""
    meta, _ = _parse(path)
    start = min(max(int(frame_offset), 0), meta.num_frames)
    stop = meta.num_frames if num_frames < 0 else min(meta.num_frames, start + int(num_frames))
    stop = max(stop, start)
    want = (stop - start) * meta.block_align
    with open(path, "rb") as f:
        f.seek(meta.data_offset + start * meta.block_align)
        raw = f.read(want)
    if len(raw) != want:
        raise ValueError(f"{path}: short read of the sound data")
    return torch.from_numpy(decode_host(raw, meta)), meta.sample_rate


def read_payload(path, into=None):
    """-> (payload, AudioInfo): the `num_frames * block_align` bytes of sound data as they stand in the file, undecoded (the device
    decodes them: generate.pcm_decode with big_endian / signed8, generate.g711_decode).  `into`: as wavio.read_payload's."""
    meta, n = _parse(path)
    buf = bytearray(n) if into is None else into(n) if callable(into) else into
    buf = memoryview(buf).cast("B")
    if len(buf) < n:
        raise ValueError(f"{path}: the buffer holds {len(buf)} bytes, the sound data {n}")
    with open(path, "rb") as f:
        f.seek(meta.data_offset)
        if n and f.readinto(buf[:n]) != n:
            raise ValueError(f"{path}: short read of the sound data")
    return buf[:n], meta
