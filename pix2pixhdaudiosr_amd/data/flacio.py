"""FLAC reader for the feeder and for whole-file generation (the reference reads .flac through torchaudio; this build has its own
decoder, csrc/flac.hip): native FLAC streams, the subset include/p2phd.h writes down.  `info` / `load` have the shape of wavio's;
samples come out as wavio.load returns the same samples from a WAV: float32 [channels, frames], integer x 2^-(bits-1).

Everything here runs on the host (p2phd_flac_info / p2phd_flac_index / p2phd_flac_decode_host need no device): DataLoader workers
have none.  The frame index of a file -- one row per frame, every CRC verified -- is built once per (path, size, mtime) and kept
in a bounded cache of the process, so with the cache warm a random training segment costs one seek, one read of the covering
frames' bytes and their decode.  Whole-file generation copies the file's bytes and the index to the device instead and decodes
there (generate.flac_decode).

FLAC writer (csrc/flacenc.hip, the stream contract of include/p2phd.h): `encode` is the host encoder p2phd_flac_encode_host,
`write_stream` puts "fLaC" and STREAMINFO in front of encoded frames -- the host encoder's or the device encoder's
(generate.flac_encode) -- and `save` is the twin of wavio.save."""
import ctypes
import hashlib
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch

# the leading four fields are WavInfo's; num_flac_frames: rows of the frame index
FlacInfo = namedtuple("FlacInfo", "sample_rate num_frames num_channels bits_per_sample min_block max_block first_frame_offset md5 seek_points "
                                  "num_flac_frames")

ROW = 6                                                                     # P2PHD_FLAC_ROW_WORDS: offset, length, first sample, block size, assignment, bits
INDEX_CACHE_ENTRIES = 4096                                                  # files whose index the process keeps
STATS = {"index_builds": 0, "index_hits": 0}                                # (tests read these)
_CACHE = OrderedDict()                                                      # (path, size, mtime_ns) -> (FlacInfo, table)


class _StreamInfo(ctypes.Structure):
    """struct p2phd_flac_streaminfo (include/p2phd.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("sample_rate", "channels", "bits", "min_block", "max_block", "seek_points")] + \
               [("total_samples", ctypes.c_int64), ("first_frame_offset", ctypes.c_int64), ("md5", ctypes.c_uint8 * 16)]


def _lib():
    from .. import _lib as L
    return L.lib()


def _err(name):
    return ValueError("%s: %s" % (name, _lib().p2phd_last_error().decode("utf-8", "replace")))


def _address(buf):
    """(address, length, keep-alive) of a bytes-like object."""
    a = np.frombuffer(buf, dtype=np.uint8)
    return ctypes.c_void_p(a.ctypes.data if a.size else None), a.size, a


def index_bytes(buf, name="<bytes>"):
    """The whole stream as a bytes-like object -> (FlacInfo, table): table int64 [frames, 6], one row per frame
    (p2phd_flac_index: every CRC-8 and CRC-16 verified, the frames chained without a gap, the sample numbers consecutive).
    Anything the subset does not hold, and any corruption, is a ValueError that names `name` and the reason."""
    lib = _lib()
    addr, n, keep = _address(buf)
    si = _StreamInfo()
    if lib.p2phd_flac_info(addr, n, ctypes.byref(si)) != 0:
        raise _err(name)
    count = lib.p2phd_flac_index(addr, n, None, 0)
    if count < 0:
        raise _err(name)
    table = np.zeros((count, ROW), dtype=np.int64)
    if count and lib.p2phd_flac_index(addr, n, ctypes.c_void_p(table.ctypes.data), count) != count:
        raise _err(name)
    total = int(table[:, 3].sum()) if count else 0
    meta = FlacInfo(si.sample_rate, total, si.channels, si.bits, si.min_block, si.max_block, si.first_frame_offset, bytes(si.md5), si.seek_points, count)
    return meta, table


def _indexed(path):
    path = os.fspath(path)
    st = os.stat(path)
    key = (os.path.abspath(path), st.st_size, st.st_mtime_ns)
    hit = _CACHE.get(key)
    if hit is not None:
        _CACHE.move_to_end(key)
        STATS["index_hits"] += 1
        return hit
    with open(path, "rb") as f:
        data = f.read()
    hit = index_bytes(data, path)
    hit[1].setflags(write=False)
    STATS["index_builds"] += 1
    _CACHE[key] = hit
    while len(_CACHE) > INDEX_CACHE_ENTRIES:
        _CACHE.popitem(last=False)
    return hit


def info(path):
    """-> FlacInfo (num_frames: the samples the frames hold, counted where STREAMINFO states 0).  Builds, or re-uses, the file's index."""
    return _indexed(path)[0]


def decode_frames(buf, table, first, count, channels, name="<bytes>"):
    """Frames [first, first + count) of `table`, whose offsets point into `buf` -> int32 [channels, samples] (p2phd_flac_decode_host)."""
    rows = table[first:first + count]
    total = int(rows[:, 3].sum()) if count else 0
    out = np.zeros((channels, total), dtype=np.int32)
    if count:
        addr, n, keep = _address(buf)
        t = np.ascontiguousarray(table, dtype=np.int64)
        if _lib().p2phd_flac_decode_host(addr, n, ctypes.c_void_p(t.ctypes.data), int(first), int(count), int(channels), ctypes.c_void_p(out.ctypes.data), total) != 0:
            raise _err(name)
    return out


def load(path, frame_offset=0, num_frames=-1):
    """-> (float32 tensor [channels, frames], sample_rate), like wavio.load: only the FLAC frames that cover the window are read and
    decoded (on the host)."""
    meta, table = _indexed(path)
    start = min(max(int(frame_offset), 0), meta.num_frames)
    stop = meta.num_frames if num_frames < 0 else min(meta.num_frames, start + int(num_frames))
    if stop <= start:
        return torch.zeros((meta.num_channels, 0), dtype=torch.float32), meta.sample_rate
    first_sample = table[:, 2] - table[0, 2]
    f0 = int(np.searchsorted(first_sample, start, side="right")) - 1
    f1 = int(np.searchsorted(first_sample, stop, side="left"))                # one behind the last covering frame
    byte0, byte1 = int(table[f0, 0]), int(table[f1 - 1, 0] + table[f1 - 1, 1])
    with open(path, "rb") as f:
        f.seek(byte0)
        data = f.read(byte1 - byte0)
    if len(data) != byte1 - byte0:
        raise ValueError("%s: short read of frames %d .. %d" % (path, f0, f1 - 1))
    rows = table[f0:f1].copy()
    rows[:, 0] -= byte0
    pcm = decode_frames(data, rows, 0, f1 - f0, meta.num_channels, path)
    lo = start - int(first_sample[f0])
    a = pcm[:, lo:lo + (stop - start)].astype(np.float32) * np.float32(2.0 ** -(meta.bits_per_sample - 1))
    return torch.from_numpy(np.ascontiguousarray(a)), meta.sample_rate


def read_file(path, into=None):
    """-> (bytes, FlacInfo, table): the whole file, undecoded (the device decodes it, generate.flac_decode), and its index, built
    from those bytes.  `into`: as wavio.read_payload's -- a writable buffer at least as long as the file, or a callable that is given
    the byte count and returns one (a pinned host tensor's memory); the bytes are a view of it, cut to size."""
    with open(path, "rb") as f:
        n = os.fstat(f.fileno()).st_size
        buf = bytearray(n) if into is None else into(n) if callable(into) else into
        buf = memoryview(buf).cast("B")
        if len(buf) < n:
            raise ValueError(f"{path}: the buffer holds {len(buf)} bytes, the file {n}")
        if f.readinto(buf[:n]) != n:
            raise ValueError(f"{path}: short read")
    meta, table = index_bytes(buf[:n], os.fspath(path))
    return buf[:n], meta, table


def verify(path):
    """Decodes the whole file on the host and compares the MD5 of its interleaved little-endian samples with STREAMINFO's -> True /
    False; None where STREAMINFO's is all zeros ("not set")."""
    meta, table = _indexed(path)
    if meta.md5 == b"\0" * 16:
        return None
    with open(path, "rb") as f:
        data = f.read()
    pcm = decode_frames(data, table, 0, meta.num_flac_frames, meta.num_channels, path)
    nb = (meta.bits_per_sample + 7) // 8
    le = np.ascontiguousarray(pcm.T).astype("<i4").reshape(-1, 1).view(np.uint8)[:, :nb]
    return hashlib.md5(np.ascontiguousarray(le).tobytes()).digest() == meta.md5


# ---- writer ------------------------------------------------------------------------------------------------------------------
DEFAULT_BLOCK = 4096
MAX_LPC_ORDER = 12                                                          # the option lpc_order: 0 (off) .. 12
MAX_LPC_BLOCK = 16384                                                       # the largest block with lpc_order > 0
ENCODINGS = {"pcm16": 16, "pcm24": 24}                                      # what a FLAC stream of this build holds


def check_output(channels, bits, rate, block, what="flacio"):
    """The writer's refusals, raised before a file is opened: the ranges of the stream contract."""
    if bits not in (16, 24):
        raise ValueError("%s: FLAC output holds pcm16 or pcm24 samples, not %r bits (float32 is not built)" % (what, bits))
    if not 1 <= int(channels) <= 8:
        raise ValueError("%s: FLAC output holds 1 to 8 channels, not %r" % (what, channels))
    if not 16 <= int(block) <= 65535:
        raise ValueError("%s: the FLAC block size must lie in 16 .. 65535, got %r" % (what, block))
    if not 1 <= int(rate) <= 1048575:
        raise ValueError("%s: the sample rate of a FLAC stream must lie in 1 .. 1048575, got %r" % (what, rate))


def encode_plan(channels, bits, total, block=DEFAULT_BLOCK):
    """-> (frames, worst-case bytes of the frames, workspace bytes of the device encoder): p2phd_flac_encode_plan."""
    out = (ctypes.c_int64 * 3)()
    addr = ctypes.addressof(out)
    if _lib().p2phd_flac_encode_plan(int(channels), int(bits), int(total), int(block), ctypes.c_void_p(addr), ctypes.c_void_p(addr + 8),
                                     ctypes.c_void_p(addr + 16)) != 0:
        raise _err("flac_encode_plan")
    return int(out[0]), int(out[1]), int(out[2])


def check_lpc(lpc_order, block, what="flacio"):
    """The LPC option's refusals (include/p2phd.h, "FLAC output, LPC"): an int in 0 .. MAX_LPC_ORDER, and with it a block of at most
    MAX_LPC_BLOCK."""
    if isinstance(lpc_order, bool) or not isinstance(lpc_order, int) or not 0 <= lpc_order <= MAX_LPC_ORDER:
        raise ValueError("%s: the LPC order must be an int in 0 .. %d, got %r" % (what, MAX_LPC_ORDER, lpc_order))
    if lpc_order > 0 and int(block) > MAX_LPC_BLOCK:
        raise ValueError("%s: with LPC subframes the FLAC block size is at most %d, got %r" % (what, MAX_LPC_BLOCK, block))


def encode(samples_or_payload, channels=None, bits=16, rate=44100, block=DEFAULT_BLOCK, lpc_order=0):
    """The host encoder (p2phd_flac_encode_host, one thread, no device; with lpc_order M > 0 p2phd_flac_encode_lpc_host: every LPC order
    1 .. M is tried beside the fixed predictors, block at most 16384).  `samples_or_payload`: the interleaved little-endian PCM
    payload of `channels` channels as a bytes-like object, or an integer array [channels, samples] (or [samples]) whose values fit
    `bits` -> (the frames back to back as bytes, lengths: int64 [frames + 1], each frame's bytes and their total)."""
    if isinstance(samples_or_payload, np.ndarray) and samples_or_payload.dtype != np.uint8:
        a = np.atleast_2d(samples_or_payload)
        lim = 1 << (bits - 1)
        if a.size and (a.min() < -lim or a.max() >= lim):
            raise ValueError("flacio.encode: samples outside %d bits" % bits)
        channels = a.shape[0]
        le = np.ascontiguousarray(a.T).astype("<i4").reshape(-1, 1).view(np.uint8)[:, :bits // 8]
        payload = np.ascontiguousarray(le).reshape(-1)
    else:
        payload = np.frombuffer(samples_or_payload, dtype=np.uint8)
        if channels is None:
            raise ValueError("flacio.encode: a payload needs its channel count")
    check_output(channels, bits, rate, block, "flacio.encode")
    check_lpc(lpc_order, block, "flacio.encode")
    align = int(channels) * bits // 8
    if payload.size == 0 or payload.size % align:
        raise ValueError("flacio.encode: %d bytes are not one or more whole frames of %d x %d bit" % (payload.size, channels, bits))
    total = payload.size // align
    frames, worst, _ = encode_plan(channels, bits, total, block)
    out = np.empty(worst, dtype=np.uint8)
    lengths = np.zeros(frames + 1, dtype=np.int64)
    payload = np.ascontiguousarray(payload)
    if lpc_order:
        if _lib().p2phd_flac_encode_lpc_host(ctypes.c_void_p(payload.ctypes.data), int(channels), int(bits), total, int(rate), int(block), lpc_order,
                                             ctypes.c_void_p(out.ctypes.data), worst, ctypes.c_void_p(lengths.ctypes.data)) != 0:
            raise _err("flac_encode_lpc_host")
    elif _lib().p2phd_flac_encode_host(ctypes.c_void_p(payload.ctypes.data), int(channels), int(bits), total, int(rate), int(block),
                                       ctypes.c_void_p(out.ctypes.data), worst, ctypes.c_void_p(lengths.ctypes.data)) != 0:
        raise _err("flac_encode_host")
    return out[:int(lengths[-1])].tobytes(), lengths


def stream_header(lengths, rate, channels, bits, total, block, md5=None):
    """"fLaC" and the one STREAMINFO block (last-block flag set) in front of frames of the given lengths (int64 [frames + 1], as the
    encoders return them; the last entry, their total, is not a frame)."""
    check_output(channels, bits, rate, block, "flacio.stream_header")
    each = np.asarray(lengths, dtype=np.int64)[:-1]
    if each.size == 0 or not 1 <= int(total) < 1 << 36:
        raise ValueError("flacio.stream_header: no frames, or a total outside 1 .. 2^36 - 1")
    md5 = b"\0" * 16 if md5 is None else bytes(md5)
    if len(md5) != 16:
        raise ValueError("flacio.stream_header: an MD5 has 16 bytes")
    lo, hi = min(int(each.min()), 0xFFFFFF), min(int(each.max()), 0xFFFFFF)
    v = (int(rate) << 44) | ((int(channels) - 1) << 41) | ((int(bits) - 1) << 36) | int(total)
    info_block = int(block).to_bytes(2, "big") * 2 + lo.to_bytes(3, "big") + hi.to_bytes(3, "big") + v.to_bytes(8, "big") + md5
    return b"fLaC" + bytes([0x80]) + len(info_block).to_bytes(3, "big") + info_block


def write_stream(path, frames, lengths, rate, channels, bits, total, block, md5=None):
    """The one place that turns encoded frames into a file: header, STREAMINFO, then frames[:lengths[-1]] (a bytes-like object or a
    uint8 array, which may be longer: the device encoder's stream comes back at its worst-case size) -> the bytes written."""
    head = stream_header(lengths, rate, channels, bits, total, block, md5)
    n = int(np.asarray(lengths)[-1])
    body = memoryview(frames).cast("B")
    if len(body) < n:
        raise ValueError("flacio.write_stream: %d bytes of frames, the lengths state %d" % (len(body), n))
    with open(path, "wb") as f:
        f.write(head)
        f.write(body[:n])
    return len(head) + n


def save(path, waveform, sample_rate, encoding="pcm16", block=DEFAULT_BLOCK):
    """The twin of wavio.save: waveform [channels, frames] or [frames], clamped and rounded by the same expression (wavio.payload_of),
    encoded on the host, MD5 of the payload in STREAMINFO.  'float32' is refused: FLAC holds integers."""
    from . import wavio
    if encoding not in ENCODINGS:
        raise ValueError("flacio.save: encoding must be one of %s, got %r (float32 is not built for FLAC)" % (sorted(ENCODINGS), encoding))
    bits = ENCODINGS[encoding]
    w = torch.as_tensor(waveform)
    channels = 1 if w.dim() == 1 else w.shape[0]
    check_output(channels, bits, sample_rate, block, "flacio.save")
    pcm, channels = wavio.payload_of(w, encoding)
    frames, lengths = encode(pcm, channels, bits, sample_rate, block)
    return write_stream(path, frames, lengths, sample_rate, channels, bits, len(pcm) // (channels * bits // 8), block, hashlib.md5(pcm).digest())
