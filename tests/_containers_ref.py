"""What Python's aifc / sunau cannot make, assembled with struct straight from the specifications (AIFF 1.3 and AIFF-C draft 8/26/91,
the Sun audio(4) header, NIST SPHERE 2.6): writers of AIFF / AIFF-C, AU and SPHERE files around a payload, the payloads of every
coding of the "Big-endian containers" contract (include/p2phd.h) from integer or float sample arrays, and their decoding with numpy
('>i2', '>f4', ...) and the G.711 table of _wavcodec_ref (== audioop, tests/test_wavcodec_host.py).  Nothing here calls the library."""
import struct

import numpy as np

import _wavcodec_ref as W


# ---- samples <-> payload bytes -------------------------------------------------------------------------------------------------
def int_bytes(ints, width, big=True):
    """int [channels, frames] -> interleaved two's-complement samples of `width` bytes."""
    v = np.ascontiguousarray(np.asarray(ints, dtype=np.int64).T).reshape(-1) & ((1 << (8 * width)) - 1)
    order = range(width - 1, -1, -1) if big else range(width)
    return np.stack([(v >> (8 * k)) & 255 for k in order], axis=1).astype(np.uint8).tobytes()


def int_scale(ints, width):
    """What the WAV twin gives: one int -> float32 conversion (round to nearest even at 32 bits), an exact power-of-two scale."""
    return np.asarray(ints, dtype=np.int64).astype(np.float32) * np.float32(2.0 ** -(8 * width - 1))


def float_bytes(x, width, big=True):
    """float array [channels, frames] (float32 for width 4, float64 for 8) -> interleaved IEEE samples; a bit copy."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32 if width == 4 else np.float64).T).reshape(-1)
    u = a.view(np.uint32 if width == 4 else np.uint64)
    return u.astype((">" if big else "<") + ("u4" if width == 4 else "u8")).tobytes()


def float_value(x, width):
    """float32: itself (bit for bit); float64: rounded to nearest even, numpy's astype."""
    if width == 4:
        return np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def int_samples(rng, width, channels, frames):
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    x = rng.integers(lo, hi + 1, size=(channels, frames), dtype=np.int64)
    edge = [lo, hi, -1, 0, 1, lo + 1, hi - 1]
    x.reshape(-1)[:min(len(edge), x.size)] = edge[:x.size]
    return x


def float_samples(rng, width, channels, frames):
    x = rng.uniform(-1.0, 1.0, size=(channels, frames))
    return x.astype(np.float32) if width == 4 else x


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- AIFF / AIFF-C -----------------------------------------------------------------------------------------------------------------
def ext80(value):
    """An integer, a float or a fraction.Fraction-like number -> the 10 bytes of an IEEE 754 80-bit extended (truncated mantissa)."""
    if value != value:
        return struct.pack(">HQ", 0x7FFF, 0xC000000000000000)
    if value in (float("inf"), float("-inf")):
        return struct.pack(">HQ", 0x7FFF | (0x8000 if value < 0 else 0), 0x8000000000000000)
    if value == 0:
        return bytes(10)
    from fractions import Fraction
    sign, q = (0x8000, -Fraction(value)) if value < 0 else (0, Fraction(value))
    e = 0
    while q >= 2:
        q, e = q / 2, e + 1
    while q < 1:
        q, e = q * 2, e - 1
    return struct.pack(">HQ", sign | (e + 16383), int(q * (1 << 63)))


def chunk(cid, body):
    return cid + struct.pack(">I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def aiff(payload, channels, frames, bits_, rate=16000, ctype=None, cname=b"", offset=0, comm_last=False, before=(), between=(), after=(),
         rate_bytes=None, ssnd=True):
    """An AIFF file (ctype None) or an AIFF-C file with compression type `ctype` (4 bytes) and name `cname`.  offset: SSND's data
    offset (that many filler bytes in front of the samples).  comm_last: COMM behind SSND.  before / between / after: (id, body) chunks
    around the two.  rate_bytes: the 10 bytes of the rate as they stand.  ssnd=False: no SSND chunk."""
    comm = struct.pack(">hIh", channels, frames, bits_) + (ext80(rate) if rate_bytes is None else rate_bytes)
    if ctype is not None:
        comm += ctype + bytes([len(cname)]) + cname
        if not len(cname) & 1:
            comm += b"\0"                                                  # a pstring is padded to an even total length
    parts = [chunk(b"FVER", struct.pack(">I", 0xA2805140))] if ctype is not None else []
    parts += [chunk(*c) for c in before]
    sound = [chunk(b"SSND", struct.pack(">II", offset, 0) + b"\xEE" * offset + bytes(payload))] if ssnd else []
    mid = [chunk(*c) for c in between]
    parts += sound + mid + [chunk(b"COMM", comm)] if comm_last else [chunk(b"COMM", comm)] + mid + sound
    parts += [chunk(*c) for c in after]
    body = (b"AIFF" if ctype is None else b"AIFC") + b"".join(parts)
    return b"FORM" + struct.pack(">I", len(body)) + body


def aiff_header_length(data):
    """Bytes up to and with the last header field in front of the samples: SSND's offset and blockSize words (COMM in front of SSND).
    The `offset` filler bytes behind them are sound data's own padding, no field: a file cut there holds no frame, like one cut at
    its first sample."""
    return data.index(b"SSND") + 16


# ---- AU ----------------------------------------------------------------------------------------------------------------------------
def au(payload, encoding, rate, channels, size=None, annotation=b"", magic=b".snd", offset=None):
    """size None: the payload's length (0xFFFFFFFF: 'to the end of the file').  The annotation is padded to a multiple of 8."""
    note = annotation + bytes(-len(annotation) % 8)
    off = 24 + len(note) if offset is None else offset
    return magic + struct.pack(">IIIII", off, len(payload) if size is None else size, encoding, rate, channels) + note + bytes(payload)


# ---- NIST SPHERE -----------------------------------------------------------------------------------------------------------------
def sphere(payload, fields, hsize=1024):
    """fields: [(key, type letter or '-sN' text, value)] in order; the header is padded with spaces to `hsize` bytes."""
    lines = ["NIST_1A", "%7d" % hsize]
    for key, kind, value in fields:
        kind = "-s%d" % len(str(value)) if kind == "s" else "-" + kind
        lines.append("%s %s %s" % (key, kind, value))
    head = ("\n".join(lines) + "\nend_head\n").encode("ascii")
    assert len(head) <= hsize
    return head + b" " * (hsize - len(head)) + bytes(payload)


def sphere_fields(channels, rate, nbytes, count=None, coding=None, order=None):
    f = [("database_id", "s", "test"), ("channel_count", "i", channels)]
    if count is not None:
        f.append(("sample_count", "i", count))
    f += [("sample_rate", "i", rate), ("sample_n_bytes", "i", nbytes)]
    if order is not None:
        f.append(("sample_byte_format", "s", order))
    if coding is not None:
        f.append(("sample_coding", "s", coding))
    return f + [("sample_sig_bits", "i", 8 * nbytes)]


# ---- every coding of the contract ----------------------------------------------------------------------------------------------------
def g711_case(rng, channels, frames, law):
    codes = rng.integers(0, 256, size=(channels, frames)).astype(np.uint8)
    codes.reshape(-1)[:min(4, codes.size)] = [0, 255, 127, 128][:codes.size]
    ints = W.g711_table(law)[codes]
    return np.ascontiguousarray(codes.T).tobytes(), W.scale(ints), ints


def codings():
    """name -> build(rng, channels, frames) -> (file bytes, expected float32 [channels, frames], twin) with twin = (format tag, bits,
    little-endian payload of the RIFF file that holds the same samples)."""
    out = {}

    def ints(width, wrap, big=True, signed8=True):
        def build(rng, C, n):
            x = int_samples(rng, width, C, n)
            twin = x + 128 if width == 1 else x                        # a RIFF file's 8-bit samples are unsigned
            stored = x if signed8 or width > 1 else x + 128           # 'raw ': the byte is s + 128, as the twin's
            return wrap(int_bytes(stored, width, big), C, n, width), int_scale(x, width), (1, 8 * width, int_bytes(twin, width, False))
        return build

    def floats(width, wrap):
        def build(rng, C, n):
            x = float_samples(rng, width, C, n)
            return wrap(float_bytes(x, width), C, n, width), float_value(x, width), (3, 8 * width, float_bytes(x, width, False))
        return build

    def g711(law, wrap):
        def build(rng, C, n):
            payload, want, pcm = g711_case(rng, C, n, law)
            return wrap(payload, C, n, 1), want, (1, 16, int_bytes(pcm, 2, False))
        return build

    for w in (1, 2, 3, 4):
        out["aiff-%d" % (8 * w)] = ints(w, lambda p, C, n, w: aiff(p, C, n, 8 * w))
    out["aifc-NONE"] = ints(2, lambda p, C, n, w: aiff(p, C, n, 16, ctype=b"NONE", cname=b"not compressed"))
    out["aifc-twos"] = ints(2, lambda p, C, n, w: aiff(p, C, n, 16, ctype=b"twos", cname=b"big-endian"))
    out["aifc-sowt"] = ints(2, lambda p, C, n, w: aiff(p, C, n, 16, ctype=b"sowt", cname=b""), big=False)
    out["aifc-sowt24"] = ints(3, lambda p, C, n, w: aiff(p, C, n, 24, ctype=b"sowt", cname=b""), big=False)
    out["aifc-raw"] = ints(1, lambda p, C, n, w: aiff(p, C, n, 8, ctype=b"raw ", cname=b""), signed8=False)
    out["aifc-in24"] = ints(3, lambda p, C, n, w: aiff(p, C, n, 24, ctype=b"in24", cname=b""))
    out["aifc-in32"] = ints(4, lambda p, C, n, w: aiff(p, C, n, 32, ctype=b"in32", cname=b""))
    out["aifc-fl32"] = floats(4, lambda p, C, n, w: aiff(p, C, n, 32, ctype=b"fl32", cname=b"32-bit floating point"))
    out["aifc-FL32"] = floats(4, lambda p, C, n, w: aiff(p, C, n, 32, ctype=b"FL32", cname=b"Float 32"))
    out["aifc-fl64"] = floats(8, lambda p, C, n, w: aiff(p, C, n, 64, ctype=b"fl64", cname=b"64-bit floating point"))
    out["aifc-FL64"] = floats(8, lambda p, C, n, w: aiff(p, C, n, 64, ctype=b"FL64", cname=b"Float 64"))
    for name, law in (("ulaw", W.ULAW), ("ULAW", W.ULAW), ("alaw", W.ALAW), ("ALAW", W.ALAW)):
        out["aifc-" + name] = g711(law, lambda p, C, n, w, name=name: aiff(p, C, n, 16, ctype=name.encode(), cname=b"CCITT G.711", rate=8000))
    out["au-1"] = g711(W.ULAW, lambda p, C, n, w: au(p, 1, 8000, C))
    out["au-27"] = g711(W.ALAW, lambda p, C, n, w: au(p, 27, 8000, C))
    for enc, w in ((2, 1), (3, 2), (4, 3), (5, 4)):
        out["au-%d" % enc] = ints(w, lambda p, C, n, w, enc=enc: au(p, enc, 16000, C))
    out["au-6"] = floats(4, lambda p, C, n, w: au(p, 6, 16000, C))
    out["au-7"] = floats(8, lambda p, C, n, w: au(p, 7, 16000, C))
    out["sphere-pcm-10"] = ints(2, lambda p, C, n, w: sphere(p, sphere_fields(C, 16000, 2, n, "pcm", "10")))
    out["sphere-pcm-01"] = ints(2, lambda p, C, n, w: sphere(p, sphere_fields(C, 16000, 2, n, "pcm", "01")), big=False)
    out["sphere-pcm-default"] = ints(2, lambda p, C, n, w: sphere(p, sphere_fields(C, 16000, 2, n, None, "10")))
    out["sphere-ulaw"] = g711(W.ULAW, lambda p, C, n, w: sphere(p, sphere_fields(C, 8000, 1, n, "ulaw")))
    out["sphere-mu-law"] = g711(W.ULAW, lambda p, C, n, w: sphere(p, sphere_fields(C, 8000, 1, n, "mu-law", "1")))
    out["sphere-alaw"] = g711(W.ALAW, lambda p, C, n, w: sphere(p, sphere_fields(C, 8000, 1, n, "alaw")))
    return out


def write_twin(path, twin, rate, channels):
    """The RIFF/WAVE file that holds the same samples: twin = (format tag, bits, little-endian interleaved payload)."""
    tag, bits_, payload = twin
    W.write_coded_wav(path, tag, payload, rate, channels, block_align=channels * bits_ // 8, bits=bits_)
