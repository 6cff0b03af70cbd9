"""A restatement of the FLAC subset the library reads (RFC 9639), in plain Python: a bit writer, an encoder that emits every
construct on demand, a straightforward decoder, the two CRCs and the MD5.  It shares no code with the library; the tests of the
FLAC reader take their fixtures and their expected samples from here.  Pure-Python Rice coding is slow: keep fixtures small.

Its own checks (run by tests/test_flac_host.py::test_restatement): the CRC anchors, the RFC's one-frame example, and
encode -> decode identity."""
import hashlib
import struct

RFC_FRAME = bytes.fromhex("fff869180000bf0358fd03128baa9a")        # block size 1, 44.1 kHz, 2 x 16 bit: left 25588, right 10416

INDEPENDENT, LEFT_SIDE, SIDE_RIGHT, MID_SIDE = 0, 8, 9, 10

BLOCK_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
BITS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def crc16(data):
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
    return c


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def u(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0 and value == 0, (value, bits)
        self.v = (self.v << bits) | value
        self.n += bits

    def s(self, value, bits):
        assert bits == 0 and value == 0 or -(1 << (bits - 1)) <= value < (1 << (bits - 1)), (value, bits)
        self.u(value & ((1 << bits) - 1), bits)

    def unary(self, q):
        self.u(1, q + 1)

    def align(self):
        self.u(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


class BitReader:
    def __init__(self, data):
        self.v, self.total, self.pos = int.from_bytes(data, "big"), 8 * len(data), 0

    def u(self, bits):
        if self.pos + bits > self.total:
            raise ValueError("out of bits")
        self.pos += bits
        return (self.v >> (self.total - self.pos)) & ((1 << bits) - 1)

    def s(self, bits):
        v = self.u(bits)
        return v - (1 << bits) if bits and v >> (bits - 1) else v

    def unary(self):
        q = 0
        while self.u(1) == 0:
            q += 1
        return q


def coded_number(v):
    """The UTF-8-like coding of a frame or sample number: 1 to 7 bytes."""
    if v < 0x80:
        return bytes([v])
    for n, lim in ((2, 11), (3, 16), (4, 21), (5, 26), (6, 31), (7, 36)):
        if v < (1 << lim):
            out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
            for i in range(n - 2, -1, -1):
                out.append(0x80 | ((v >> (6 * i)) & 0x3F))
            return bytes(out)
    raise ValueError(v)


def zigzag(r):
    return (r << 1) if r >= 0 else ((-r) << 1) - 1


def best_rice(res, limit):
    if not res:
        return 0
    best, bits = 0, None
    for k in range(0, limit):
        b = sum((zigzag(r) >> k) + 1 + k for r in res)
        if bits is None or b < bits:
            best, bits = k, b
    return best


def predict(coefs, shift, hist):
    """hist: the samples so far; coefs[0] multiplies the newest."""
    return sum(c * hist[-1 - i] for i, c in enumerate(coefs)) >> max(shift, 0)     # (a negative shift is only ever written, for the refusal)


def write_subframe(w, samples, bps, kind="verbatim", order=0, coefs=None, precision=None, shift=0, wasted=0, method=0, porder=0,
                   params=None, escapes=None, type_bits=None, shift_field=None, method_field=None, pad_bit=0):
    """samples: the channel's integers of `bps` bits.  kind 'constant' | 'verbatim' | 'fixed' | 'lpc'.  wasted: low zero bits that
    are taken out (the samples must have them).  method 0 / 1: 4- / 5-bit Rice parameters; params: one per partition (None: the
    cheapest); escapes: {partition: raw width} (None for a width: the smallest that holds the partition).  type_bits,
    shift_field, method_field, pad_bit: raw fields for the refusal cases."""
    bs = len(samples)
    if wasted:
        assert all(s % (1 << wasted) == 0 for s in samples)
        samples = [s >> wasted for s in samples]
        bps -= wasted
    if kind == "constant":
        t = 0
    elif kind == "verbatim":
        t = 1
    elif kind == "fixed":
        t = 8 | order
        coefs = FIXED[order]
    else:
        order = len(coefs)
        t = 32 | (order - 1)
    w.u(pad_bit, 1)
    w.u(t if type_bits is None else type_bits, 6)
    w.u(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
    if kind == "constant":
        assert all(s == samples[0] for s in samples)
        w.s(samples[0], bps)
        return
    if kind == "verbatim":
        for s in samples:
            w.s(s, bps)
        return
    for s in samples[:order]:
        w.s(s, bps)
    if kind == "lpc":
        w.u(precision - 1, 4)
        w.u((shift & 31) if shift_field is None else shift_field, 5)
        for c in coefs:
            w.s(c, precision)
    res = [samples[n] - predict(coefs, shift, samples[n - order:n]) for n in range(order, bs)]
    w.u(method if method_field is None else method_field, 2)
    w.u(porder, 4)
    pbits = 5 if method else 4
    parts = 1 << porder
    assert bs % parts == 0 and bs >> porder >= order
    at = 0
    for p in range(parts):
        count = (bs >> porder) - (order if p == 0 else 0)
        part = res[at:at + count]
        at += count
        if escapes and p in escapes:
            width = escapes[p]
            if width is None:
                width = max([0] + [(r if r >= 0 else ~r).bit_length() + 1 for r in part if r])
            w.u((1 << pbits) - 1, pbits)
            w.u(width, 5)
            for r in part:
                w.s(r, width)
            continue
        k = best_rice(part, (1 << pbits) - 1) if params is None else params[p]
        w.u(k, pbits)
        for r in part:
            z = zigzag(r)
            w.unary(z >> k)
            w.u(z & ((1 << k) - 1), k)


def frame_header(bs, rate, assign, bits, number, variable=False, bs_code=None, rate_code=None, bits_code=None, reserved1=0, reserved2=0):
    """bs_code / rate_code / bits_code: None picks the table code where there is one; 6 / 7 force the 8- / 16-bit block-size
    trailer, 12 / 13 / 14 the rate trailers, 0 'from STREAMINFO'."""
    if bs_code is None:
        bs_code = BLOCK_CODES.get(bs, 6 if bs <= 256 else 7)
    if rate_code is None:
        rate_code = RATE_CODES.get(rate, 13 if rate < 65536 else 14 if rate % 10 == 0 else 0)
    if bits_code is None:
        bits_code = BITS_CODES[bits]
    h = bytearray([0xFF, 0xF8 | (reserved1 << 1) | (1 if variable else 0), (bs_code << 4) | rate_code, (assign << 4) | (bits_code << 1) | reserved2])
    h += coded_number(number)
    if bs_code == 6:
        h.append(bs - 1)
    elif bs_code == 7:
        h += struct.pack(">H", bs - 1)
    if rate_code == 12:
        h.append(rate // 1000)
    elif rate_code == 13:
        h += struct.pack(">H", rate)
    elif rate_code == 14:
        h += struct.pack(">H", rate // 10)
    h.append(crc8(h))
    return bytes(h)


def side_bit(assign, c):
    return 1 if (assign, c) in ((LEFT_SIDE, 1), (SIDE_RIGHT, 0), (MID_SIDE, 1)) else 0


def decorrelate(left, right, assign):
    """left / right -> the two coded channels of `assign`."""
    if assign == LEFT_SIDE:
        return [left, [a - b for a, b in zip(left, right)]]
    if assign == SIDE_RIGHT:
        return [[a - b for a, b in zip(left, right)], right]
    if assign == MID_SIDE:
        return [[(a + b) >> 1 for a, b in zip(left, right)], [a - b for a, b in zip(left, right)]]
    return [left, right]


def encode_frame(channels, bits, number, rate=44100, variable=False, assign=None, specs=None, cut=0, **header):
    """channels: the samples per channel as they are heard (decorrelated here for assign 8 / 9 / 10).  specs: one dict of
    write_subframe's options per coded channel (None: verbatim).  cut: drop this many bytes from the end of the subframes and
    re-seal the frame with a correct CRC-16 (the bounded-read case)."""
    nch = len(channels)
    if assign is None:
        assign = nch - 1
    coded = decorrelate(channels[0], channels[1], assign) if assign >= 8 else channels
    bs = len(channels[0])
    w = BitWriter()
    for c, ch in enumerate(coded):
        write_subframe(w, list(ch), bits + side_bit(assign, c), **((specs[c] if specs else None) or {}))
    w.align()
    body = w.bytes()
    if cut:
        body = body[:-cut]
    f = frame_header(bs, rate, assign, bits, number, variable, **header) + body
    return f + struct.pack(">H", crc16(f))


def md5_of(channels, bits):
    """MD5 of the interleaved samples, little-endian, in ceil(bits / 8) bytes each."""
    nb = (bits + 7) // 8
    h = hashlib.md5()
    h.update(b"".join((channels[c][n] & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little") for n in range(len(channels[0])) for c in range(len(channels))))
    return h.digest()


def metadata_block(kind, payload, last=False):
    return bytes([(0x80 if last else 0) | kind]) + len(payload).to_bytes(3, "big") + payload


def streaminfo(rate, channels, bits, total, min_block, max_block, md5=b"\0" * 16, min_frame=0, max_frame=0):
    v = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total
    return struct.pack(">HH", min_block, max_block) + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big") + v.to_bytes(8, "big") + md5


def id3v2(size=37, footer=False):
    ss = bytes([(size >> 21) & 0x7F, (size >> 14) & 0x7F, (size >> 7) & 0x7F, size & 0x7F])
    return b"ID3\x04\x00" + bytes([0x10 if footer else 0]) + ss + bytes((7 * i + 3) & 0x7F for i in range(size)) + (b"3DI\x04\x00\x10" + ss if footer else b"")


def every_metadata_kind():
    """PADDING, APPLICATION, SEEKTABLE (3 points), VORBIS_COMMENT, CUESHEET (opaque), PICTURE (opaque) and an unknown type 42."""
    seek = b"".join(struct.pack(">QQH", 4096 * i, 100 * i, 4096) for i in range(3))
    return [(1, b"\0" * 9), (2, b"test" + b"\x01\x02\x03"), (3, seek), (4, struct.pack("<I", 3) + b"ref" + struct.pack("<I", 0)),
            (5, b"\0" * 40), (6, b"\0" * 32), (42, b"unknown block \xff\xf8 with a sync code")]


def encode_stream(frames, rate, channels, bits, total, min_block, max_block, md5=None, blocks=(), id3=None, marker=b"fLaC"):
    """frames: the encoded frames.  blocks: (type, payload) metadata behind STREAMINFO.  id3: None, or a tag (id3v2()) in front."""
    out = bytearray(id3 or b"") + marker
    out += metadata_block(0, streaminfo(rate, channels, bits, total, min_block, max_block, md5 or b"\0" * 16), last=not blocks)
    for i, (kind, payload) in enumerate(blocks):
        out += metadata_block(kind, payload, last=i == len(blocks) - 1)
    for f in frames:
        out += f
    return bytes(out)


def make_stream(channels, bits, block, rate=44100, assign=None, specs=None, variable=False, sizes=None, first_number=0, with_md5=True,
                total=None, blocks=(), id3=None, **header):
    """channels [C][T] -> (the stream's bytes, the frames' bytes).  Frames of `block` samples (the last shorter), or of `sizes`
    (variable block size).  specs: per coded channel, or a callable (frame index, channel) -> dict.  first_number: the first
    frame's number (fixed) or sample number (variable)."""
    T = len(channels[0])
    if sizes is None:
        sizes = [min(block, T - a) for a in range(0, T, block)]
    frames, at = [], 0
    for k, bs in enumerate(sizes):
        chunk = [ch[at:at + bs] for ch in channels]
        nch = 2 if (assign or 0) >= 8 else len(channels)
        sp = [specs(k, c) for c in range(nch)] if callable(specs) else specs
        number = first_number + at if variable else first_number + k
        frames.append(encode_frame(chunk, bits, number, rate, variable, assign, sp, **header))
        at += bs
    assert at == T
    data = encode_stream(frames, rate, len(channels), bits, T if total is None else total, max(min(sizes[:-1] or sizes), 16), max(sizes + [16]),
                         md5_of(channels, bits) if with_md5 else None, blocks, id3)
    return data, frames


# ---- decoder -------------------------------------------------------------------------------------------------------------
def read_subframe(r, bs, bps):
    if r.u(1):
        raise ValueError("padding bit")
    t = r.u(6)
    wasted = 0
    if r.u(1):
        wasted = r.unary() + 1
        bps -= wasted
    if t == 0:
        out = [r.s(bps)] * bs
    elif t == 1:
        out = [r.s(bps) for _ in range(bs)]
    else:
        if t & 32:
            order = (t & 31) + 1
        elif t & 0x38 == 8 and (t & 7) <= 4:
            order = t & 7
        else:
            raise ValueError("reserved subframe type")
        out = [r.s(bps) for _ in range(order)]
        shift = 0
        if t & 32:
            precision = r.u(4) + 1
            if precision == 16:
                raise ValueError("reserved precision")
            shift = r.s(5)
            if shift < 0:
                raise ValueError("negative shift")
            coefs = [r.s(precision) for _ in range(order)]
        else:
            coefs = FIXED[order]
        method = r.u(2)
        if method > 1:
            raise ValueError("reserved residual method")
        pbits = 5 if method else 4
        porder = r.u(4)
        for p in range(1 << porder):
            count = (bs >> porder) - (order if p == 0 else 0)
            k = r.u(pbits)
            if k == (1 << pbits) - 1:
                width = r.u(5)
                res = [r.s(width) for _ in range(count)]
            else:
                res = []
                for _ in range(count):
                    z = (r.unary() << k) | r.u(k)
                    res.append((z >> 1) if z & 1 == 0 else -((z + 1) >> 1))
            for e in res:
                out.append(e + predict(coefs, shift, out))
    return [s << wasted for s in out]


def decode_frame(data, si_rate=44100, si_bits=16):
    """One frame at the start of `data` -> (channels as heard, its length in bytes, header dict)."""
    r = BitReader(data)
    if r.u(14) != 0x3FFE or r.u(1):
        raise ValueError("sync")
    variable = r.u(1)
    bs_code, rate_code, assign, bits_code = r.u(4), r.u(4), r.u(4), r.u(3)
    r.u(1)
    lead = r.u(8)
    n = 0
    while lead & (0x80 >> n):
        n += 1
    number = lead & (0xFF >> (n + 1)) if n else lead
    for _ in range(max(n - 1, 0)):
        number = (number << 6) | (r.u(8) & 0x3F)
    inv = {v: k for k, v in BLOCK_CODES.items()}
    bs = r.u(8) + 1 if bs_code == 6 else r.u(16) + 1 if bs_code == 7 else inv[bs_code]
    rinv = {v: k for k, v in RATE_CODES.items()}
    rate = si_rate if rate_code == 0 else r.u(8) * 1000 if rate_code == 12 else r.u(16) if rate_code == 13 else r.u(16) * 10 if rate_code == 14 else rinv[rate_code]
    bits = si_bits if bits_code == 0 else {v: k for k, v in BITS_CODES.items()}[bits_code]
    hlen = r.pos // 8
    if crc8(data[:hlen]) != r.u(8):
        raise ValueError("CRC-8")
    nch = assign + 1 if assign < 8 else 2
    ch = [read_subframe(r, bs, bits + side_bit(assign, c)) for c in range(nch)]
    r.u(-r.pos % 8)
    length = r.pos // 8 + 2
    if crc16(data[:length - 2]) != r.u(16):
        raise ValueError("CRC-16")
    if assign == LEFT_SIDE:
        ch = [ch[0], [a - b for a, b in zip(*ch)]]
    elif assign == SIDE_RIGHT:
        ch = [[a + b for a, b in zip(*ch)], ch[1]]
    elif assign == MID_SIDE:
        mid = [(m << 1) | (s & 1) for m, s in zip(*ch)]
        ch = [[(m + s) >> 1 for m, s in zip(mid, ch[1])], [(m - s) >> 1 for m, s in zip(mid, ch[1])]]
    return ch, length, {"block": bs, "rate": rate, "bits": bits, "assign": assign, "number": number, "variable": variable}


def decode_stream(data):
    """-> (info dict, channels [C][T])."""
    at = 0
    if data[:3] == b"ID3":
        at = 10 + ((data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9]) + (10 if data[5] & 0x10 else 0)
    if data[at:at + 4] != b"fLaC":
        raise ValueError("marker")
    at += 4
    info = None
    while True:
        last, kind, n = data[at] >> 7, data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        body = data[at + 4:at + 4 + n]
        at += 4 + n
        if kind == 0:
            v = int.from_bytes(body[10:18], "big")
            info = {"rate": v >> 44, "channels": ((v >> 41) & 7) + 1, "bits": ((v >> 36) & 31) + 1, "total": v & ((1 << 36) - 1), "md5": body[18:34]}
        if last:
            break
    out = [[] for _ in range(info["channels"])]
    while at < len(data):
        ch, n, _ = decode_frame(data[at:], info["rate"], info["bits"])
        for c in range(info["channels"]):
            out[c] += ch[c]
        at += n
    return info, out


def self_check():
    assert crc8(b"123456789") == 0xF4 and crc16(b"123456789") == 0xFEE8
    ch, n, h = decode_frame(RFC_FRAME)
    assert (ch, n, h["block"], h["rate"], h["bits"]) == ([[25588], [10416]], len(RFC_FRAME), 1, 44100, 16)
    assert encode_frame([[25588], [10416]], 16, 0, specs=[{"wasted": 2}, {"wasted": 4}], bs_code=6) == RFC_FRAME
