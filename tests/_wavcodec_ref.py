"""Plain Python / numpy restatement of the "Coded WAV input" contract of include/p2phd.h: the two G.711 decoders, the IMA ADPCM
decoder of a WAVE data chunk, simple encoders (G.711 by nearest code, the standard IMA encoder) and writers of coded WAV files.
Nothing here calls the library: the tests compare the library with this, and this with Python's audioop (tests/golden/
wavcodec_audioop.npz, made from audioop once, and audioop itself where it imports)."""
import struct

import numpy as np

TAG_ALAW, TAG_ULAW, TAG_IMA = 6, 7, 0x11
ULAW, ALAW = 0, 1                                                           # P2PHD_G711_ULAW / _ALAW

STEP = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,
        173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,
        1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635,
        13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767]
INDEX_STEP = [-1, -1, -1, -1, 2, 4, 6, 8]
assert len(STEP) == 89


def ulaw_one(b):
    u = ~b & 0xFF
    e, m = (u >> 4) & 7, u & 15
    mag = (((m << 3) + 0x84) << e) - 0x84
    return -mag if u & 0x80 else mag


def alaw_one(b):
    a = b ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
    return mag if a & 0x80 else -mag


ULAW_TABLE = np.array([ulaw_one(b) for b in range(256)], dtype=np.int32)
ALAW_TABLE = np.array([alaw_one(b) for b in range(256)], dtype=np.int32)


def g711_table(law):
    return ALAW_TABLE if law == ALAW else ULAW_TABLE


def scale(ints):
    """int16 values -> what wavio returns for 16-bit PCM: float32(int16) * (1 / 32768)."""
    return np.asarray(ints).astype(np.int16).astype(np.float32) * np.float32(1.0 / 32768.0)


def g711_decode(payload, frames, channels, law):
    """interleaved bytes -> int32 [channels, frames]"""
    b = np.frombuffer(bytes(payload), dtype=np.uint8)[:frames * channels].reshape(frames, channels)
    return np.ascontiguousarray(g711_table(law)[b].T)


def g711_encode(ints, law):
    """int [channels, frames] -> interleaved bytes: for every sample the code whose value is nearest (the lowest such code)."""
    t = g711_table(law).astype(np.int64)
    x = np.asarray(ints, dtype=np.int64)
    codes = np.abs(x[..., None] - t[None, None, :]).argmin(axis=-1).astype(np.uint8)
    return np.ascontiguousarray(codes.T).tobytes()


# ---- IMA ADPCM ---------------------------------------------------------------------------------------------------------------------
def ima_step(pred, index, n):
    st = STEP[index]
    d = st >> 3
    if n & 1:
        d += st >> 2
    if n & 2:
        d += st >> 1
    if n & 4:
        d += st
    pred = pred - d if n & 8 else pred + d
    pred = max(-32768, min(32767, pred))
    index = max(0, min(88, index + INDEX_STEP[n & 7]))
    return pred, index


def ima_chain(pred, index, nibbles):
    """One chain: header values and its nibbles in time order -> the samples behind the header's (the header's predictor is the first
    sample of the block).  The index is clamped to 0 .. 88 on load, as every decoder of the library does."""
    index = min(index, 88)
    out = []
    for n in nibbles:
        pred, index = ima_step(pred, index, n)
        out.append(pred)
    return out


def ima_spb(channels, block_align):
    c4 = 4 * channels
    if channels < 1 or block_align < 2 * c4 or (block_align - c4) % c4:
        return None
    return 1 + 8 * ((block_align - c4) // c4)


def ima_frames(nbytes, channels, block_align):
    spb, c4 = ima_spb(channels, block_align), 4 * channels
    full, rest = divmod(nbytes, block_align)
    return full * spb + (1 + 8 * (rest // c4 - 1) if rest >= c4 else 0)


def ima_decode(payload, channels, block_align, frames=None):
    """A data chunk's bytes -> int32 [channels, frames] (default: every frame the bytes hold)."""
    data = bytes(payload)
    C, c4 = channels, 4 * channels
    spb = ima_spb(C, block_align)
    total = ima_frames(len(data), C, block_align)
    frames = total if frames is None else frames
    assert 0 <= frames <= total
    out = np.zeros((C, total), dtype=np.int32)
    for B in range(-(-len(data) // block_align)):
        blk = data[B * block_align:(B + 1) * block_align]
        if len(blk) < c4:
            break
        groups = len(blk) // c4 - 1
        for c in range(C):
            pred, index = struct.unpack("<hB", blk[4 * c:4 * c + 3])
            nibbles = []
            for g in range(groups):
                for byte in blk[c4 * (g + 1) + 4 * c:c4 * (g + 1) + 4 * c + 4]:
                    nibbles += [byte & 15, byte >> 4]                       # the low nibble comes first
            out[c, B * spb] = pred
            out[c, B * spb + 1:B * spb + 1 + 8 * groups] = ima_chain(pred, index, nibbles)
    return np.ascontiguousarray(out[:, :frames])


def ima_encode_nibble(sample, pred, index):
    """The standard IMA encoder's step: -> (nibble, pred, index) with the decoder's own reconstruction."""
    st = STEP[index]
    diff = sample - pred
    n = 0
    if diff < 0:
        n, diff = 8, -diff
    if diff >= st:
        n |= 4
        diff -= st
    if diff >= st >> 1:
        n |= 2
        diff -= st >> 1
    if diff >= st >> 2:
        n |= 1
    pred, index = ima_step(pred, index, n)
    return n, pred, index


def ima_encode(ints, block_align, partial=True):
    """int [channels, frames] -> the data chunk's bytes.  Every block's header takes the block's first sample as the predictor; the
    index runs on from block to block.  A tail that does not fill a block is zero-padded to whole groups (`partial`: and written as a
    partial block of 1 + 8k samples' worth; else padded to a whole block)."""
    x = np.asarray(ints, dtype=np.int64)
    C, L = x.shape
    spb = ima_spb(C, block_align)
    out = bytearray()
    index = [0] * C
    for n0 in range(0, L, spb):
        seg = x[:, n0:n0 + spb]
        have = seg.shape[1]
        groups = (spb - 1) // 8 if (have == spb or not partial) else -(-(have - 1) // 8)
        seg = np.concatenate([seg, np.repeat(seg[:, -1:], 1 + 8 * groups - have, axis=1)], axis=1)
        words = [[] for _ in range(C)]
        for c in range(C):
            pred = int(seg[c, 0])
            out += struct.pack("<hBB", pred, index[c], 0)
            for g in range(groups):
                w = 0
                for k in range(8):
                    n, pred, index[c] = ima_encode_nibble(int(seg[c, 1 + 8 * g + k]), pred, index[c])
                    w |= n << (4 * k)
                words[c].append(struct.pack("<I", w))
        for g in range(groups):
            for c in range(C):
                out += words[c][g]
    return bytes(out)


# ---- writers -----------------------------------------------------------------------------------------------------------------------
def write_coded_wav(path, tag, payload, rate, channels, block_align=None, bits=None, fact=None, extensible=False, samples_per_block=None,
                    data_size=None, cb_size=None):
    """A RIFF/WAVE file around `payload`.  fact: None (no fact chunk) or the sample length to state.  extensible: WAVE_FORMAT_EXTENSIBLE
    with the tag in the sub-format.  samples_per_block: the value of the fmt extension (IMA; default: what block_align holds; False:
    no extension).  bits / block_align / data_size override what would be right, for the refusals."""
    C = channels
    if block_align is None:
        block_align = C
    if bits is None:
        bits = 4 if tag == TAG_IMA else 8
    if tag == TAG_IMA:
        spb = ima_spb(C, block_align) if samples_per_block is None else samples_per_block
        byte_rate = rate * block_align // (spb or 1)
    else:
        spb, byte_rate = False, rate * block_align
    if extensible:
        ext = struct.pack("<HHI", 22, spb or 0, 0) + struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xAA\x00\x38\x9B\x71"
        fmt = struct.pack("<HHIIHH", 0xFFFE, C, rate, byte_rate, block_align, bits) + ext
    elif spb is not False:
        fmt = struct.pack("<HHIIHH", tag, C, rate, byte_rate, block_align, bits) + struct.pack("<HH", 2 if cb_size is None else cb_size, spb)
    else:
        fmt = struct.pack("<HHIIHH", tag, C, rate, byte_rate, block_align, bits) + struct.pack("<H", 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if fact is not None:
        body += b"fact" + struct.pack("<II", 4, fact)
    payload = bytes(payload)
    body += b"data" + struct.pack("<I", len(payload) if data_size is None else data_size) + payload + (b"\0" if len(payload) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def write_pcm16_wav(path, ints, rate):
    """The PCM16 twin: int [channels, frames] as a plain 44-byte-header WAVE file."""
    x = np.asarray(ints).astype("<i2")
    C = x.shape[0]
    payload = np.ascontiguousarray(x.T).tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, C, rate, rate * 2 * C, 2 * C, 16))
        f.write(b"data" + struct.pack("<I", len(payload)) + payload)


def speech_like(channels, frames, seed=0, amp=9000.0):
    """A deterministic band-limited test signal, int64 [channels, frames] inside int16."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    x = np.zeros((channels, frames))
    for c in range(channels):
        for k in range(5):
            x[c] += rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * rng.uniform(0.002, 0.2) * t + rng.uniform(0, 6.28))
        x[c] += 0.05 * rng.standard_normal(frames)
    return np.clip(np.rint(x * amp / 3.0), -32768, 32767).astype(np.int64)
