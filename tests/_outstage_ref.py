"""numpy restatement of the output stage of whole-file generation (csrc/pcm.hip: p2phd_pcm_peak, p2phd_pcm_encode_ex), written
from the equations of include/p2phd.h: the peak report (peak / over / nonfinite / gain), the dither hash and the extended
encoder.  tests/test_outstage_host.py holds it to the hash's known answers and to the plain encoder of tests/_pcm_ref.py;
tests/test_gpu_outstage.py holds the kernels to it, bit for bit."""
import numpy as np

BITS = {"pcm16": 16, "pcm24": 24}
M32 = np.uint64(0xFFFFFFFF)


def hi_of(encoding):
    """The largest value the encoding holds, as float32: (2^(bits-1) - 1) / 2^(bits-1); 1 for float32."""
    if encoding == "float32":
        return np.float32(1.0)
    scale = np.float32(2 ** (BITS[encoding] - 1))
    return (scale - np.float32(1)) / scale


def peaks(planar, encoding, ceiling=0.0):
    """planar float32 [channels, frames] -> (peak[C] float32, over[C] int64, nonfinite[C] int64, gain float32)."""
    x = np.asarray(planar, dtype=np.float32)
    C = x.shape[0]
    finite = np.isfinite(x)
    mag = np.where(finite, np.abs(x), np.float32(0)).astype(np.float32)
    peak = mag.max(axis=1) if x.shape[1] else np.zeros(C, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if encoding == "float32":
            clamped = np.abs(x) > np.float32(1)
        else:
            clamped = (x > hi_of(encoding)) | (x < np.float32(-1))
    over = clamped.sum(axis=1).astype(np.int64)
    nonfinite = (~finite).sum(axis=1).astype(np.int64)
    m = np.float32(peak.max())
    c = np.float32(ceiling)
    c = hi_of(encoding) if c <= 0 else c
    gain = c / m if m > c else np.float32(1)                     # one float32 division
    return peak.astype(np.float32), over, nonfinite, np.float32(gain)


def fmix(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def dither_hash(seed, index):
    """uint32 hash h of (seed, index), both 64-bit; `index` may be an array."""
    i = np.asarray(index, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo_s, hi_s = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    inner = fmix((i >> np.uint64(32)) ^ lo_s ^ np.uint64(0x9E3779B9))
    return fmix((i & M32) ^ inner ^ hi_s)


def dither_lsb16(seed, index):
    """d * 2^16 as int64: the low half of h minus its high half."""
    h = dither_hash(seed, index)
    return (h & np.uint64(0xFFFF)).astype(np.int64) - (h >> np.uint64(16)).astype(np.int64)


def dither(seed, index):
    """d as float32, in (-1, 1): exact."""
    return (dither_lsb16(seed, index).astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float32)


def encode_ex(planar, encoding, gain=None, tpdf=False, seed=0, first_index=0):
    """planar float32 [channels, frames] -> interleaved payload bytes.  y = x * gain (None: y = x); integer formats:
    v = y * 2^(bits-1) (+ d), r = rint(v) clamped to the integer range, NaN -> 0; float32: the bits of y."""
    x = np.ascontiguousarray(np.asarray(planar, dtype=np.float32).T)            # [frames, channels]: the interleaved order
    with np.errstate(invalid="ignore", over="ignore"):
        y = x if gain is None else (x * np.float32(gain)).astype(np.float32)
        if encoding == "float32":
            if tpdf:
                raise ValueError("dither is for pcm16 only")
            return y.astype("<f4").tobytes()
        bits = BITS[encoding]
        scale = np.float32(2 ** (bits - 1))
        v = (y * scale).astype(np.float32)
        if tpdf:
            if encoding != "pcm16":
                raise ValueError("dither is for pcm16 only")
            idx = np.uint64(first_index) + np.arange(x.size, dtype=np.uint64)
            v = (v + dither(seed, idx).reshape(x.shape)).astype(np.float32)
        r = np.clip(np.rint(v), -scale, scale - np.float32(1))
    q = np.where(np.isnan(v), np.float32(0), r).astype(np.int32)
    if encoding == "pcm16":
        return q.astype("<i2").tobytes()
    return np.ascontiguousarray(q.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()
