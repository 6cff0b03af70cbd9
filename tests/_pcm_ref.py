"""numpy restatement of the PCM codec (csrc/pcm.hip) and the payloads its tests run on.  tests/test_pcm_host.py ties the
restatement to data/wavio.py as it stands; tests/test_gpu_pcm.py holds the kernels to both."""
import struct

import numpy as np

# name -> (format tag, bits, P2PHD_PCM_* code)
FORMATS = {"u8": (1, 8, 0), "s16": (1, 16, 1), "s24": (1, 24, 2), "s32": (1, 32, 3), "f32": (3, 32, 4), "f64": (3, 64, 5)}
ENCODINGS = {"pcm16": (1, 16, 1), "pcm24": (1, 24, 2), "float32": (3, 32, 4)}


def decode(payload, channels, name):
    """interleaved little-endian bytes -> planar float32 [channels, frames]; written independently of wavio.load."""
    tag, bits, _ = FORMATS[name]
    raw = np.frombuffer(bytes(payload), dtype=np.uint8)
    if name == "u8":
        a = (raw.astype(np.int32) - 128).astype(np.float32) / np.float32(128)
    elif name == "s16":
        a = raw.view("<i2").astype(np.float32) / np.float32(32768)
    elif name == "s24":
        b = raw.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] + 256 * b[:, 1] + 65536 * b[:, 2]
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        a = v.astype(np.float32) / np.float32(8388608)
    elif name == "s32":
        a = raw.view("<i4").astype(np.float32) / np.float32(2147483648)
    elif name == "f32":
        a = raw.view("<f4").copy()
    else:
        with np.errstate(over="ignore"):
            a = raw.view("<f8").astype(np.float32)
    return np.ascontiguousarray(a.reshape(-1, channels).T)


def encode(planar, name):
    """planar float32 [channels, frames] -> interleaved payload bytes.  Integer formats: NaN -> 0, clamp to
    [-1, 1 - 2^-(bits-1)], times 2^(bits-1), round half to even."""
    x = np.ascontiguousarray(np.asarray(planar, dtype=np.float32).T)            # [frames, channels]
    if name == "float32":
        return x.astype("<f4").tobytes()
    bits = ENCODINGS[name][1]
    scale = np.float32(2 ** (bits - 1))
    y = np.where(np.isnan(x), np.float32(0), x)
    y = np.clip(y, np.float32(-1), (scale - np.float32(1)) / scale).astype(np.float32) * scale
    q = np.rint(y).astype(np.int32)
    if name == "pcm16":
        return q.astype("<i2").tobytes()
    return np.ascontiguousarray(q.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()


def payload(name, frames, channels, seed=0):
    """Test payload of frames * channels samples: the extremes of the type first (integer: min, max, -1, 0, 1 ...; float: +-0,
    denormals, +-inf, +-max, values that round either way to float32), random bytes behind.  NaN only for f32."""
    rng = np.random.default_rng(seed + 17 * frames + channels)
    n = frames * channels
    if name == "u8":
        special = np.array([0, 255, 127, 128, 129, 1], dtype=np.uint8)
        body = rng.integers(0, 256, n, dtype=np.uint8)
    elif name == "s16":
        special = np.array([-32768, 32767, -1, 0, 1, -32767], dtype="<i2")
        body = rng.integers(-32768, 32768, n).astype("<i2")
    elif name == "s24":
        v = np.concatenate([np.array([-(1 << 23), (1 << 23) - 1, -1, 0, 1, -(1 << 23) + 1]), rng.integers(-(1 << 23), 1 << 23, n)])[:n]
        return np.ascontiguousarray(v.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3]).tobytes()
    elif name == "s32":
        # 2^24 + 1 and 2^25 + 2 are ties of the int -> float conversion; 2^31 - 1 rounds up to 2^31
        special = np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1, (1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, -(1 << 24) - 1],
                           dtype="<i4")
        body = rng.integers(-(1 << 31), 1 << 31, n).astype("<i4")
    elif name == "f32":
        special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7FC00000,
                            0xFFC12345, 0x7F800001, 0x3F800000], dtype="<u4").view("<f4")
        body = rng.standard_normal(n).astype("<f4")
    else:
        tiny32 = float(np.float32(1e-45))                                       # the smallest float32 denormal
        special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, np.inf, -np.inf, 1.7976931348623157e308,
                            tiny32, -tiny32, tiny32 / 2, tiny32 * 0.75, tiny32 * 1.5, 1e-40, -1e-40, 3.4028235677973366e38,
                            1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, 1.0 - 2.0 ** -25], dtype="<f8")
        body = rng.standard_normal(n).astype("<f8")
    v = np.concatenate([special, body])[:n] if n else body[:0]
    return v.tobytes()


def encode_input(frames, channels, seed=0):
    """planar float32 [channels, frames] for the encoders: every (k + 1/2) / 32768 tie around 0 and at both ends, the 24-bit
    ties, +-1, +-(1 + 2^-20), the upper clamp values, +-inf, denormals, +-0, random values inside and outside [-1, 1].  No NaN."""
    rng = np.random.default_rng(seed + 31 * frames + channels)
    k = np.concatenate([np.arange(-40, 40), np.arange(-32770, -32730), np.arange(32730, 32770)]).astype(np.float64)
    k24 = np.concatenate([np.arange(-20, 20), np.arange(-(1 << 23) - 3, -(1 << 23) + 20), np.arange((1 << 23) - 20, (1 << 23) + 3)]).astype(np.float64)
    special = np.concatenate([
        (k + 0.5) / 32768.0, k / 32768.0, (k24 + 0.5) / 8388608.0,
        [1.0, -1.0, 1.0 + 2.0 ** -20, -(1.0 + 2.0 ** -20), 32767.0 / 32768.0, 8388607.0 / 8388608.0, np.inf, -np.inf, 0.0, -0.0,
         1e-45, -1e-45, 1e-40, 1.1754942e-38, 3.4028235e38, -3.4028235e38]]).astype(np.float32)
    n = frames * channels
    body = np.concatenate([rng.uniform(-1.0, 1.0, n), rng.standard_normal(n) * 2.0]).astype(np.float32)
    v = np.concatenate([special, body])
    if n > len(special):
        v = np.concatenate([special, rng.permutation(body)[:n - len(special)]])
    return np.ascontiguousarray(v[:n].reshape(frames, channels).T)


def quantise_edges(bits):
    """float32 values at which the order of clamping and rounding could matter for `bits` (16: every code, 24: every 251st):
    each code boundary k / 2^(bits-1) and half-way point (k + 1/2) / 2^(bits-1) with its neighbours 1 ulp either side, the
    +-1030 codes around -2^(bits-1), 0 and 2^(bits-1) - 1 the same way, and every exponent with mantissa 0, 1, 0x400000 and
    all-ones, both signs (denormals, +-inf and NaNs with payloads among them)."""
    half = 1 << (bits - 1)
    near = np.arange(-1030, 1031)
    k = np.unique(np.concatenate([np.arange(-half, half, 1 if bits == 16 else 251), near - half, near, near + half - 1])).astype(np.float64)
    points = (np.concatenate([k, k + 0.5]) / half).astype(np.float32)
    grid = np.concatenate([points, np.nextafter(points, np.float32(4)), np.nextafter(points, np.float32(-4))])
    pattern = ((np.arange(256, dtype=np.uint32) << 23)[:, None] | np.array([0, 1, 0x400000, 0x7FFFFF], dtype=np.uint32)[None, :]).ravel()
    return np.concatenate([grid, np.concatenate([pattern, pattern | np.uint32(0x80000000)]).astype("<u4").view("<f4")])


def wav_bytes(payload_bytes, rate, channels, name, extensible=False):
    """A RIFF/WAVE file image around a payload; `extensible`: the 40-byte WAVE_FORMAT_EXTENSIBLE fmt chunk."""
    tag, bits, _ = FORMATS[name]
    align = channels * bits // 8
    if extensible:
        guid = struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * align, align, bits) + struct.pack("<HHI", 22, bits, 0) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload_bytes)) + payload_bytes
    if len(payload_bytes) & 1:
        body += b"\0"
    return b"RIFF" + struct.pack("<I", len(body)) + body
