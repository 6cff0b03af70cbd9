"""Writes tests/golden/containers_stdlib.npz from Python's aifc, sunau and audioop, the independent readers the contract of the
big-endian containers (include/p2phd.h, data/containers.py) is held against: small files written by the stdlib WRITERS, and beside each
what the stdlib READER returns for it, as an int32 array [frames, channels].

  aifc   compression NONE at 1 / 2 / 3 / 4 bytes per sample, ulaw, alaw; one or three channels
  sunau  encodings 1 (mu-law), 2, 3, 4, 5 (8 / 16 / 24 / 32-bit integers) and 27 (A-law); one or two channels

Two things sunau does not do are made up for here and nowhere else: its writer takes 1, 2 or 4 channels only (so two stands where aifc
has three), and it neither writes nor decodes A-law -- the encoding-27 file is the writer's mu-law file with the encoding word set to
27, and the reader's bytes (which it returns as they stand) go through audioop.alaw2lin.  Run once where the three modules import
(they left the standard library in Python 3.13): python tools/gen_golden_containers.py"""
import os
import struct
import warnings

import numpy as np

warnings.simplefilter("ignore", DeprecationWarning)
import aifc  # noqa: E402
import audioop  # noqa: E402
import sunau  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 41


def be_ints(raw, width):
    """Big-endian two's-complement samples of `width` bytes -> int32."""
    b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width).astype(np.int64)
    v = np.zeros(len(b), dtype=np.int64)
    for k in range(width):
        v = (v << 8) | b[:, k]
    return (v - ((v >> (8 * width - 1)) << (8 * width))).astype(np.int32)


def be_bytes(ints, width):
    v = np.asarray(ints, dtype=np.int64).reshape(-1) & ((1 << (8 * width)) - 1)
    return np.stack([(v >> (8 * (width - 1 - k))) & 255 for k in range(width)], axis=1).astype(np.uint8).tobytes()


def samples(rng, width, channels):
    lo, hi = -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1
    x = rng.integers(lo, hi + 1, size=(FRAMES, channels), dtype=np.int64)
    x.reshape(-1)[:4] = [lo, hi, -1, 0]
    return x


def main():
    rng = np.random.default_rng(20261021)
    out, tmp = {}, os.path.join(ROOT, "tests", "golden", "_containers_tmp")
    cases = [("aifc_none1", 1, 1), ("aifc_none2", 2, 3), ("aifc_none3", 3, 1), ("aifc_none4", 4, 3), ("aifc_ulaw", 2, 3), ("aifc_alaw", 2, 1),
             ("sunau_1", 2, 2), ("sunau_2", 1, 1), ("sunau_3", 2, 2), ("sunau_4", 3, 1), ("sunau_5", 4, 2), ("sunau_27", 2, 1)]
    for name, width, channels in cases:
        x = samples(rng, width, channels)
        lib, what = name.split("_")
        coded = what in ("ulaw", "alaw", "1", "27")
        if lib == "aifc":
            w = aifc.open(tmp, "wb")
            w.setnchannels(channels), w.setsampwidth(width), w.setframerate(16000)
            if coded:
                w.setcomptype(what.encode(), what.encode())
                w.writeframes(x.astype("<i2").tobytes())                   # (linear samples in native order: audioop codes them)
            else:
                w.writeframes(be_bytes(x, width))
            w.close()
            r = aifc.open(tmp, "rb")
            raw = r.readframes(r.getnframes())
            r.close()
            ints = np.frombuffer(raw, dtype="<i2").astype(np.int32) if coded else be_ints(raw, width)
        else:
            w = sunau.open(tmp, "wb")
            w.setnchannels(channels), w.setsampwidth(width), w.setframerate(8000)
            w.setcomptype("ULAW" if coded else "NONE", "")
            w.writeframes(x.astype("<i2").tobytes() if coded else be_bytes(x, width))
            w.close()
            if what == "27":
                data = bytearray(open(tmp, "rb").read())
                assert struct.unpack(">I", data[12:16])[0] == 1
                data[12:16] = struct.pack(">I", 27)
                open(tmp, "wb").write(data)
            r = sunau.open(tmp, "rb")
            raw = r.readframes(r.getnframes())
            r.close()
            if what == "27":
                raw = audioop.alaw2lin(raw, 2)
            ints = np.frombuffer(raw, dtype="<i2").astype(np.int32) if coded else be_ints(raw, width)
        out["file_" + name] = np.frombuffer(open(tmp, "rb").read(), dtype=np.uint8)
        out["ints_" + name] = ints.reshape(-1, channels)
        assert out["ints_" + name].shape == (FRAMES, channels), name
    os.remove(tmp)
    path = os.path.join(ROOT, "tests", "golden", "containers_stdlib.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
