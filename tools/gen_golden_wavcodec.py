"""Writes tests/golden/wavcodec_audioop.npz from Python's audioop, the independent decoder the coded-WAV contract is held against:
the 2 x 256 G.711 values, and 200 random IMA ADPCM chains (predictor, index, 64 nibbles in time order, the 64 outputs).  audioop's
adpcm2lin takes the high nibble of a byte first, so two nibbles in time order (a, b) are packed as a << 4 | b.  Run once where audioop
imports (it left the standard library in Python 3.13): python tools/gen_golden_wavcodec.py"""
import audioop
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    codes = bytes(range(256))
    ulaw = np.frombuffer(audioop.ulaw2lin(codes, 2), dtype="<i2").astype(np.int16)
    alaw = np.frombuffer(audioop.alaw2lin(codes, 2), dtype="<i2").astype(np.int16)
    rng = np.random.default_rng(20261020)
    chains = 200
    pred = rng.integers(-32768, 32768, size=chains).astype(np.int16)
    index = rng.integers(0, 89, size=chains).astype(np.uint8)
    nibbles = rng.integers(0, 16, size=(chains, 64)).astype(np.uint8)
    # a quarter of the chains lean on one side, so that predictor and index run into their clamps
    nibbles[:25] |= 7
    nibbles[25:50] = (nibbles[25:50] | 7) & 7
    nibbles[50:60] &= 8
    out = np.zeros((chains, 64), dtype=np.int16)
    for k in range(chains):
        packed = bytes((int(a) << 4) | int(b) for a, b in zip(nibbles[k, 0::2], nibbles[k, 1::2]))
        pcm, _ = audioop.adpcm2lin(packed, 2, (int(pred[k]), int(index[k])))
        out[k] = np.frombuffer(pcm, dtype="<i2")
    path = os.path.join(ROOT, "tests", "golden", "wavcodec_audioop.npz")
    np.savez_compressed(path, ulaw=ulaw, alaw=alaw, ima_pred=pred, ima_index=index, ima_nibbles=nibbles, ima_out=out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
