"""A numpy float64 restatement of the album loudness of csrc/loudness.hip (EBU R 128: a folder as one programme), built on
tests/_loudness_ref.py: every file's own 400 ms blocks, one behind the other, and both gates over the union of them."""
import numpy as np

import _loudness_ref as R

# the hand-made album of the tests, 48 kHz (hop 4800): per file the single-hop levels in LUFS, one tuple per channel
ALBUM_LEVELS = (((-20.0,) * 40,), ((-45.0,) * 30,), ((-30.0,) * 3,),
                (tuple(np.linspace(-30.0, -18.0, 12)), (-26.0,) * 12), ((-80.0,) * 9,))
ALBUM_BLOCKS = (37, 27, 0, 9, 6)


def hand_made_album(hop=4800):
    """-> the list of z [C, J], one per file of ALBUM_LEVELS."""
    return [np.stack([R.hops_at_level(row, hop) for row in rows]) for rows in ALBUM_LEVELS]


def album_blocks(zs, rate, weights=None):
    """zs: a list of z [C, J], one per file; weights: None, or a list with one entry (None or a sequence) per file -> the block
    powers of all files, one file's behind the other's (R.gating's 'p': a block never spans two files)."""
    weights = [None] * len(zs) if weights is None else weights
    parts = [R.gating(z, rate, w)['p'] for z, w in zip(zs, weights)]
    return np.concatenate(parts) if parts else np.zeros(0)


def album_gating(p):
    """p [NB] -> {'I', 'max', 'gamma', 'kept', 'l'}: the absolute gate at -70 LUFS, the relative one 10 LU under the mean of what
    passed; a block whose level is NaN stays in, as in R.gating."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    ninf = float('-inf')
    if p.size == 0:
        return {'I': ninf, 'max': ninf, 'gamma': ninf, 'kept': 0, 'l': np.zeros(0)}
    with np.errstate(invalid='ignore', over='ignore'):
        l = R._lufs(p)
        top = float(np.fmax.reduce(np.concatenate([[ninf], l])))
        A = ~(l <= -70.0)
        if not A.any():
            return {'I': ninf, 'max': top, 'gamma': ninf, 'kept': 0, 'l': l}
        gamma = float(R._lufs(p[A].mean())) - 10.0
        B = A & ~(l <= gamma)
        I = float(R._lufs(p[B].mean())) if B.any() else ninf
    return {'I': I, 'max': top, 'gamma': gamma, 'kept': int(B.sum()), 'l': l}
