"""A numpy restatement of segment_norm's encode (p2phd_spectro_encode_rows, csrc/spectro.hip): the statistics of every row of a
batch on its own, and the encode of tests/_norm_scope_ref.py applied row by row under them, a range of zero scaling by 0.  Like
that module it states the premise and is no bit-for-bit model of the kernels: log10 is numpy's."""
import numpy as np

import _norm_scope_ref as NR

F32 = np.float32


def row_stats(spec, noise=None, alpha=0.6, min_value=1e-7, channels=2):
    """spec [B, F, M], noise [B, channels, mask_rows, F] or None -> norm_rows [B, 8]: (min, max, 0, 0, noise min, noise max, 0, 0)
    per row, the dB values over all M bins and both channels, NaN entries passed over, (+inf, -inf) without noise."""
    spec = np.asarray(spec, dtype=F32)
    B = spec.shape[0]
    out = np.zeros((B, 8), dtype=F32)
    out[:, 4], out[:, 5] = np.inf, -np.inf
    for b in range(B):
        db = NR.db_encode(spec[b:b + 1], alpha, min_value, channels)
        with np.errstate(invalid='ignore'):
            out[b, 0] = np.fmin.reduce(db, axis=None, initial=np.inf)
            out[b, 1] = np.fmax.reduce(db, axis=None, initial=-np.inf)
            if noise is not None and noise[b].size:
                out[b, 4] = np.fmin.reduce(np.asarray(noise[b], dtype=F32), axis=None, initial=np.inf)
                out[b, 5] = np.fmax.reduce(np.asarray(noise[b], dtype=F32), axis=None, initial=-np.inf)
    return out


def encode_rows(spec, alpha=0.6, min_value=1e-7, channels=2):
    """spec [B, F, M] -> (log_spectro [B, channels, M, F], norm_rows [B, 8]): every row under its own range."""
    spec = np.asarray(spec, dtype=F32)
    table = row_stats(spec, None, alpha, min_value, channels)
    rows = [NR.normalise(NR.db_encode(spec[b:b + 1], alpha, min_value, channels), table[b, 0:2], guard=True) for b in range(spec.shape[0])]
    return np.concatenate(rows) if rows else np.zeros((0, channels) + spec.shape[:0:-1], dtype=F32), table
