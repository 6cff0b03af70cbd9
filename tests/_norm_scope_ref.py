"""A numpy restatement of the dB encode of Pix2PixHDModel.to_spectro (explicit encoding and the single-channel magnitude
encoding) and of its normalisation under a range that is given, in float32 like the kernels (csrc/spectro.hip).  It states the
premise of norm_scope='clip' -- a group under its own range against the same group under its clip's range -- and is no
bit-for-bit model of the kernels: log10 is numpy's."""
import numpy as np

F32 = np.float32


def db_encode(spec, alpha=0.6, min_value=1e-7, channels=2):
    """spec [B, F, M] -> the dB planes [B, channels, M, F] in front of the normalisation."""
    s = np.asarray(spec, dtype=F32)
    alpha, mv = F32(alpha), F32(min_value)
    if channels == 2:
        neg = F32(0.5) * (np.abs(s) - s)
        pos = s + neg
        d0 = F32(20) * np.log10(np.maximum(alpha * pos + (F32(1) - alpha) * neg, mv)) - F32(20)
        d1 = F32(20) * np.log10(np.maximum((F32(1) - alpha) * pos + alpha * neg, mv)) - F32(20)
        d = np.stack([d0, d1], axis=1)
    else:
        d = (F32(20) * np.log10(np.maximum(np.abs(s) + mv, mv)) - F32(20))[:, None]
    return np.ascontiguousarray(d.transpose(0, 1, 3, 2)).astype(F32)


def own_range(db):
    """The range the group's own statistics give: what norm_scope='group' normalises by."""
    return F32(db.min()), F32(db.max())


def fold(a, b):
    """Two ranges -> the range of their union; (+inf, -inf) is the neutral element."""
    return min(a[0], b[0]), max(a[1], b[1])


EMPTY = (F32(np.inf), F32(-np.inf))


def normalise(db, rng, guard=False):
    """(db - min) * (1 / (max - min)), as encode_pass2_kernel writes it; with `guard` a range of zero scales by 0, as
    encode_given_kernel does."""
    mn, mx = F32(rng[0]), F32(rng[1])
    with np.errstate(divide='ignore', invalid='ignore'):
        width = mx - mn
        scale = F32(0) if guard and width == 0 else F32(1) / width
        return ((db - mn) * scale).astype(F32)
