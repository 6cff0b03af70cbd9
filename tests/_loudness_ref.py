"""A numpy float64 restatement of the loudness measurement of csrc/loudness.hip (ITU-R BS.1770-4 / EBU R 128): the K-weighting
coefficients, a plain sequential biquad cascade from zero state, hop energies, the two gates and the gain.  No scipy."""
import math

import numpy as np

# the seven coefficients BS.1770 prints for 48 kHz: shelf b0 b1 b2 a1 a2, high-pass a1 a2 (its b is 1, -2, 1)
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              -1.99004745483398, 0.99007225036621)
# single-hop levels (LUFS) of the gating vector of the tests, hop = 4800: loud, silent (under the absolute gate), quiet (under the
# relative one), loud again
GATING_LEVELS = (-20.0,) * 6 + (-80.0,) * 6 + (-35.0,) * 6 + (-20.0,) * 4


def coefficients(rate):
    """b0 b1 b2 a1 a2 of the shelf, then of the high-pass, as a float64 array of 10."""
    rate = float(rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(shelf + hp, dtype=np.float64)


def biquad(x, c5):
    """y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2] from zero state, one sample after the other, float64."""
    b0, b1, b2, a1, a2 = (float(v) for v in c5)
    y = [0.0] * len(x)
    x1 = x2 = y1 = y2 = 0.0
    for n, xn in enumerate(x.tolist()):
        yn = b0 * xn + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, xn, y1, yn
        y[n] = yn
    return np.array(y, dtype=np.float64)


def k_weighted(x, rate):
    """[C, L] (or [L]) -> the rows through the shelf and then the high-pass, float64."""
    c = coefficients(rate)
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    return np.stack([biquad(biquad(row, c[:5]), c[5:]) for row in x]) if x.shape[1] else x.copy()


def hop_energies(x, rate):
    """[C, L] -> z [C, J] float64: the sum of y^2 over each whole hop of rate / 10 samples."""
    hop = int(rate) // 10
    y = k_weighted(x, rate)
    J = y.shape[1] // hop
    return (y[:, :J * hop] ** 2).reshape(y.shape[0], J, hop).sum(axis=2)


def _lufs(p):
    with np.errstate(divide='ignore', invalid='ignore'):
        return -0.691 + 10.0 * np.log10(p)


def gating(z, rate, weights=None):
    """z [C, J] -> {'I', 'max', 'gamma', 'kept', 'l' (the block levels), 'p'}: 400 ms blocks of four hops, the absolute gate at
    -70 and the relative one 10 LU under the ungated mean; a block whose level is NaN stays in (as the kernel keeps it)."""
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    C, J = z.shape
    hop = int(rate) // 10
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    NB = max(J - 3, 0)
    ninf = float('-inf')
    if NB == 0:
        return {'I': ninf, 'max': ninf, 'gamma': ninf, 'kept': 0, 'l': np.zeros(0), 'p': np.zeros(0)}
    with np.errstate(invalid='ignore', over='ignore'):
        P = (((z[:, 0:NB] + z[:, 1:NB + 1]) + z[:, 2:NB + 2]) + z[:, 3:NB + 3]) / (4.0 * hop)
        p = np.zeros(NB)
        for c in range(C):
            p = p + w[c] * P[c]
        l = _lufs(p)
        top = float(np.fmax.reduce(np.concatenate([[ninf], l])))
        A = ~(l <= -70.0)
        if not A.any():
            return {'I': ninf, 'max': top, 'gamma': ninf, 'kept': 0, 'l': l, 'p': p}
        gamma = float(_lufs(p[A].mean())) - 10.0
        B = A & ~(l <= gamma)
        I = float(_lufs(p[B].mean())) if B.any() else ninf
    return {'I': I, 'max': top, 'gamma': gamma, 'kept': int(B.sum()), 'l': l, 'p': p}


def integrated(x, rate, weights=None):
    """The integrated loudness of [C, L] in LUFS."""
    return gating(hop_energies(x, rate), rate, weights)['I']


def gain(I, target, max_gain_db):
    """The float64 gain to `target` (None or NaN: none), clamped to +-max_gain_db; 1 where either level is not finite."""
    if target is None or not math.isfinite(target) or not math.isfinite(I):
        return 1.0
    return 10.0 ** (min(max(target - I, -max_gain_db), max_gain_db) / 20.0)


def hops_at_level(levels, hop):
    """Hop energies whose single-hop level is `levels` (LUFS): z = hop * 10^((L + 0.691) / 10)."""
    return hop * 10.0 ** ((np.asarray(levels, dtype=np.float64) + 0.691) / 10.0)


def warmup_hop_energies(x, rate, warm_hops=2):
    """What the kernel computes, restated: hop j from zero state at sample max(0, (j - warm_hops) hop), counting its own hop."""
    hop = int(rate) // 10
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    J = x.shape[1] // hop
    z = np.zeros((x.shape[0], J))
    for j in range(J):
        s0 = max(0, (j - warm_hops) * hop)
        y = k_weighted(x[:, s0:(j + 1) * hop], rate)
        z[:, j] = (y[:, j * hop - s0:] ** 2).sum(axis=1)
    return z
