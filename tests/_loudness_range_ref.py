"""A numpy float64 restatement of the loudness-range measurement of csrc/loudness.hip (EBU Tech 3342, the short-term maximum of
EBU R 128): the 3 s blocks of 30 hops, the absolute gate at -70 LUFS and the relative gate 20 LU under the mean of what passed,
both in the power domain, and the 10th / 95th percentile by the integer rank of the Tech 3342 reference code.  No scipy."""
import numpy as np

BLOCK_HOPS = 30
P_ABS = 1.1724653045822981e-07                                     # 10^((-70 + 0.691) / 10)
FOLD = 256                                                         # the fixed order of the mean: 256 strided partial sums, a tree


def _lufs(p):
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(-0.691 + 10.0 * np.log10(np.float64(p)))


def ranks(n):
    """The zero-based ranks of the 10th and the 95th percentile among n ordered values: round((n - 1) PRC / 100 + 1) - 1."""
    n = int(n)
    return ((n - 1) * 10 + 50) // 100, ((n - 1) * 95 + 50) // 100


def block_powers(z, rate, weights=None, gain=None):
    """z [C, J] -> p [max(J - 29, 0)]: every block's own 30-term sum left to right, / (30.0 hop), the channels weighted in ascending
    order from 0.0, times (g g) where a gain (a float32) is given.  One IEEE operation per step, nothing contracted."""
    z = np.atleast_2d(np.asarray(z, dtype=np.float64))
    C, J = z.shape
    hop = int(rate) // 10
    w = np.ones(C) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    NS = max(J - (BLOCK_HOPS - 1), 0)
    p = np.zeros(NS)
    if NS == 0:
        return p
    with np.errstate(invalid='ignore', over='ignore'):
        for c in range(C):
            S = z[c, 0:NS] + z[c, 1:NS + 1]
            for i in range(2, BLOCK_HOPS):
                S = S + z[c, i:NS + i]
            p = p + w[c] * (S / (30.0 * hop))
        if gain is not None:
            g = np.float64(np.float32(gain))
            p = p * (g * g)
    return p


def _fold_mean(p, kept):
    """The mean of p[kept] in the kernel's order: partial sum t takes the kept powers of blocks t, t + 256, .. in ascending order
    (a block that is not kept adds 0.0, which changes no bit of a non-negative sum), the 256 partial sums meet in a halving tree."""
    n = int(kept.sum())
    v = np.where(kept, p, 0.0)
    v = np.concatenate([v, np.zeros((-len(v)) % FOLD)]).reshape(-1, FOLD)
    s = np.zeros(FOLD)
    with np.errstate(invalid='ignore', over='ignore'):
        for row in v:
            s = s + row
        o = FOLD // 2
        while o > 0:
            s[:o] = s[:o] + s[o:2 * o]
            o //= 2
        return s[0] / np.float64(n)


def loudness_range(p):
    """p [NS] -> {'lra', 'low', 'high', 'threshold' (LUFS), 'n', 'short_term_max' (LUFS), 'q_lo', 'q_hi' (the selected powers),
    'margin': the smallest relative distance |p - T| / T of any block power to either threshold T (inf where there is none)}."""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    ninf, inf, nan = float('-inf'), float('inf'), float('nan')
    top = float(np.fmax.reduce(np.concatenate([[0.0], p])))      # a NaN never wins
    out = {'lra': 0.0, 'low': ninf, 'high': ninf, 'threshold': ninf, 'n': 0, 'short_term_max': _lufs(top), 'q_lo': 0.0, 'q_hi': 0.0,
           'margin': inf}
    bad = bool(np.isnan(p).any())
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        A = p > P_ABS
        finite = p[np.isfinite(p)]
        if finite.size:
            out['margin'] = float(np.min(np.abs(finite - P_ABS) / P_ABS))
        if A.any():
            rel = 0.01 * _fold_mean(p, A)
            out['threshold'] = _lufs(rel)
            if np.isfinite(rel) and rel > 0.0 and finite.size:
                out['margin'] = min(out['margin'], float(np.min(np.abs(finite - rel) / rel)))
            q = np.sort(p[A & (p > rel)])
            out['n'] = int(q.size)
    if bad:
        out.update(lra=nan, low=nan, high=nan, q_lo=nan, q_hi=nan)
    elif out['n'] > 0:
        k_lo, k_hi = ranks(out['n'])
        out.update(q_lo=float(q[k_lo]), q_hi=float(q[k_hi]), low=_lufs(q[k_lo]), high=_lufs(q[k_hi]))
        out['lra'] = out['high'] - out['low']
    return out


def integer_hops(C, J, seed=5):
    """z [C, J] of integers below 2^20 as float64 -- every 30-term sum is exact (below 2^25), so each later step of block_powers is
    one IEEE operation and a kernel must give its bits.  Every block passes both gates, far from either threshold."""
    return np.random.default_rng(seed).integers(0, 1 << 20, size=(C, J)).astype(np.float64)


def measure(z, rate, weights=None, gain=None):
    """block_powers and loudness_range in a row."""
    return loudness_range(block_powers(z, rate, weights, gain))
