"""Float64 numpy restatement of the output stage's rate converter (csrc/rateconv.hip, include/p2phd.h): the plan, the polyphase
table, the output length and the sum, exactly as the header defines them -- nothing of the library is used."""
import math

import numpy as np

from _truepeak_ref import bessel_i0

PASSBAND, ATTEN_DB = 0.907, 120.0


def plan(in_rate, out_rate, passband=PASSBAND, atten_db=ATTEN_DB):
    """-> {'o', 'n', 'taps_per_phase', 'beta', 'cutoff', 'passband_hz', 'stopband_hz'}; no refusals: the length is what the formula gives."""
    g = math.gcd(in_rate, out_rate)
    nyq = min(in_rate, out_rate) / 2.0
    fp = passband * nyq
    fs = 2.0 * nyq - fp
    P = 2 * int(math.ceil((atten_db - 7.95) / (2.0 * 2.285 * (2.0 * math.pi * (fs - fp) / in_rate))))
    return {'in_rate': in_rate, 'out_rate': out_rate, 'o': in_rate // g, 'n': out_rate // g, 'taps_per_phase': P,
            'beta': 0.1102 * (atten_db - 8.7), 'cutoff': 2.0 * nyq / in_rate, 'passband_hz': fp, 'stopband_hz': fs}


def table(o, n, P, beta, cutoff):
    """c[n][P] in float64: phase p has frac = ((p o) mod n) / n, tau = (k - (P/2 - 1)) - frac,
    c = fc sinc(fc tau) I0(beta sqrt(1 - (tau / (P/2))^2)) / I0(beta), every phase divided by its own sum."""
    c = np.zeros((n, P), dtype=np.float64)
    i0b = bessel_i0(beta)
    half = P // 2 - 1
    for p in range(n):
        frac = ((p * o) % n) / n
        for k in range(P):
            tau = (k - half) - frac
            r = tau / (P // 2)
            c[p, k] = cutoff * np.sinc(cutoff * tau) * bessel_i0(beta * math.sqrt(max(0.0, 1.0 - r * r))) / i0b
        c[p] /= c[p].sum()
    return c


def out_len(L, o, n):
    return -((-L * n) // o)


def convert(x, c, o, n, absolute=False):
    """Row x [L] (any numeric dtype; integers stay integers, everything else is float64) through the table c [n][P] ->
    y [ceil(L n / o)]: y[j n + p] = sum_k c[p][k] x~[j o + (p o) div n + k - half], x~ zero outside the row.  `absolute`: sum_k |c x~|
    instead, what the worst-case bound of an fp32 dot product multiplies."""
    x, c = np.asarray(x), np.asarray(c)
    if not (np.issubdtype(x.dtype, np.integer) and np.issubdtype(c.dtype, np.integer)):
        x, c = x.astype(np.float64), c.astype(np.float64)
    if absolute:
        x, c = np.abs(x), np.abs(c)
    P = c.shape[1]
    half = P // 2 - 1
    Lo = out_len(len(x), o, n)
    m = np.arange(Lo, dtype=np.int64)
    p = m % n
    i0 = (m // n) * o + (p * o) // n                                        # window m starts at x~[i0 - half]
    ext = np.zeros(half + len(x) + P + o + 1, dtype=x.dtype)
    ext[half:half + len(x)] = x                                             # ext[q + half] = x~[q]
    return (ext[i0[:, None] + np.arange(P, dtype=np.int64)[None, :]] * c[p]).sum(axis=1)


def dot_bound(x, c, o, n):
    """P 2^-24 sum_k |c x~| per output of `convert`: how far an fp32 fma chain of P terms may lie from the float64 sum (after
    _truepeak_ref.dot_bound: every product exact in the fma, P roundings of partial sums none of which exceeds the absolute sum, plus
    the rounding of the operands, which here are fp32 already)."""
    return np.asarray(c).shape[1] * 2.0 ** -24 * convert(x, c, o, n, absolute=True)


def response_db(c, o, n, in_rate, n_fft=None):
    """The magnitude response of the prototype the table samples, through a zero-padded FFT at rate n * in_rate -> (f in Hz, dB),
    DC at 0 dB: coefficient c[p][k] sits at fine index (k - half) n - ((p o) mod n)."""
    c = np.asarray(c, dtype=np.float64)
    P = c.shape[1]
    half = P // 2 - 1
    h = np.zeros((P + 1) * n, dtype=np.float64)
    for p in range(n):
        r = (p * o) % n
        h[(np.arange(P) - half) * n - r + half * n + n] = c[p]
    if n_fft is None:
        n_fft = 1 << int(math.ceil(math.log2(16 * len(h))))
    H = np.abs(np.fft.rfft(h, n_fft)) / n
    f = np.arange(len(H)) * (n * float(in_rate) / n_fft)
    return f, 20.0 * np.log10(np.maximum(H, 1e-300))
