"""numpy restatement of what streaming a file in windows (generate/stream.py, plans.stream_plan) rests on, written from the
definitions: the polyphase resampler of csrc/resample.hip in integer arithmetic -- an integer table, integer samples, int64 sums,
so that "the same operands" is "the same number" with no rounding to hide behind -- over a whole row and over a window with its
halo, and the cross-fading stitch of tests/_generate_ref.py over one window with the carry of the window before."""
import math

import numpy as np

import _generate_ref as G


def geometry(orig, new, lpw=6, rolloff=0.99):
    """(o, n, width, klen): the rates over their common divisor, the halo and the taps of one phase."""
    gd = math.gcd(orig, new)
    o, n = orig // gd, new // gd
    width = int(math.ceil(lpw * o / (min(o, n) * rolloff)))
    return o, n, width, 2 * width + o


def table(orig, new, seed=0):
    """An integer phase table [n, klen]: any numbers do, the test is about which operands meet."""
    o, n, width, klen = geometry(orig, new)
    return np.random.default_rng(seed + 7 * orig + new).integers(-9, 10, size=(n, klen)).astype(np.int64)


def out_len(T, orig, new):
    o, n, _, _ = geometry(orig, new)
    return (n * T + o - 1) // o


def resample(x, orig, new, h):
    """y[j n + p] = sum_k h[p][k] x[j o + k - width], zeros outside the row; ceil(n T / o) outputs.  x: int64 [T]."""
    o, n, width, klen = geometry(orig, new)
    T = len(x)
    T_out = (n * T + o - 1) // o
    J = -(-T_out // n)
    padded = np.zeros(width + max(T, (J - 1) * o + klen), dtype=np.int64)
    padded[width:width + T] = x
    y = np.zeros((J, n), dtype=np.int64)
    for j in range(J):
        y[j] = h @ padded[j * o:j * o + klen]
    return y.reshape(-1)[:T_out]


def chain(in_rate, lr_rate, hr_rate, is_lr_input):
    pairs = [(in_rate, hr_rate)] if is_lr_input else [(in_rate, lr_rate), (lr_rate, hr_rate)]
    return [(a, b) for a, b in pairs if a != b]


def round_trip(x, in_rate, lr_rate, hr_rate, is_lr_input, seed=0):
    """The whole row through the low-rate round trip, cut to its own length where the input is at the high rate."""
    y = np.asarray(x, dtype=np.int64)
    for a, b in chain(in_rate, lr_rate, hr_rate, is_lr_input):
        y = resample(y, a, b, table(a, b, seed))
    return y[:len(x)] if not is_lr_input and in_rate == hr_rate else y


def round_trip_window(x, plan, window, seed=0):
    """The window's frames alone through the stages of the plan, each cut as the plan says -> the needed range of the clip."""
    f0, f1 = window['read']
    y = np.asarray(x[f0:f1], dtype=np.int64)
    for (a, b, *_), (lo, hi) in zip(plan['stages'], window['cuts']):
        y = resample(y, a, b, table(a, b, seed))
        assert 0 <= lo <= hi <= len(y), (lo, hi, len(y))
        y = y[lo:hi]
    return y


def stitch_stream(seg, stride, gain, carry_in, n_out, last):
    """One window's K segments [K, T] (float64) -> (its n_out stitched samples, its carry).  `carry_in`: None for the clip's first
    window, else the raw samples [stride, T) of the segment in front.  The sums are _generate_ref.stitch's, in its order: the earlier
    segment's part first."""
    seg = np.asarray(seg, dtype=np.float64)
    K, T = seg.shape
    V = T - stride
    f = G.fade_in(V)
    out = np.zeros((K - 1) * stride + T, dtype=np.float64)
    if carry_in is not None and V:
        out[:V] += (1.0 - f) * np.asarray(carry_in, dtype=np.float64)
    for s in range(K):
        w = np.ones(T, dtype=np.float64)
        if (s > 0 or carry_in is not None) and V:
            w[:V] = f
        if s < K - 1 and V:
            w[T - V:] = 1.0 - f
        out[s * stride:s * stride + T] += w * seg[s]
    assert last or n_out <= K * stride
    return float(gain) * out[:n_out], seg[K - 1, stride:].copy()
