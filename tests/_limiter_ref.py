"""Float64 numpy restatement of the look-ahead true-peak limiter (csrc/limiter.hip, include/p2phd.h): the window, the envelope,
the sliding minimum, the curve and its application, exactly as the header comment of csrc/limiter.hip defines them -- nothing of
the library is used.  `curve32` is the curve in the kernel's own order and precision, for operands whose sums fp32 holds."""
import numpy as np

import _truepeak_ref as TP


def window(A):
    """w[0 .. A] in float64: 0.5 - 0.5 cos(2 pi (k + 1) / (A + 2)), divided by its sum."""
    k = np.arange(int(A) + 1, dtype=np.float64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1.0) / (int(A) + 2.0))
    return w / w.sum()


def envelope(x, c):
    """Rows x [C, L], table c [F][P] -> m [L] float64: per sample the largest, over the rows, of |x~[i]| and the fractional phases
    |y[i][p]|, |y[i - 1][p]| on both of its sides."""
    x = np.atleast_2d(np.asarray(x))
    L = x.shape[1]
    m = np.zeros(L, dtype=np.float64)
    for row in x:
        y = np.abs(TP.oversampled(row, c))                         # line i + 1: y[i][.], i = -1 .. L - 1
        frac = y[:, 1:].max(axis=1) if y.shape[1] > 1 else np.zeros(L + 1)
        m = np.maximum(m, np.maximum(y[1:, 0], np.maximum(frac[1:], frac[:-1])))
    return m


def ratio(m, ceiling):
    """r = m > c ? c / m : 1 in fp32, one division (m and c are rounded to fp32 first)."""
    m, c = np.asarray(m, dtype=np.float32), np.float32(ceiling)
    with np.errstate(divide='ignore'):
        return np.where(m > c, c / np.where(m > c, m, np.float32(1.0)), np.float32(1.0)).astype(np.float32)


def sliding_min(r, A, H):
    """h[j] = min(r[j - H .. j + A]) for j = -A .. L - 1 (index q = j + A), r taken as 1 outside [0, L); the dtype of r."""
    r = np.asarray(r)
    A, H = int(A), int(H)
    ext = np.concatenate([np.ones(A + H, dtype=r.dtype), r, np.ones(A, dtype=r.dtype)])      # ext[p] = r[p - A - H]
    return np.lib.stride_tricks.sliding_window_view(ext, A + H + 1).min(axis=1)


def curve(r, w, A, H):
    """The gain curve in float64 from fp32 r and the window w: g = min(r, 1 - sum_k w[k] d[i - k]) with d = 1.0f - h formed in fp32
    as the definition has it -> (g [L], sum_k |w[k] d[i - k]| [L], what the bound of the fp32 sum multiplies)."""
    r = np.asarray(r, dtype=np.float32)
    L, A = len(r), int(A)
    d = (np.float32(1.0) - sliding_min(r, A, H)).astype(np.float64)
    w = np.asarray(w, dtype=np.float64)
    s = np.convolve(d, w)[A:A + L]
    a = np.convolve(np.abs(d), np.abs(w))[A:A + L]
    return np.minimum(r.astype(np.float64), 1.0 - s), a


def curve32(r, w, A, H):
    """The curve in the kernel's order: d = 1.0f - h, one fp32 accumulator from +0 that takes fma(w[k], d[i - k], acc) for
    k = 0 .. A, g = min(r, 1.0f - s).  The fma is formed as a float64 product (exact) and sum, rounded to fp32: the kernel's bits
    wherever that sum is exact in float64 -- always for operands on a dyadic grid."""
    r = np.asarray(r, dtype=np.float32)
    L, A = len(r), int(A)
    d = (np.float32(1.0) - sliding_min(r, A, H)).astype(np.float32).astype(np.float64)
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    acc = np.zeros(L, dtype=np.float32)
    for k in range(A + 1):
        acc = (w[k] * d[A - k:A - k + L] + acc.astype(np.float64)).astype(np.float32)
    return np.minimum(r, np.float32(1.0) - acc).astype(np.float32)


def reach(r, A, H):
    """True at every i whose g a sample with r < 1 can reach: i - (A + H) .. i + A holds one."""
    low = (np.asarray(r) < 1).astype(np.int64)
    A, H = int(A), int(H)
    ext = np.concatenate([np.zeros(A + H, dtype=np.int64), low, np.zeros(A, dtype=np.int64)])
    return np.lib.stride_tricks.sliding_window_view(ext, 2 * A + H + 1).max(axis=1) > 0 if len(low) else np.zeros(0, dtype=bool)


def limit(x, ceiling, c, A, H):
    """The whole limiter in float64 on rows x [C, L] (the envelope and the division rounded to fp32 as defined, the window in
    fp32 as the library stores it) -> (the limited rows, g, m)."""
    x = np.atleast_2d(np.asarray(x))
    m = envelope(x, c)
    r = ratio(m, ceiling)
    g, _ = curve(r, window(A).astype(np.float32), A, H)
    return TP.clean(x) * g[None, :], g, m
