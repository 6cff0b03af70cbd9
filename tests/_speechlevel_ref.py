"""Numpy restatement of the active speech level (ITU-T P.56 method B) of whole-file generation, exactly as the section "Active
speech level" of include/p2phd.h defines it -- nothing of the product is imported.  Two forms:

  sequential(x, rate)      the plain recursion sample by sample, with one hangover counter per threshold, as a speech voltmeter
                           runs it; Python floats (IEEE doubles, every operation rounded on its own).
  chunked(x, consts, I)    the contract's parallel order: chunks of 256, the carry over the chunks, the chunks again; the trailing
                           maximum in place of the counters.  `consts` are the values of p2phd_speechlevel_consts_fill, so the bits do
                           not rest on two exp implementations agreeing.

Both return the same dictionary per row; decide() and file_figure() are shared.
"""
import math

import numpy as np

L = 256
M = 15.9
THRESHOLDS = [2.0 ** (j - 15) for j in range(15)]
MIN_RATE, MAX_RATE = 8000, 192000


def consts(rate):
    """Python's own constants for `rate`: (g, h, gL, hL), I."""
    g = math.exp(-1.0 / (0.03 * rate))
    h = 1.0 - g
    gL = g
    for _ in range(8):
        gL = gL * gL
    return (g, h, gL, (256.0 * h) * gL), (rate + 4) // 5


def _log10(v):
    if v != v:
        return float('nan')
    if v == 0.0:
        return float('-inf')
    if v == float('inf'):
        return float('inf')
    return math.log10(v)


def decide(sq, a, n):
    """sq, the 15 counts and the number of frames -> {'active', 'long_term', 'activity', 'bracket'}."""
    sq = float(sq)
    if n <= 0:
        return {'active': float('-inf'), 'long_term': float('-inf'), 'activity': 0.0, 'bracket': -1}
    long_term = 10.0 * _log10(sq / n)
    if a[0] <= 0:
        return {'active': float('-inf'), 'long_term': long_term, 'activity': 0.0, 'bracket': -1}
    A = Ap = Dp = 0.0
    found = -1
    j = 0
    while j < 15 and a[j] > 0:
        Aj = 10.0 * _log10(sq / float(a[j]))
        Dj = Aj - 20.0 * math.log10(THRESHOLDS[j])
        if Dj <= M:
            if j == 0:
                A = Aj
            else:
                t = (Dp - M) / (Dp - Dj)
                A = Ap + t * (Aj - Ap)
            found = j
            break
        Ap, Dp = Aj, Dj
        j += 1
    if found < 0:
        A, found = Ap, j - 1
    e = (long_term - A) / 10.0
    activity = float('nan') if e != e else 10.0 ** e
    return {'active': A, 'long_term': long_term, 'activity': activity, 'bracket': found}


def file_figure(rows):
    """The per-row figures -> (the file's figure, the channel it is)."""
    pick = -1
    for c, r in enumerate(rows):
        if math.isfinite(r['active']) and (pick < 0 or r['active'] > rows[pick]['active']):
            pick = c
    if pick < 0:
        pick = 0
        for c, r in enumerate(rows):
            if not r['active'] == float('-inf'):
                pick = c
                break
    return rows[pick], pick


def gain_of(target, active, max_gain_db=40.0):
    """The float32 gain that brings `active` to `target`, clamped; 1 where either is not finite."""
    if target is None or not math.isfinite(target) or not math.isfinite(active):
        return np.float32(1.0)
    return np.float32(10.0 ** (min(max(target - active, -max_gain_db), max_gain_db) / 20.0))


def sequential_row(x, rate, k=None, I=None):
    """One row by the plain recursion and per-threshold hangover counters -> {'sq', 'a', and decide()'s keys}."""
    if k is None:
        k, I = consts(rate)
    g, h = k[0], k[1]
    xs = [float(v) for v in np.asarray(x, dtype=np.float32)]
    p = q = sq = 0.0
    a = [0] * 15
    hang = [I] * 15
    for v in xs:
        sq += v * v
        p = g * p + h * abs(v)
        q = g * q + h * p
        for j in range(15):
            if q >= THRESHOLDS[j]:
                a[j] += 1
                hang[j] = 0
            elif hang[j] < I:
                a[j] += 1
                hang[j] += 1
            else:
                break            # (exact: a threshold above was last met no later than this one, so its counter has run out too)
    out = decide(sq, a, len(xs))
    out.update(sq=sq, a=a)
    return out


def envelope_chunked(x, k, carries=False):
    """One row -> (m uint8 [n], sq) in the contract's order; `k` = (g, h, gL, hL).  `carries`: also (P, Q, s), one float64 per chunk:
    the state at the chunk's start and the chunk's energy -- what p2phd_speechlevel_envelope leaves in its workspace."""
    g, h, gL, hL = (np.float64(v) for v in k)
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    nch = -(-n // L)
    pad = np.zeros(nch * L, dtype=np.float64)
    pad[:n] = x.astype(np.float64)
    X = pad.reshape(nch, L)
    valid = (np.arange(nch * L).reshape(nch, L) < n)
    with np.errstate(all='ignore'):
        R = np.abs(X)
        # 1. every chunk from (0, 0); the chunk's energy left to right
        zp = np.zeros(nch); zq = np.zeros(nch); s = np.zeros(nch)
        for i in range(L):
            zp = (g * zp) + (h * R[:, i])
            zq = (g * zq) + (h * zp)
            s = np.where(valid[:, i], s + X[:, i] * X[:, i], s)
        # 2. the carry, left to right
        P = np.zeros(nch); Q = np.zeros(nch)
        cp = cq = np.float64(0.0)
        sq = np.float64(0.0)
        for c in range(nch):
            P[c], Q[c] = cp, cq
            sq = sq + s[c]
            cq = ((gL * cq) + (hL * cp)) + zq[c]
            cp = (gL * cp) + zp[c]
        # 3. every chunk again from (P, Q)
        m = np.zeros((nch, L), dtype=np.uint8)
        p, q = P.copy(), Q.copy()
        thr = np.array(THRESHOLDS)
        for i in range(L):
            p = (g * p) + (h * R[:, i])
            q = (g * q) + (h * p)
            m[:, i] = (q[:, None] >= thr[None, :]).sum(axis=1)     # (a NaN compares false: 0)
    if carries:
        return m.reshape(-1)[:n].copy(), float(sq), (P, Q, s)
    return m.reshape(-1)[:n].copy(), float(sq)


def trailing_max(m, I):
    """tm[i] = max(m[max(0, i - I)] .. m[i])."""
    r = np.asarray(m).copy()
    W, span = I + 1, 1
    while span < W:
        s = min(span, W - span)
        if s < r.shape[0]:
            r[s:] = np.maximum(r[s:], r[:-s])
        span += s
    return r


def counts_of(m, I):
    tm = trailing_max(m, I)
    return [int((tm > j).sum()) for j in range(15)]


def chunked_row(x, k, I):
    m, sq = envelope_chunked(x, k)
    a = counts_of(m, I)
    out = decide(sq, a, len(m))
    out.update(sq=sq, a=a, m=m)
    return out


def chunked(clip, k, I):
    """clip [C, n] -> (rows, file figure, channel)."""
    rows = [chunked_row(r, k, I) for r in np.atleast_2d(clip)]
    fig, ch = file_figure(rows)
    return rows, fig, ch


def sequential(clip, rate):
    rows = [sequential_row(r, rate) for r in np.atleast_2d(clip)]
    fig, ch = file_figure(rows)
    return rows, fig, ch


def modulated_noise(n, rate, seed, depth_hz=1.3, level=0.1):
    """Seeded noise under a slow raised-cosine modulation that reaches silence: a stand-in for speech with pauses."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    env = np.clip(np.sin(2 * np.pi * depth_hz * t), 0.0, None) ** 2
    return (level * env * rng.standard_normal(n)).astype(np.float32)


def gated_tone(n, rate, amp=0.25, freq=997.0, on_s=1.0, off_s=1.0):
    t = np.arange(n) / float(rate)
    gate = ((t % (on_s + off_s)) < on_s)
    return (amp * np.sin(2 * np.pi * freq * t) * gate).astype(np.float32)
