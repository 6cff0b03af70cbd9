"""A restatement of the LPC extension of the FLAC encoder's stream contract (include/p2phd.h, "FLAC output, LPC") in Python.  It shares
no code with the library: steps 2 and 3 run on Python floats (IEEE float64, one operation per expression, never contracted), everything
else on numpy int64; the subframe every block starts from is tests/_flac_enc_ref.py's choice, the Rice bits are counted from cumulative
sums as its `candidates` counts them, and the bits are written by tests/_flac_ref.py's write_subframe(kind='lpc').

    analysis(x, bps, M)                  step 1: R[0 .. Mo] as Python ints
    fit(R)                               steps 2 and 3: {order: (q, shift)} of the admitted orders
    analyse(x, bps, M)                   both
    residual(x, q, shift)                step 4: r[o .. bs) as int64
    lpc_candidates(x, bps, bits, M)      {(o, p): (bits, [k per partition], q, shift)} of every admitted LPC pair
    choose(x, bps, bits, M)              the subframe of one coded channel, as _flac_enc_ref.choose returns it
    encode_frames / header / stream      as _flac_enc_ref's, with M"""
import math

import numpy as np

import _flac_enc_ref as E
import _flac_ref as R

P = 13                                                                      # bits of a coefficient
MAX_ORDER = 12
MAX_BLOCK = 16384
RES_LIMIT = 1 << 28


def analysis(x, bps, M):
    x = np.asarray(x, dtype=np.int64)
    bs = len(x)
    a = x >> max(0, bps - 16)
    n = np.arange(bs, dtype=np.int64)
    d, D = 2 * n - (bs - 1), bs + 1
    W = ((D * D - d * d) << 15) // (D * D)
    v = (a * W) >> 15
    Mo = min(M, bs - 1)
    return [int((v[l:] * v[:bs - l]).sum()) for l in range(Mo + 1)]


def fit(Rl):
    """R[0 .. Mo] -> {o: (q, shift)}."""
    out = {}
    Mo = len(Rl) - 1
    if Rl[0] == 0:
        return out
    Rf = [float(r) for r in Rl]
    err = Rf[0]
    lp = []
    for i in range(Mo):
        acc = Rf[i + 1]
        for j in range(i):
            acc = acc - lp[j] * Rf[i - j]
        k = acc / err
        new = [lp[j] - k * lp[i - 1 - j] for j in range(i)] + [k]
        err = err * (1.0 - k * k)
        if not err > 0.0 or not math.isfinite(err):
            break
        lp = new
        cmax = max(abs(c) for c in lp)
        if cmax == 0.0:
            continue
        shift = P - 1 - math.frexp(cmax)[1]
        if shift < 0:
            continue
        shift = min(shift, 15)
        ee, q = 0.0, []
        for c in lp:
            ee = ee + math.ldexp(c, shift)
            v = math.floor(ee + 0.5) if ee >= 0 else -math.floor(-ee + 0.5)
            v = max(-(1 << (P - 1)), min((1 << (P - 1)) - 1, v))
            q.append(int(v))
            ee = ee - v
        out[i + 1] = (q, shift)
    return out


def analyse(x, bps, M):
    Rl = analysis(x, bps, M)
    return Rl, fit(Rl)


def residual(x, q, shift):
    x = np.asarray(x, dtype=np.int64)
    o, bs = len(q), len(x)
    s = np.zeros(bs - o, dtype=np.int64)
    for j, c in enumerate(q):
        s += c * x[o - 1 - j:bs - 1 - j]
    return x[o:] - (s >> shift)


def rice_bits(r, bs, o, bits):
    """The residuals r of samples o .. bs - 1 -> {p: (the partitions' bits with their parameters' fields, [k per partition])}: the
    counting of _flac_enc_ref.candidates."""
    pbits, K = (4, 15) if bits == 16 else (5, 31)
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    cs = np.zeros((K, len(u) + 1), dtype=np.int64)
    for k in range(K):
        cs[k, 1:] = np.cumsum(u >> k)
    out = {}
    for p in range(0, min(8, E.trailing_zeros(bs)) + 1):
        psize = bs >> p
        if psize <= o:
            continue
        edges = np.maximum(np.arange((1 << p) + 1) * psize - o, 0)
        n = np.diff(edges)
        cost = n[None, :] * (np.arange(K)[:, None] + 1) + (cs[:, edges[1:]] - cs[:, edges[:-1]])
        out[p] = (int((pbits + cost.min(axis=0)).sum()), [int(k) for k in cost.argmin(axis=0)])
    return out


def lpc_candidates(x, bps, bits, M):
    x = np.asarray(x, dtype=np.int64)
    bs = len(x)
    out = {}
    for o, (q, shift) in analyse(x, bps, M)[1].items():
        r = residual(x, q, shift)
        if int(np.abs(r).max()) >= RES_LIMIT:
            continue
        for p, (part, ks) in rice_bits(r, bs, o, bits).items():
            out[(o, p)] = (8 + o * bps + 4 + 5 + o * P + 2 + 4 + part, ks, q, shift)
    return out


def choose(x, bps, bits, M):
    x = np.ascontiguousarray(x, dtype=np.int64)
    spec, total, described = E.choose(x, bps, bits)
    if M == 0 or described[0] == "constant":
        return spec, total, described
    best = None
    for (o, p), (t, ks, q, shift) in sorted(lpc_candidates(x, bps, bits, M).items(), key=lambda item: (item[0][1], item[0][0])):
        if t < total:                                                       # strictly fewer; among LPC pairs the smaller p, then the smaller o
            total, best = t, (o, p, ks, q, shift)
    if best is None:
        return spec, total, described
    o, p, ks, q, shift = best
    return (dict(kind="lpc", coefs=list(q), precision=P, shift=shift, method=0 if bits == 16 else 1, porder=p, params=list(ks)), total,
            ("lpc", o, p, ks))


def encode_frames(channels, bits, rate, block, M):
    if not 0 <= M <= MAX_ORDER or (M > 0 and block > MAX_BLOCK):
        raise ValueError("lpc_order %r with block %r" % (M, block))
    C, L = len(channels), len(channels[0])
    chans = [np.asarray(c, dtype=np.int64) for c in channels]
    rate_code = 0 if rate not in R.RATE_CODES and rate >= 65536 and (rate % 10 or rate // 10 >= 65536) else None
    frames, decisions = [], []
    for number, at in enumerate(range(0, L, block)):
        chunk = [c[at:at + block] for c in chans]
        if C == 2:
            left, right = chunk
            cand = [choose(left, bits, bits, M), choose(right, bits, bits, M), choose((left + right) >> 1, bits, bits, M), choose(left - right, bits + 1, bits, M)]
            l, r, m, s = (c[1] for c in cand)
            sums = [(l + r, 1, (0, 1)), (l + s, R.LEFT_SIDE, (0, 3)), (s + r, R.SIDE_RIGHT, (3, 1)), (m + s, R.MID_SIDE, (2, 3))]
            _, assign, pick = min(sums, key=lambda t: t[0])
            chosen = [cand[i] for i in pick]
        else:
            assign = C - 1
            chosen = [choose(c, bits, bits, M) for c in chunk]
        kw = {} if rate_code is None else dict(rate_code=rate_code)
        frames.append(R.encode_frame([[int(v) for v in c] for c in chunk], bits, number, rate, assign=assign, specs=[c[0] for c in chosen], **kw))
        decisions.append((assign, [c[2] for c in chosen]))
    return frames, decisions


header = E.header


def stream(channels, bits, rate, block, M, md5=False):
    frames, _ = encode_frames(channels, bits, rate, block, M)
    return header(frames, channels, bits, rate, block, md5) + b"".join(frames)
