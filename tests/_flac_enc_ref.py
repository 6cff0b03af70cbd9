"""A restatement of the FLAC encoder's stream contract (include/p2phd.h, "FLAC output") in Python.  It shares no code with the
library: the decisions are taken here from cumulative sums in numpy int64 (the library folds a tree of partition sums), and the bits
are written by tests/_flac_ref.py's bit writer, subframe writer and frame header, which the FLAC reader's tests already hold.

    candidates(x, bps, bits)             every admitted (order, partition order) of one block with its bits
    choose(x, bps, bits)                 the subframe of one coded channel: (spec for _flac_ref.write_subframe, its bits, a description)
    encode_frames(channels, bits, rate, block)   -> (frames, decisions): the frames' bytes; per frame (assignment, [description per coded channel])
    stream(channels, bits, rate, block, md5=False)   -> the whole file
    payload(channels, bits)              the interleaved little-endian payload the encoders take"""
import numpy as np

import _flac_ref as R


def payload(channels, bits):
    nb = bits // 8
    a = np.asarray(channels, dtype=np.int64).T.reshape(-1)
    return b"".join((int(v) & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little") for v in a)


def trailing_zeros(v):
    return (v & -v).bit_length() - 1


def candidates(x, bps, bits):
    """Every admitted FIXED pair of one block: {(o, p): (bits of the subframe, [k per partition], a partition has two equally cheap k)}."""
    x = np.asarray(x, dtype=np.int64)
    bs = len(x)
    pbits, K = (4, 15) if bits == 16 else (5, 31)
    out = {}
    for o in range(0, min(4, bs - 1) + 1):
        r = np.diff(x, n=o)                                                 # the fixed predictor's residuals of samples o .. bs - 1
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        cs = np.zeros((K, len(u) + 1), dtype=np.int64)
        for k in range(K):
            cs[k, 1:] = np.cumsum(u >> k)
        for p in range(0, min(8, trailing_zeros(bs)) + 1):
            psize = bs >> p
            if psize <= o:
                continue
            edges = np.maximum(np.arange((1 << p) + 1) * psize - o, 0)     # in residual indices
            n = np.diff(edges)
            cost = n[None, :] * (np.arange(K)[:, None] + 1) + (cs[:, edges[1:]] - cs[:, edges[:-1]])
            ks = cost.argmin(axis=0)                                        # the first minimum: the smaller k
            low = cost.min(axis=0)
            out[(o, p)] = (8 + o * bps + 2 + 4 + int((pbits + low).sum()), [int(k) for k in ks], bool(((cost == low[None, :]).sum(axis=0) > 1).any()))
    return out


_CHOSEN = {}                                                                # (the block's bytes, bps, bits) -> choose's answer


def choose(x, bps, bits):
    """x: the coded channel's integers of one block -> (spec, bits of the subframe, (kind, order, porder, [k per partition])).  The
    answer depends on nothing else, so it is kept: the same block under another rate or frame number is not worked out again."""
    x = np.ascontiguousarray(x, dtype=np.int64)
    key = (x.tobytes(), bps, bits)
    if key not in _CHOSEN:
        if len(_CHOSEN) >= 4096:
            _CHOSEN.clear()
        _CHOSEN[key] = _choose(x, bps, bits)
    spec, total, described = _CHOSEN[key]
    return dict(spec, **({'params': list(spec['params'])} if 'params' in spec else {})), total, described


def _choose(x, bps, bits):
    bs = len(x)
    if (x == x[0]).all():
        return dict(kind="constant"), 8 + bps, ("constant", 0, 0, [])
    best = (8 + bs * bps, None)                                             # VERBATIM, unless something is strictly smaller
    for (o, p), (total, ks, _) in sorted(candidates(x, bps, bits).items(), key=lambda item: (item[0][1], item[0][0])):
        if total < best[0]:                                                 # strict: ties keep the smaller p, then the smaller o
            best = (total, (o, p, ks))
    if best[1] is None:
        return dict(kind="verbatim"), best[0], ("verbatim", 0, 0, [])
    o, p, ks = best[1]
    return dict(kind="fixed", order=o, method=0 if bits == 16 else 1, porder=p, params=ks), best[0], ("fixed", o, p, ks)


def encode_frames(channels, bits, rate, block):
    C, L = len(channels), len(channels[0])
    chans = [np.asarray(c, dtype=np.int64) for c in channels]
    rate_code = 0 if rate not in R.RATE_CODES and rate >= 65536 and (rate % 10 or rate // 10 >= 65536) else None
    frames, decisions = [], []
    for number, at in enumerate(range(0, L, block)):
        chunk = [c[at:at + block] for c in chans]
        if C == 2:
            left, right = chunk
            cand = [choose(left, bits, bits), choose(right, bits, bits), choose((left + right) >> 1, bits, bits), choose(left - right, bits + 1, bits)]
            l, r, m, s = (c[1] for c in cand)
            sums = [(l + r, 1, (0, 1)), (l + s, R.LEFT_SIDE, (0, 3)), (s + r, R.SIDE_RIGHT, (3, 1)), (m + s, R.MID_SIDE, (2, 3))]
            _, assign, pick = min(sums, key=lambda t: t[0])                 # min keeps the first of equals: ties in that order
            chosen = [cand[i] for i in pick]
        else:
            assign = C - 1
            chosen = [choose(c, bits, bits) for c in chunk]
        kw = {} if rate_code is None else dict(rate_code=rate_code)
        frames.append(R.encode_frame([[int(v) for v in c] for c in chunk], bits, number, rate, assign=assign, specs=[c[0] for c in chosen], **kw))
        decisions.append((assign, [c[2] for c in chosen]))
    return frames, decisions


def header(frames, channels, bits, rate, block, md5=False):
    C, L = len(channels), len(channels[0])
    digest = R.md5_of([[int(v) for v in c] for c in channels], bits) if md5 else b"\0" * 16
    return b"fLaC" + R.metadata_block(0, R.streaminfo(rate, C, bits, L, block, block, digest, min(map(len, frames)), max(map(len, frames))), last=True)


def stream(channels, bits, rate, block, md5=False):
    frames, _ = encode_frames(channels, bits, rate, block)
    return header(frames, channels, bits, rate, block, md5) + b"".join(frames)
