"""numpy restatement of the ragged gather and stitch of whole-file generation (csrc/stitch.hip, p2phd_segments_gather_ragged /
p2phd_segments_stitch_ragged): N clip rows -- the channels of several clips, each with its own length L and segment count S --
share one seg[rows, T].  Written from the entry's contract, one table row at a time and one output sample at a time, nothing
shared with the product code or with the per-clip restatement (tests/_generate_ref.py) it is compared with."""
import math

import numpy as np


def segments(L, T, stride):
    """The fewest segments whose span (S - 1) * stride + T reaches L, at least one."""
    return max(1, int(math.ceil((L - (T - stride)) / stride)))


def table(clips, T, stride):
    """clips: [C_i, L_i] arrays -> the rows (clip, channel, L, S, row0) in the order the entries take them: clip after clip, each
    channel-major; and the segment rows they close at."""
    rows, at = [], 0
    for k, clip in enumerate(clips):
        C, L = clip.shape
        S = segments(L, T, stride)
        for c in range(C):
            rows.append((k, c, L, S, at))
            at += S
    return rows, at


def gather_ragged(clips, T, stride):
    """clips: a list of [C_i, L_i] float32 arrays -> seg [rows, T]: seg[row0 + s, i] = clip[c, s * stride + i], zero beyond L."""
    rows, total = table(clips, T, stride)
    seg = np.zeros((total, T), dtype=np.float32)
    for k, c, L, S, row0 in rows:
        for s in range(S):
            for i in range(T):
                n = s * stride + i
                if n < L:
                    seg[row0 + s, i] = clips[k][c, n]
    return seg


def stitch_ragged(seg, lengths, channel_counts, stride, gain):
    """seg [rows, T] -> a list of [C_i, L_i] float64 arrays.  Output n of a row comes from the latest segment a = min(n // stride,
    S - 1) that covers it, at its sample i = n - a * stride; inside the overlap with the segment before (a > 0, i < V = T - stride)
    the two are cross-faded with w = sin^2(pi (i + 1/2) / (2 V)) on the later one."""
    seg = np.asarray(seg, dtype=np.float64)
    T = seg.shape[1]
    V = T - stride
    outs, at = [], 0
    for L, C in zip(lengths, channel_counts):
        S = segments(L, T, stride)
        out = np.zeros((C, L), dtype=np.float64)
        for c in range(C):
            for n in range(L):
                a = min(n // stride, S - 1)
                i = n - a * stride
                cur = seg[at + a, i]
                if a == 0 or i >= V:
                    out[c, n] = gain * cur
                else:
                    w = math.sin(math.pi * (i + 0.5) / (2.0 * V)) ** 2
                    out[c, n] = gain * (w * cur + (1.0 - w) * seg[at + a - 1, i + stride])
            at += S
        outs.append(out)
    assert at == seg.shape[0]
    return outs
