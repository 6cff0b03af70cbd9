"""numpy restatement of the segment gather and the cross-fading stitch of whole-file generation (csrc/stitch.hip), in
float64: what tests/test_generate_host.py and tests/test_gpu_generate.py compare the kernels and the segment arithmetic
with.  Written from the definitions, one loop over segments, nothing shared with the product code."""
import math

import numpy as np


def plan(L, T, overlap):
    """(S, stride, V): V = int(overlap * T) shared samples, stride = T - V, S = max(1, ceil((L - V) / stride))."""
    V = int(overlap * T)
    stride = T - V
    return max(1, int(math.ceil((L - V) / stride))), stride, V


def gather(audio, T, stride, S):
    audio = np.asarray(audio)
    out = np.zeros((S, T), dtype=audio.dtype)
    for s in range(S):
        piece = audio[s * stride: s * stride + T]
        out[s, :len(piece)] = piece
    return out


def fade_in(V):
    """Weights of the incoming segment over an overlap of V samples: sin^2(pi (i + 1/2) / (2 V))."""
    i = np.arange(V, dtype=np.float64)
    return np.sin(np.pi * (i + 0.5) / (2.0 * V)) ** 2 if V else np.zeros(0)


def weights(S, T, stride):
    """[S, T] float64: the weight of every sample of every segment (1 outside the overlaps; no fade-in on the first
    segment, no fade-out on the last)."""
    V = T - stride
    w = np.ones((S, T), dtype=np.float64)
    f = fade_in(V)
    for s in range(S):
        if s > 0:
            w[s, :V] = f
        if s < S - 1 and V:
            w[s, T - V:] = 1.0 - f
    return w


def stitch(seg, stride, gain, L_out):
    """float64 overlap-add of the weighted segments, cut to L_out."""
    seg = np.asarray(seg, dtype=np.float64)
    S, T = seg.shape
    w = weights(S, T, stride)
    out = np.zeros((S - 1) * stride + T, dtype=np.float64)
    for s in range(S):
        out[s * stride: s * stride + T] += w[s] * seg[s]
    return float(gain) * out[:L_out]


def weight_sum(S, T, stride):
    """Sum of the weights that land on every sample of the span."""
    w = weights(S, T, stride)
    out = np.zeros((S - 1) * stride + T, dtype=np.float64)
    for s in range(S):
        out[s * stride: s * stride + T] += w[s]
    return out
