"""Helpers of the weight-pack tests: index coding, rounding vectors, an e4m3 encoder and the guarded pack call.

Index coding.  A pack kernel moves values, it computes nothing, so WHERE every master element lands can be read from the packed
buffer itself when the values name their own position.  Element i of a master tensor of n <= 2^24 - 1 elements is given the
number i + 1, split into three base-256 digits; one pack per digit.  A digit 0..255 is an integer of at most 8 significant bits:
exact in bf16, fp16 and f32, so the coding survives every storage type.  A packed element that is zero in all three passes is
padding (index + 1 >= 1 has a non-zero digit), anything else decodes to one master index.

Rounding vectors.  The integer operands of tests/_exact.py are representable in every storage type, so the f32 -> 16-bit
conversion of a pack never rounds there.  `rounding_vectors` builds, from the bit layout of the target type alone, the f32 values
at which a conversion can go wrong; the reference cast is torch.Tensor.to(dtype) on the CPU.

e4m3.  `e4m3_encode` is OCP e4m3fn in numpy: round to nearest even, saturating at +-448; tests/test_wpack_host.py pins it to
torch.float8_e4m3fn on every code, every midpoint and their f32 neighbours.

This module is a plain helper (no fixtures, no test functions); tests/test_wpack_host.py checks it on the CPU."""
import numpy as np
import torch

import _exact as X

MAX_ELEMS = 2 ** 24 - 1


# ----------------------------------------------------------------------------------------------------------------------
# index coding
# ----------------------------------------------------------------------------------------------------------------------
def index_digits(n):
    """Three float32 arrays [n]: digit p of (index + 1) in base 256, least significant first."""
    assert 0 < n <= MAX_ELEMS, n
    v = np.arange(1, n + 1, dtype=np.int64)
    return [((v >> (8 * p)) & 255).astype(np.float32) for p in range(3)]


def decode(passes, n):
    """`passes`: the three packed buffers (arrays of any float dtype, same shape) of the three digit packs.  Returns an int64
    array of that shape: -1 where all three are zero, else the master index.  Raises ValueError on a digit that is not an integer
    in 0..255 (a sum or a blend of elements, a stale byte pattern) and on an index >= n."""
    assert len(passes) == 3
    d = [np.asarray(p, dtype=np.float64) for p in passes]
    assert d[0].shape == d[1].shape == d[2].shape
    for p, a in enumerate(d):
        bad = ~((a >= 0) & (a <= 255) & (a == np.floor(a)))                # (NaN compares false: rejected)
        if bad.any():
            at = np.flatnonzero(bad.reshape(-1))[:8]
            raise ValueError(f"digit pass {p}: {int(bad.sum())} packed elements are not integers in 0..255, first at flat offsets "
                             f"{at.tolist()} = {a.reshape(-1)[at].tolist()}")
    v = d[0].astype(np.int64) + (d[1].astype(np.int64) << 8) + (d[2].astype(np.int64) << 16)
    src = v - 1
    if (src >= n).any():
        at = np.flatnonzero((src >= n).reshape(-1))[:8]
        raise ValueError(f"{int((src >= n).sum())} packed elements decode to an index >= {n}, first at flat offsets {at.tolist()} = "
                         f"{src.reshape(-1)[at].tolist()}")
    return src


def multiplicity(src, n):
    """How often every master element occurs in the decoded pack; raises ValueError unless all n occur equally often (>= 1).
    Returns that number."""
    counts = np.bincount(src[src >= 0].reshape(-1), minlength=n)
    lo, hi = int(counts.min()), int(counts.max())
    if lo == 0:
        miss = np.flatnonzero(counts == 0)
        raise ValueError(f"{miss.size} of {n} master elements appear nowhere in the pack, first {miss[:8].tolist()}")
    if lo != hi:
        odd = np.flatnonzero(counts != lo)
        raise ValueError(f"master elements appear {lo} to {hi} times; {odd.size} differ from {lo}, first {odd[:8].tolist()} x "
                         f"{counts[odd[:8]].tolist()}")
    return lo


def plain_pack(w, rows_pad, Cp, KK):
    """The documented plain layout in numpy: w [rows][inner][R][S] -> [rows_pad][KK] with element (row, tap, c) at
    row * KK + tap * Cp + c, zero in the channels inner..Cp, the K tail taps * Cp..KK and the rows rows..rows_pad."""
    rows, inner, R, S = w.shape
    assert rows <= rows_pad and inner <= Cp and R * S * Cp <= KK
    out = np.zeros((rows_pad, KK), dtype=w.dtype)
    body = np.zeros((rows, R * S, Cp), dtype=w.dtype)
    body[:, :, :inner] = w.reshape(rows, inner, R * S).transpose(0, 2, 1)
    out[:rows, :R * S * Cp] = body.reshape(rows, -1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# rounding vectors
# ----------------------------------------------------------------------------------------------------------------------
# (exponent bits, stored significand bits) of the 16-bit types; f32 drops DROP = 23 - significand bits on the way
_FMT = {torch.bfloat16: (8, 7), torch.float16: (5, 10)}
CLASSES = ("tie_even_below", "tie_even_above", "tie_minus_ulp", "tie_plus_ulp", "max_finite", "first_to_inf", "subnormal", "zero",
           "ordinary")


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def rounding_vectors(dtype, n_ordinary=64, seed=0):
    """dict class -> finite float32 array for the 16-bit `dtype` (both signs in every class):
    tie_even_below / tie_even_above: exactly halfway between two neighbours of the target's normal range, the even one being
    the smaller / the larger in magnitude; tie_minus_ulp / tie_plus_ulp: those ties moved by one f32 ulp towards / away from
    zero; max_finite: the largest finite value and the largest f32 that still rounds to it; first_to_inf: the smallest f32 that
    rounds to infinity (the tie above the largest finite value; its even neighbour is infinity) and its successor; subnormal:
    values whose rounded result is subnormal in the target or zero -- ties with either parity, their f32 neighbours, the
    smallest subnormal, half of it (a tie with zero) and the f32 next to that on either side; zero: +0 and -0; ordinary:
    normal(0, 0.02) draws, the size of the weight initialisation."""
    ebits, mbits = _FMT[dtype]
    drop = 23 - mbits
    half = 1 << (drop - 1)
    bias = (1 << (ebits - 1)) - 1
    emin = 1 - bias                                                        # exponent of the smallest normal of the target
    out = {}
    # normal-range ties: f32 exponent fields across the target's normal range (well inside it), a few significands of either parity
    exps = [127 - 6, 127 - 1, 127, 127 + 3, 127 + emin + 1, 127 + bias - 1]
    sig_even = [0, 2 << drop, ((1 << mbits) - 2) << drop]                  # kept significand even: the tie rounds down to it
    sig_odd = [1 << drop, 3 << drop, ((1 << mbits) - 1) << drop]           # kept significand odd: the tie rounds up (carry into the exponent for the last)
    def ties(sigs):
        return np.array([(e << 23) | s | half for e in exps for s in sigs], dtype=np.uint32)
    both = lambda b: np.concatenate([b, b | np.uint32(0x80000000)])
    below, above = ties(sig_even), ties(sig_odd)
    out["tie_even_below"] = _f32(both(below))
    out["tie_even_above"] = _f32(both(above))
    allt = np.concatenate([below, above])
    out["tie_minus_ulp"] = _f32(both(allt - np.uint32(1)))
    out["tie_plus_ulp"] = _f32(both(allt + np.uint32(1)))
    top = np.uint32(((127 + bias) << 23) | (((1 << mbits) - 1) << drop))    # largest finite value of the target, as f32 bits
    out["max_finite"] = _f32(both(np.array([top, top | np.uint32(half - 1)], dtype=np.uint32)))
    out["first_to_inf"] = _f32(both(np.array([top | np.uint32(half), (top | np.uint32(half)) + np.uint32(1)], dtype=np.uint32)))
    # subnormal results: the target's subnormals are k * q, q = 2^(emin - mbits), 0 < k < 2^mbits
    q = np.float64(2.0) ** (emin - mbits)
    ks = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 100.5, 101.5, (1 << mbits) - 1.5, (1 << mbits) - 1.0, (1 << mbits) - 0.5])
    sub = (ks * q).astype(np.float32)
    assert np.array_equal(sub.astype(np.float64), ks * q)                 # every k q is an f32 value (an f32 subnormal for bf16)
    sb = sub.view(np.uint32)
    nb = np.concatenate([sb, sb - np.uint32(1), sb + np.uint32(1)])
    out["subnormal"] = _f32(both(nb))
    out["zero"] = _f32(np.array([0, 0x80000000], dtype=np.uint32))
    out["ordinary"] = (0.02 * np.random.default_rng(seed).standard_normal(n_ordinary)).astype(np.float32)
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    return out


def rounding_tensor(dtype, shape, seed=0):
    """float32 tensor of `shape` made of the rounding vectors of `dtype` (f32: those of both 16-bit types; its cast is the
    identity): every special value at least once, about half of the elements ordinary weights, shuffled with a fixed seed."""
    n = int(np.prod(shape))
    kinds = [torch.bfloat16, torch.float16] if dtype == torch.float32 else [dtype]
    special = np.concatenate([v for dt in kinds for k, v in rounding_vectors(dt).items() if k != "ordinary"])
    assert n >= special.size, (n, special.size)
    rng = np.random.default_rng(seed)
    reps = max(1, n // (2 * special.size))
    body = np.tile(special, reps)
    rest = (0.02 * rng.standard_normal(n - body.size)).astype(np.float32)
    flat = np.concatenate([body, rest])[rng.permutation(n)]
    return torch.from_numpy(flat.copy()).reshape(shape)


# ----------------------------------------------------------------------------------------------------------------------
# OCP e4m3fn
# ----------------------------------------------------------------------------------------------------------------------
def e4m3_encode(x):
    """uint8 codes of float32 `x` in OCP e4m3fn: sign, 4 exponent bits (bias 7), 3 significand bits; subnormals k * 2^-9; round
    to nearest, ties to the even code; magnitudes that would round past 448 (code 0x7E) saturate to it.  Finite input only.
    Every step is exact in float64: x, x * 2^9 and (x / 2^e - 1) * 8 carry at most 24 significant bits."""
    x = np.asarray(x, dtype=np.float32)
    assert np.isfinite(x).all()
    sign = (x.view(np.uint32) >> 24).astype(np.uint8) & np.uint8(0x80)
    a = np.abs(x).astype(np.float64)
    sub = np.rint(np.minimum(a, 1.0) * 512.0)                                         # below 2^-6: units of 2^-9 (rint: half to even); 8 = code 0x08 = 2^-6
    m, e = np.frexp(np.where(a > 0, a, 1.0))                               # a = m 2^e, m in [0.5, 1)  ->  (2 m) 2^(e - 1)
    e = e.astype(np.int64) - 1
    qn = np.rint((2.0 * m - 1.0) * 8.0).astype(np.int64)                   # 0..8; 8 carries into the exponent: code arithmetic does it
    code_n = ((e + 7) << 3) + qn
    code = np.where(a < 2.0 ** -6, sub.astype(np.int64), code_n)
    code = np.minimum(code, 0x7E)
    return (code.astype(np.uint8) | sign)


def e4m3_decode(codes):
    """float32 values of uint8 e4m3fn codes (0x7F / 0xFF: NaN)."""
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7).astype(np.float64))
    mag = np.where((c & 0x7F) == 0x7F, np.nan, mag)
    return (np.where(c & 0x80, -mag, mag)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# the pack call into a guarded buffer (GPU)
# ----------------------------------------------------------------------------------------------------------------------
def pack_guarded(ops, Lb, d, which, w, fill_byte=0xFF, into=None):
    """p2phd_conv_pack_weights of the master tensor `w` (device, float32, in the layout d.w_layout names) into a guarded buffer
    of exactly p2phd_conv_packed_bytes, prefilled with `fill_byte` (or into the guarded buffer `into` as it is).  Synchronises;
    the caller checks the guards."""
    import ctypes as C
    nbytes = Lb.p2phd_conv_packed_bytes(C.byref(d), which)
    assert nbytes > 0, ("conv_packed_bytes", which)
    g = into if into is not None else X.guarded(nbytes, fill_byte=fill_byte)
    assert g.nbytes == nbytes
    ops.check(Lb.p2phd_conv_pack_weights(C.byref(d), which, ops.ptr(w), C.c_void_p(g.ptr()), ops.stream_ptr()), "conv_pack_weights")
    torch.cuda.synchronize()
    return g


def pack_guarded_fp8(ops, Lb, d, w, fill_byte=0xFF, into=None):
    """The same for p2phd_conv_fp8_pack_weights / p2phd_conv_fp8_packed_bytes."""
    import ctypes as C
    nbytes = Lb.p2phd_conv_fp8_packed_bytes(C.byref(d))
    assert nbytes > 0, "conv_fp8_packed_bytes"
    g = into if into is not None else X.guarded(nbytes, fill_byte=fill_byte)
    assert g.nbytes == nbytes
    ops.check(Lb.p2phd_conv_fp8_pack_weights(C.byref(d), ops.ptr(w), C.c_void_p(g.ptr()), ops.stream_ptr()), "conv_fp8_pack_weights")
    torch.cuda.synchronize()
    return g
