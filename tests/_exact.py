"""Exact integer-operand checks of the conv kernels: operands, CPU references and bit-level comparison.

Why integers.  Every 16-bit (and e4m3) conv kernel multiplies its operands exactly and accumulates in fp32.  With
small-integer operands every product and every partial sum -- in any order, with any split-K, through any 16-bit
intermediate -- is an integer, and an integer n is held exactly by fp32 for |n| < 2^24, by bf16 (8 significand bits) for
|n| <= 256 and by fp16 (11 bits) for |n| <= 2048.  So as long as the LARGEST POSSIBLE magnitude of any partial sum,
`abs_bound` = the same operation on |x|, |w|, |b| (+ |addend|), stays inside the format, no rounding happens anywhere and
the only correct output is one bit pattern per element.  Three conditions are asserted on the reference alone, on the CPU,
before a case touches the GPU (`operands`):
  1. abs_bound <= 256 where the output (or an intermediate of the path) is stored in 16 bits -- the bf16 limit is used for
     the fp16 library and the fp32 mode as well, so one set of operands serves all three --, < 2^24 for fp32 outputs (dw, db);
  2. at least half of the expected outputs are non-zero;
  3. every tap position (r, s), every input channel and every output channel carries a non-zero weight (a dropped tap or
     channel cannot hide behind zeros).
A zero is the integer 0 whatever its sign bit: `x * 0.f` (a ReLU slope) gives -0.0 for negative x, so the sign of zero is
canonicalised on both sides before the bit comparison; every other element is compared bit for bit.

This module is a plain helper (no fixtures, no test functions); tests/test_exact_helper.py checks it on the CPU.
"""
import collections
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                     # unit roundoff of fp32
LIMIT16 = 256                        # largest |integer| for which every integer below is a bf16 value (fp16: 2048)
LIMIT32 = 2 ** 24
ADDEND_MAX = 3                       # largest |integer| of a dgrad addend

Layer = collections.namedtuple("Layer", "name cin cout k stride pad pad_mode transposed opad shape")


def L(name, cin, cout, k, stride, pad, pad_mode, transposed, opad, shape):
    return Layer(name, cin, cout, k, stride, pad, pad_mode, bool(transposed), opad, tuple(shape))


# ----------------------------------------------------------------------------------------------------------------------
# The case table: family -> layers.  Geometries are those the existing tests reach each family with (their comments and the
# route functions of csrc/convapi.hip state the eligibility rules), plus the smallest eligible plane, odd / ragged ones
# and batches where an M tile straddles two samples.  `calls`: which references the GPU module needs ("fwd", "dgrad",
# "dgrad_add", "wgrad"); the CPU test checks exactly these.
# ----------------------------------------------------------------------------------------------------------------------
GENERIC = [
    L("wide_k200_c136", 136, 200, 3, 1, 1, 1, 0, 0, (1, 12, 12)),        # > 1 N tile, K not / 64
    L("big_m_tiles", 8, 8, 3, 1, 1, 0, 0, 0, (2, 40, 33)),               # 1320-pixel planes: an M tile straddles the two samples
    L("c3_s2_odd", 16, 24, 3, 2, 1, 0, 0, 0, (1, 15, 9)),
    L("ct3_s2", 16, 8, 3, 2, 1, 0, 1, 1, (2, 5, 7)),
    L("c4_s2", 8, 16, 4, 2, 2, 0, 0, 0, (2, 9, 7)),
    L("c4_s1", 16, 32, 4, 1, 2, 0, 0, 0, (2, 5, 4)),
    L("c3_reflect_2x2", 32, 32, 3, 1, 1, 1, 0, 0, (2, 2, 2)),            # smallest reflect plane (padded grid + fold)
    L("c3_reflect_6x5", 16, 16, 3, 1, 1, 1, 0, 0, (2, 6, 5)),            # exact-grid reflect gradient and its generic form
    L("cfold_c3", 3, 24, 5, 1, 2, 0, 0, 0, (1, 11, 13)),                 # C = 3: input W-fold
    L("kfold_k3", 8, 3, 7, 1, 3, 1, 0, 0, (2, 14, 19)),                  # K = 3: output W-fold, reflect
    L("kfold_c4_k4", 4, 4, 3, 1, 1, 0, 0, 0, (2, 9, 11)),                # both tiny
    L("tile_72to384", 72, 384, 3, 1, 1, 1, 0, 0, (2, 18, 16)),           # 384 = 2 x 192: every forced tile height applies
    L("tile_64to64_s2", 64, 64, 4, 2, 2, 0, 0, 0, (2, 34, 30)),
]
HALO_FWD = [
    L("trunk_768", 768, 768, 3, 1, 1, 1, 0, 0, (27, 32, 16)),            # the benchmarked layer (256 x 192 tiles from N = 27)
    L("halo_64to768_rows16", 64, 768, 3, 1, 1, 1, 0, 0, (56, 16, 16)),   # one tile holds both borders
    L("halo_64to768_rows48", 64, 768, 3, 1, 1, 1, 0, 0, (19, 48, 16)),   # a tile with neither border
    L("halo_64to768_rows96", 64, 768, 3, 1, 1, 1, 0, 0, (10, 96, 16)),
    L("halo_64to768_b16", 64, 768, 3, 1, 1, 1, 0, 0, (16, 32, 16)),      # 256 x 128 tiles
]
HALO_DGRAD = [                                                          # input gradient through the reflection extras: GEMM N = C
    L("trunk_768", 768, 768, 3, 1, 1, 1, 0, 0, (27, 32, 16)),
    # (K wide enough for the plane to take the single-launch InstanceNorm backward, the only writer of extras: N * ceil(K / 32) >= 128)
    L("halo_768to128_rows16", 768, 128, 3, 1, 1, 1, 0, 0, (56, 16, 16)),
    L("halo_768to256_b16", 768, 256, 3, 1, 1, 1, 0, 0, (16, 32, 16)),
]
TILE128X192_FWD = L("t128x192_192to1536", 192, 1536, 3, 1, 1, 1, 0, 0, (32, 16, 8))
# (input gradient: a 128-pixel plane reaches this tile only with per-sample tiles, i.e. with the fused InstanceNorm-backward sums,
# which zero-padded layers have: gconv.hip gconv_choose_tile, `flat_m`)
TILE128X192_DGRAD = L("t128x192_1152to64", 1152, 64, 3, 1, 1, 0, 0, 0, (32, 16, 8))
SPLITK = [
    L("c3_64to96", 64, 96, 3, 1, 1, 1, 0, 0, (3, 40, 28)),
    L("d_256to512_n5", 256, 512, 4, 1, 2, 0, 0, 0, (5, 34, 18)),         # (at N = 9 the tail round holds 216 of 256 CUs' tiles: nothing to split)
    L("c3s2_odd_128", 128, 128, 3, 2, 1, 0, 0, 0, (5, 33, 47)),
]
TILE256 = L("d_256to512", 256, 512, 4, 1, 2, 0, 0, 0, (9, 34, 18))       # the 256 x 256 tile (gconv_bm = 512)
CLS_SKIP_FWD = [L("skip_ct_192to96", 192, 96, 3, 2, 1, 0, 1, 1, (8, 64, 64)),      # class pitch 96: two classes per tile
                L("skip_ct_384to192", 384, 192, 3, 2, 1, 0, 1, 1, (4, 64, 64))]    # class pitch 192: one
CLS_SKIP_DGRAD = [L("skip_s2_96to192", 96, 192, 3, 2, 1, 0, 0, 0, (8, 128, 128))]
MARCH_CONV = [L("march_s_1strip", 48, 96, 3, 2, 1, 0, 0, 0, (2, 16, 128)),
              L("march_s_2strips", 48, 96, 3, 2, 1, 0, 0, 0, (1, 24, 256)),
              L("march_s_512x256", 48, 96, 3, 2, 1, 0, 0, 0, (1, 512, 256))]
MARCH_CONVT = [L("march_ct_1strip", 96, 48, 3, 2, 1, 0, 1, 1, (2, 8, 64)),
               L("march_ct_2strips", 96, 48, 3, 2, 1, 0, 1, 1, (1, 12, 128)),
               L("march_ct_256x128", 96, 48, 3, 2, 1, 0, 1, 1, (1, 256, 128))]
THIN = [L("thin_2to48", 2, 48, 7, 1, 3, 1, 0, 0, (2, 16, 128)),
        L("thin_48to2", 48, 2, 7, 1, 3, 1, 0, 0, (2, 16, 128)),
        L("thin_4to64", 4, 64, 4, 2, 2, 0, 0, 0, (3, 37, 50))]
WGRAD = [L("wgrad_rows256", 72, 256, 3, 1, 1, 1, 0, 0, (2, 10, 9)),
         L("ct_wgrad_rows256", 256, 40, 3, 2, 1, 0, 1, 1, (1, 6, 7)),
         L("wgrad_c3_s2_odd", 16, 24, 3, 2, 1, 0, 0, 0, (1, 15, 9)),
         L("wgrad_kfold_k3", 8, 3, 7, 1, 3, 1, 0, 0, (2, 14, 19)),
         L("wgrad_cfold_c3", 3, 24, 5, 1, 2, 0, 0, 0, (1, 11, 13))]
WGRAD_KMAJOR = [L("trunk_768_n2", 768, 768, 3, 1, 1, 1, 0, 0, (2, 32, 16)),
                L("kmajor_128to64_k4", 128, 64, 4, 1, 2, 0, 0, 0, (2, 9, 7))]
DFIRST = [L("dfirst_c4", 4, 64, 4, 2, 2, 0, 0, 0, (4, 256, 128)),
          L("dfirst_c3_odd", 3, 64, 4, 2, 2, 0, 0, 0, (3, 37, 51)),
          L("dfirst_c1_tiny", 1, 64, 4, 2, 2, 0, 0, 0, (1, 5, 3)),
          L("dfirst_c2", 2, 64, 4, 2, 2, 0, 0, 0, (2, 16, 24)),
          L("dfirst_c8", 8, 64, 4, 2, 2, 0, 0, 0, (3, 37, 51))]
DLAST = [L("dlast_512", 512, 1, 4, 1, 2, 0, 0, 0, (6, 33, 17)),
         L("dlast_128_tiny", 128, 1, 4, 1, 2, 0, 0, 0, (2, 3, 5)),
         L("dlast_384", 384, 1, 4, 1, 2, 0, 0, 0, (1, 40, 36)),
         L("dlast_256", 256, 1, 4, 1, 2, 0, 0, 0, (2, 9, 23))]
C7_IN = [L("c7_2to48", 2, 48, 7, 1, 3, 1, 0, 0, (2, 16, 128)),
         L("c7_2to96", 2, 96, 7, 1, 3, 1, 0, 0, (1, 8, 256)),
         L("c7_2to32", 2, 32, 7, 1, 3, 1, 0, 0, (1, 24, 128))]
C7_OUT = [L("c7_48to2", 48, 2, 7, 1, 3, 1, 0, 0, (2, 16, 128)),
          L("c7_96to2", 96, 2, 7, 1, 3, 1, 0, 0, (1, 8, 256)),
          L("c7_32to2", 32, 2, 7, 1, 3, 1, 0, 0, (1, 24, 128))]
FP8 = [L("trunk256", 256, 256, 3, 1, 1, 1, 0, 0, (2, 32, 16)),
       L("d256to512", 256, 512, 4, 1, 2, 0, 0, 0, (2, 17, 9))]

# Small layers that reach the edges of the weight-pack kernels (csrc/wpack.hip; tests/test_gpu_wpack.py says which edge each one
# is for).  The pack does not depend on the plane; these run forward and input gradient once on a pack into poisoned memory.
WPACK = [L("wp_c72_k6", 72, 6, 3, 1, 1, 0, 0, 0, (1, 6, 5)),              # inner 72: a partly filled 64-column block; rows 6 / 72
         L("wp_c2_k37_s2", 2, 37, 3, 2, 1, 0, 0, 0, (1, 9, 8)),           # C = 2: Cp = 8 > inner; rows 37; stride 2 keeps it off the W-fold
         L("wp_c24_k7_2x2", 24, 7, 2, 1, 0, 0, 0, 0, (1, 6, 5)),          # 4 taps: a K tail behind taps * Cp
         L("wp_c24_k72", 24, 72, 3, 1, 1, 1, 0, 0, (1, 5, 6)),            # input gradient: rows 24 = 1.5 bricks of 16, inner 72
         L("wp_c5_k6_7x7", 5, 6, 7, 1, 3, 0, 0, 0, (1, 8, 9)),            # 49 taps, no W-fold (S * C = 35 > 32): the tap walk wraps its batches of 16
         L("wp_kmajor_c64_k72", 64, 72, 3, 1, 1, 1, 0, 0, (1, 6, 5))]     # K-major eligible; K = 72 and rows_pad = 128 > C: tiles that hang over


def at_batch(layer, n):
    return layer._replace(name=f"{layer.name}_n{n}", shape=(n,) + layer.shape[1:])


# (layer, calls) of everything the GPU module runs: the CPU test walks this list
def case_table():
    t = []
    t += [(l, ("fwd", "dgrad", "dgrad_add")) for l in GENERIC]
    t += [(l, ("fwd",)) for l in HALO_FWD] + [(l, ("dgrad", "dgrad_add")) for l in HALO_DGRAD]
    t += [(TILE128X192_FWD, ("fwd",)), (TILE128X192_DGRAD, ("dgrad",))]
    t += [(l, ("fwd", "dgrad")) for l in SPLITK + [TILE256]]
    t += [(l, ("fwd",)) for l in CLS_SKIP_FWD] + [(at_batch(l, 1), ("fwd",)) for l in CLS_SKIP_FWD]
    t += [(l, ("dgrad",)) for l in CLS_SKIP_DGRAD] + [(at_batch(l, 1), ("dgrad",)) for l in CLS_SKIP_DGRAD]
    t += [(l, ("fwd", "dgrad", "wgrad")) for l in MARCH_CONV + MARCH_CONVT]
    t += [(l, ("wgrad",)) for l in THIN + WGRAD + WGRAD_KMAJOR]
    t += [(at_batch(l, 2), ("fwd", "dgrad", "dgrad_add")) for l in WGRAD_KMAJOR]
    t += [(l, ("fwd",)) for l in DFIRST + C7_IN]
    t += [(l, ("fwd", "dgrad", "dgrad_add")) for l in DLAST]
    t += [(l, ("fwd", "dgrad")) for l in C7_OUT]
    t += [(l, ("fwd8",)) for l in FP8]
    t += [(l, ("fwd", "dgrad")) for l in WPACK]
    return t


# ----------------------------------------------------------------------------------------------------------------------
# integer tensors and references
# ----------------------------------------------------------------------------------------------------------------------
def int_tensor(shape, lo, hi, density, gen):
    """float32 tensor of integers drawn uniformly from [lo, hi] without 0, each element non-zero with probability `density`."""
    mag = torch.randint(lo, hi + 1, shape, generator=gen)
    if lo <= 0 <= hi:                                                  # re-draw the zeros of the value draw: density is the mask's alone
        alt = torch.where(torch.rand(shape, generator=gen) < 0.5, torch.full(shape, lo), torch.full(shape, hi))
        mag = torch.where(mag == 0, alt, mag)
    keep = torch.rand(shape, generator=gen) < density
    return (mag * keep).to(torch.float32)


def out_hw(l):
    N, H, W = l.shape
    if l.transposed:
        return (H - 1) * l.stride - 2 * l.pad + l.k + l.opad, (W - 1) * l.stride - 2 * l.pad + l.k + l.opad
    return (H + 2 * l.pad - l.k) // l.stride + 1, (W + 2 * l.pad - l.k) // l.stride + 1


def w_shape(l):
    return (l.cin, l.cout, l.k, l.k) if l.transposed else (l.cout, l.cin, l.k, l.k)


def conv_reference(l, x, w, b):
    """conv(x) + b of the layer (NCHW, PyTorch weight layout), in the dtype of the arguments (float32 or float64)."""
    if l.transposed:
        return F.conv_transpose2d(x, w, b, stride=l.stride, padding=l.pad, output_padding=l.opad)
    if l.pad_mode:
        return F.conv2d(F.pad(x, (l.pad,) * 4, mode="reflect"), w, b, stride=l.stride)
    return F.conv2d(x, w, b, stride=l.stride, padding=l.pad)


def _reflect_pad_adjoint(gp, pad):
    """Adjoint of F.pad(., reflect) applied to gp [N, C, H + 2 pad, W + 2 pad], through F.pad's own autograd."""
    N, C, Hp, Wp = gp.shape
    z = torch.zeros(N, C, Hp - 2 * pad, Wp - 2 * pad, dtype=gp.dtype, requires_grad=True)
    (g,) = torch.autograd.grad(F.pad(z, (pad,) * 4, mode="reflect"), z, gp)
    return g


def dgrad_reference(l, dy, w, addend=None):
    """Gradient with respect to the layer's input of <conv(x), dy>, (+ addend)."""
    N, H, W = l.shape
    if l.transposed:                                                   # adjoint of conv_transpose2d(., w) = conv2d(., w)
        dx = F.conv2d(dy, w, stride=l.stride, padding=l.pad)
    else:
        P = l.pad if l.pad_mode else 0
        Hp, Wp = H + 2 * P, W + 2 * P
        p = 0 if l.pad_mode else l.pad
        oh = Hp - ((dy.shape[2] - 1) * l.stride - 2 * p + l.k)
        ow = Wp - ((dy.shape[3] - 1) * l.stride - 2 * p + l.k)
        dx = F.conv_transpose2d(dy, w, stride=l.stride, padding=p, output_padding=(oh, ow))
        if l.pad_mode:
            dx = _reflect_pad_adjoint(dx, l.pad)
    assert tuple(dx.shape) == (N, l.cin, H, W), (l.name, tuple(dx.shape))
    return dx if addend is None else dx + addend


def wgrad_reference(l, x, dy):
    """(dw in the PyTorch layout of the layer's weight, db) of <conv(x) + b, dy>."""
    if l.transposed:                                                   # <convT(x, w), dy> = <x, conv2d(dy, w)>
        dw = torch.nn.grad.conv2d_weight(dy, w_shape(l), x, stride=l.stride, padding=l.pad)
    elif l.pad_mode:
        dw = torch.nn.grad.conv2d_weight(F.pad(x, (l.pad,) * 4, mode="reflect"), w_shape(l), dy, stride=l.stride)
    else:
        dw = torch.nn.grad.conv2d_weight(x, w_shape(l), dy, stride=l.stride, padding=l.pad)
    return dw, dy.sum((0, 2, 3))


def abs_bound(l, call, ops):
    """Largest possible magnitude of any partial sum of `call`: the same operation on the magnitudes of its operands
    (the weight gradient's includes the `_acc` prefill)."""
    a = {k: (v.abs() if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}
    if call in ("fwd", "fwd8"):
        return float(conv_reference(l, a["x"], a["w"], a["b"]).max())
    if call in ("dgrad", "dgrad_add"):
        return float(dgrad_reference(l, a["dy"], a["w"], a.get("addend")).max())
    dw, db = wgrad_reference(l, a["x"], a["dy"])
    return float(max((dw + a["dw0"]).max(), (db + a["db0"]).max()))


def _cover(w, gen):
    """Condition 3: a non-zero weight at every tap position, in every row and in every column of the [d0, d1] channel grid."""
    d0, d1, R, S = w.shape
    for r in range(R):
        for s in range(S):
            if not w[:, :, r, s].any():
                w[(r * S + s) % d0, (r * S + s) % d1, r, s] = 1.0
    for i in range(d0):
        if not w[i].any():
            w[i, i % d1, i % R, i % S] = -1.0
    for j in range(d1):
        if not w[:, j].any():
            w[j % d0, j, j % R, (j + 1) % S] = 1.0
    return w


def covers(w):
    return bool(w.ne(0).sum((0, 1)).all() and w.ne(0).sum((1, 2, 3)).all() and w.ne(0).sum((0, 2, 3)).all())


_DENSITIES = (0.5, 0.35, 0.25, 0.18, 0.13, 0.09, 0.065, 0.045, 0.03, 0.02)


def _draw(l, call, dens, seed):
    gen = torch.Generator().manual_seed(seed)
    N, H, W = l.shape
    Ho, Wo = out_hw(l)
    ops = {}
    if call == "fwd8":          # x: integers in -8..8 (e4m3 values); w / scale must be e4m3 values at scale max|w| / 448 = 2^-6
        ops["x"] = int_tensor((N, l.cin, H, W), -8, 8, dens, gen)
        # (mostly +-1: the 4096-deep reduction of the 4 x 4 layer has to stay inside 256 with half of the outputs non-zero)
        mag = torch.tensor([1., 2., 4., 7.])[torch.multinomial(torch.tensor([0.85, 0.08, 0.05, 0.02]), int(np.prod(w_shape(l))), True,
                                                               generator=gen)].reshape(w_shape(l))
        sign = torch.where(torch.rand(w_shape(l), generator=gen) < 0.5, -1.0, 1.0)
        w = mag * sign * (torch.rand(w_shape(l), generator=gen) < dens)
        w = _cover(w, gen)
        w[0, 0, 0, 0] = 7.0
        ops["w"], ops["b"] = w, int_tensor((l.cout,), -2, 2, 1.0, gen)
        return ops
    ops["w"] = _cover(int_tensor(w_shape(l), -1, 1, dens, gen), gen)
    if call == "fwd":
        ops["x"] = int_tensor((N, l.cin, H, W), -2, 2, dens, gen)
        ops["b"] = int_tensor((l.cout,), -2, 2, 1.0, gen)
    elif call == "dgrad":
        ops["dy"] = int_tensor((N, l.cout, Ho, Wo), -2, 2, dens, gen)
    else:                        # wgrad: fp32 outputs, dense operands; integer prefill of the accumulating entry point
        del ops["w"]
        ops["x"] = int_tensor((N, l.cin, H, W), -2, 2, 0.5, gen)
        ops["dy"] = int_tensor((N, l.cout, Ho, Wo), -2, 2, 0.5, gen)
        ops["dw0"] = int_tensor(w_shape(l), -5, 5, 1.0, gen)
        ops["db0"] = int_tensor((l.cout,), -5, 5, 1.0, gen)
    return ops


def _head(l, ops, n):
    """The first n samples of a case (density search on a part of a large batch; the assertion is on the whole)."""
    sub = {k: (v[:n] if isinstance(v, torch.Tensor) and v.dim() == 4 and k in ("x", "dy", "addend") else v) for k, v in ops.items()}
    return l._replace(shape=(n,) + l.shape[1:]), sub


def reference(l, call, ops, dtype=torch.float32):
    """Expected result(s) of `call` in `dtype`: y / dx (NCHW), or (dw + dw0, db + db0)."""
    c = {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in ops.items()}
    if call in ("fwd", "fwd8"):
        return conv_reference(l, c["x"], c["w"], c["b"])
    if call in ("dgrad", "dgrad_add"):
        return dgrad_reference(l, c["dy"], c["w"], c.get("addend"))
    dw, db = wgrad_reference(l, c["x"], c["dy"])
    return dw + c["dw0"], db + c["db0"]


_CACHE = {}


def operands(l, call):
    """Deterministic integer operands of (layer, call) that meet the three conditions, with the float32 reference:
    dict(ops..., want=..., bound=..., density=...).  The densest entry of _DENSITIES whose abs_bound fits is taken -- a
    choice made from the reference alone; the conditions are asserted on what is returned."""
    key = (l, call)
    if key in _CACHE:
        return _CACHE[key]
    if call == "dgrad_add":      # the operands of "dgrad" plus an integer addend: dx + addend, bound = max(|dx|-bound + |addend|)
        base = operands(l, "dgrad")
        gen = torch.Generator().manual_seed(zlib.crc32(f"{l.name}/addend".encode()))
        addend = int_tensor(tuple(base["want"].shape), -ADDEND_MAX, ADDEND_MAX, 0.7, gen)
        out = {k: v for k, v in base.items() if k != "abs"}
        out.update(addend=addend, want=base["want"] + addend, bound=float((base["abs"] + addend.abs()).max()))
        check_conditions(l, call, out, out["want"], out["bound"])
        _CACHE[key] = out
        return out
    limit = LIMIT32 - 1 if call == "wgrad" else (LIMIT16 - ADDEND_MAX if call == "dgrad" else LIMIT16)
    fwd = call in ("fwd", "fwd8")
    gathers = l.stride == 1 or (fwd != l.transposed)                # a stride-2 scatter direction sees about a quarter of the taps
    depth = (l.k * l.k if gathers else (l.k * l.k + 3) // 4) * (l.cin if fwd else l.cout)
    seed = zlib.crc32(f"{l.name}/{call}".encode())
    chosen = None
    for dens in ((0.5,) if call == "wgrad" else _DENSITIES):
        if call != "wgrad" and depth * dens * dens > 1.5 * limit:      # shortcut only: the mean alone (E|x| >= 1.5, |w| = 1) is far outside
            continue
        ops = _draw(l, call, dens, seed)
        if l.shape[0] > 2 and call != "wgrad":
            hl, hops = _head(l, ops, 1)
            if abs_bound(hl, call, hops) > limit:
                continue
        bound = abs_bound(l, call, ops)
        if bound <= limit:
            chosen = (ops, bound, dens)
            break
    assert chosen is not None, f"{l.name}/{call}: no density keeps the partial sums exact"
    ops, bound, dens = chosen
    want = reference(l, call, ops)
    check_conditions(l, call, ops, want, bound)
    out = dict(ops, want=want, bound=bound, density=dens)
    if call == "dgrad":
        out["abs"] = dgrad_reference(l, ops["dy"].abs(), ops["w"].abs())
    if len(_CACHE) > 4:
        _CACHE.clear()
    _CACHE[key] = out
    return out


def check_conditions(l, call, ops, want, bound):
    limit = LIMIT32 - 1 if call == "wgrad" else LIMIT16
    assert bound <= limit, (l.name, call, bound)
    for t in (want if isinstance(want, tuple) else (want,)):
        assert torch.equal(t, t.round()), (l.name, call, "reference is not integer valued")
        share = float(t.ne(0).float().mean())
        assert share >= 0.5, (l.name, call, "non-zero share of the expected output", share)
    if "w" in ops:
        assert covers(ops["w"]), (l.name, call, "a tap or a channel has no non-zero weight")
    else:                        # weight gradient: every tap / channel of dw is hit when x and dy are dense; checked on the result
        assert covers(want[0] - ops["dw0"]), (l.name, call, "a tap or a channel of dw is zero")


# ----------------------------------------------------------------------------------------------------------------------
# physical layout, bit comparison
# ----------------------------------------------------------------------------------------------------------------------
def cpitch(c):
    return (c + 7) & ~7


def to_nhwc(t, dtype):
    """NCHW float -> physical NHWC [N, H, W, Cp] in `dtype`, pad channels +0 (host tensor)."""
    N, C, H, W = t.shape
    out = torch.zeros(N, H, W, cpitch(C), dtype=torch.float32)
    out[..., :C] = t.permute(0, 2, 3, 1)
    return out.to(dtype)


def _bits(t):
    t = t.contiguous()
    t = torch.where(t == 0, torch.zeros_like(t), t)                   # -0 -> +0: the integer 0 (module docstring)
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _hist(idx, mod=None, top=8):
    v = idx if mod is None else idx % mod
    u, c = np.unique(v, return_counts=True)
    order = np.argsort(-c)[:top]
    return {int(u[i]): int(c[i]) for i in sorted(order, key=lambda i: u[i])}


def assert_bits_equal(got, want, layout, what):
    """`got`: the whole physical tensor as the kernel left it (host copy).  `want`: the integer reference --
    layout "nhwc": got [N, H, W, Cp], want NCHW [N, C, H, W] (valid channels = the integer, pad channels = +0);
    layout "flat": same shape as got (weight gradients, NCHW outputs).  Compares bit patterns of every element.  The failure
    message says where: count, the first few (n, h, w, c, got, want), and histograms of the differing elements over h, w, n
    and c mod 8 / 32 / 64 -- a border row, a tile seam or a sample boundary is readable from it."""
    got = got.detach().cpu()
    if layout == "nhwc":
        exp = to_nhwc(want.to(torch.float32), got.dtype)
    else:
        exp = want.to(got.dtype).reshape(got.shape)
    assert tuple(got.shape) == tuple(exp.shape), (what, tuple(got.shape), tuple(exp.shape))
    diff = _bits(got).ne(_bits(exp))
    n = int(diff.sum())
    if n == 0:
        return
    idx = diff.nonzero().numpy()
    g, e = got.float()[diff].numpy(), exp.float()[diff].numpy()
    if layout == "nhwc":
        names = ("n", "h", "w", "c")
        first = [tuple(int(v) for v in idx[i]) + (float(g[i]), float(e[i])) for i in range(min(8, n))]
        c = idx[:, 3]
        hist = {"h": _hist(idx[:, 1]), "w": _hist(idx[:, 2]), "n": _hist(idx[:, 0]), "c%8": _hist(c, 8), "c%32": _hist(c, 32),
                "c%64": _hist(c, 64), "pad_channels": int((c >= want.shape[1]).sum())}
    else:
        names = tuple(f"d{i}" for i in range(idx.shape[1]))
        first = [tuple(int(v) for v in idx[i]) + (float(g[i]), float(e[i])) for i in range(min(8, n))]
        hist = {nm: _hist(idx[:, i]) for i, nm in enumerate(names)}
    raise AssertionError(f"{what}: {n} of {diff.numel()} elements differ in their bits; first {names + ('got', 'want')}: {first}; "
                         f"histograms of differing elements: {hist}")


# ----------------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ----------------------------------------------------------------------------------------------------------------------
GUARD_BYTES = 4096
GUARD_BYTE = 0xA5


class Guarded:
    """`nbytes` of device memory with GUARD_BYTES of the byte GUARD_BYTE in front and right behind (no rounding of nbytes:
    a one-byte overrun shows).  `fill_byte`: prefill of the payload (0xFF: NaN in every float type, for scratch)."""

    def __init__(self, nbytes, device="cuda", fill_byte=0xFF):
        self.nbytes = int(nbytes)
        self.raw = torch.full((self.nbytes + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.bytes = self.raw[GUARD_BYTES:GUARD_BYTES + self.nbytes]
        self.bytes.fill_(fill_byte)

    def view(self, dtype, shape):
        return self.bytes.view(dtype).view(shape)

    def ptr(self):
        return self.raw.data_ptr() + GUARD_BYTES

    def touched(self):
        lo = self.raw[:GUARD_BYTES].ne(GUARD_BYTE).nonzero().flatten()
        hi = self.raw[GUARD_BYTES + self.nbytes:].ne(GUARD_BYTE).nonzero().flatten()
        return [int(v) - GUARD_BYTES for v in lo.tolist()[:4]] + [self.nbytes + int(v) for v in hi.tolist()[:4]]


def guarded(nbytes, device="cuda", fill_byte=0xFF):
    return Guarded(nbytes, device, fill_byte)


def guarded_like(shape, dtype, device="cuda", sentinel=0.7):
    """Guarded tensor pre-filled with a non-integer sentinel: an element the kernel does not write shows in the comparison."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    g = Guarded(n, device, 0)
    t = g.view(dtype, tuple(shape))
    t.fill_(sentinel)
    return g, t


def check_guards(bufs, what):
    for name, g in bufs.items():
        bad = g.touched()
        assert not bad, f"{what}: writes outside `{name}` ({g.nbytes} bytes) at byte offsets {bad}"


# ----------------------------------------------------------------------------------------------------------------------
# quantities that are NOT exact: bounds, derived
# ----------------------------------------------------------------------------------------------------------------------
def sum_bound(terms_abs_sum, P, extra=0):
    """Worst case of an fp32 sum of P terms in ANY order (per-wave partials, Chan merges, shuffle trees): each of the at most
    P - 1 additions rounds a partial sum that is bounded by sum|term|, relative error <= u = 2^-24 each; `+ 8` covers the
    division by the count / the final scalings of the merge, `extra` the roundings of each term itself (in units of u)."""
    return (P + 8 + extra) * U32 * terms_abs_sum


def stats_reference(y):
    """(mean, M2) per (n, c) of an NCHW integer tensor in float64, with the bounds of sum_bound: mean = sum of the P terms
    y / P, M2 = sum of the P terms (y - mean)^2."""
    y = y.double()
    P = y.shape[2] * y.shape[3]
    mean = y.mean((2, 3))
    dev2 = (y - mean[:, :, None, None]) ** 2
    return mean, dev2.sum((2, 3)), sum_bound(y.abs().sum((2, 3)) / P, P), sum_bound(dev2.sum((2, 3)), P)


# yhat of the fused InstanceNorm-backward sums (csrc/gconv.hip, store loop with GDesc::bs_out; the same formula in
# csrc/march.hip and csrc/dlast.hip): rstd = rsqrtf(fmaxf(M2 * inv_hw, 0) + eps), yh = (y - mean) * rstd.  With integer y and
# mean, y - mean is exact.  inv_hw = 1.f / (H * W): one rounding; M2 * inv_hw: one; + eps: one -> the argument is within 3 u,
# its inverse square root within 1.5 u; rsqrtf itself: 1 ulp = 2 u (HIP math API); the product with y - mean: one more.
# Together |yh / yh_exact - 1| <= 1.5 u + 2 u + u < 5 u; the term gp * yh adds one rounding: 6 u; YHAT_ULPS = 8 leaves the
# second-order terms room.  The branch yh > 0 is the sign of the exact y - mean: no rounding can move it.
YHAT_ULPS = 8


def bsum_reference(dx, prev_y, mean, m2, eps, slope):
    """(sum g', sum g' yhat) per (n, c) in float64 and their bounds; dx, prev_y NCHW, mean / m2 [N, C] (float32 values)."""
    P = dx.shape[2] * dx.shape[3]
    rstd = 1.0 / torch.sqrt(m2.double() / P + float(np.float32(eps)))
    yh = (prev_y.double() - mean.double()[:, :, None, None]) * rstd[:, :, None, None]
    gp = dx.double() * torch.where(yh > 0, 1.0, float(np.float32(slope)))
    s1, s2 = gp.sum((2, 3)), (gp * yh).sum((2, 3))
    return s1, s2, sum_bound(gp.abs().sum((2, 3)), P, 1), sum_bound((gp * yh).abs().sum((2, 3)), P, YHAT_ULPS)


def act_bwd_reference(g, x_act, slope, dtype):
    """p2phd_conv_dgrad_act's store (csrc/gconv.hip, store loop, `if (act_only)`):
    vv[e] = from_f<TO>(to_f(vv[e]) * (to_f(yy[e]) > 0.f ? 1.f : slope_b)) -- the stored (exact) gradient times 1 or the fp32
    slope, rounded once to fp32 by the multiplication and once to the storage type."""
    s = torch.where(x_act > 0, torch.ones((), dtype=torch.float32), torch.tensor(slope, dtype=torch.float32))
    return (g.to(torch.float32) * s).to(dtype)


# ----------------------------------------------------------------------------------------------------------------------
# reflection extras (csrc/norm.hip, in_act_bwd_fused_kernel `if (rx != nullptr)`; read by the pad_mode 3 gather of gconv.hip)
# ----------------------------------------------------------------------------------------------------------------------
def reflect_extras(dy):
    """Extras block of dy [N, H, W, Cp] (any float dtype, host) in float64: [N][2 (W + 2) + 2 H][Cp] --
    entries 0 .. 2 (W + 2): rows H = dy[0] + dy[2] and H + 1 = dy[H-3] + dy[H-1], W + 2 columns each, the last two being
    those rows' own pair sums (columns 0 + 2, W-3 + W-1); then columns W = dy[:, 0] + dy[:, 2] and W + 1 = dy[:, W-3] +
    dy[:, W-1] for rows < H, column-major."""
    d = dy.double()
    N, H, W, Cp = d.shape
    cols = torch.stack([d[:, :, 0] + d[:, :, 2], d[:, :, W - 3] + d[:, :, W - 1]], dim=1)          # [N, 2, H, Cp]
    wide = torch.cat([d, cols.permute(0, 2, 1, 3)], dim=2)                                           # [N, H, W + 2, Cp]
    rows = torch.stack([wide[:, 0] + wide[:, 2], wide[:, H - 3] + wide[:, H - 1]], dim=1)            # [N, 2, W + 2, Cp]
    return torch.cat([rows.reshape(N, 2 * (W + 2), Cp), cols.reshape(N, 2 * H, Cp)], dim=1)


def reflect_dgrad_from_extras(l, dy_nhwc, extras, w):
    """The input gradient as the pad_mode 3 gather forms it (csrc/gconv.hip gather table): a zero-padded transposed 3x3 conv of dy
    in which output row 1's tap onto row 2 reads virtual row H instead, output row H-2's tap onto row H-3 virtual row H + 1
    (columns likewise).  Host model, float64; used by the CPU test to pin the builder to the autograd reference."""
    N, H, W = l.shape
    d = dy_nhwc.double()[..., :l.cout]
    ex = extras[..., :l.cout]
    rows = ex[:, :2 * (W + 2)].reshape(N, 2, W + 2, l.cout)
    cols = ex[:, 2 * (W + 2):].reshape(N, 2, H, l.cout)
    big = torch.zeros(N, H + 2, W + 2, l.cout, dtype=torch.float64)
    big[:, :H, :W] = d
    big[:, H:, :] = rows
    big[:, :H, W:] = cols.permute(0, 2, 1, 3)
    wd = w.double()
    dx = torch.zeros(N, H, W, l.cin, dtype=torch.float64)
    for ho in range(H):
        for r in range(3):
            hi = ho + 1 - r
            if ho == 1 and hi == 2: hi = H
            elif ho == H - 2 and hi == H - 3: hi = H + 1
            elif hi >= H: hi = -1
            if hi < 0:
                continue
            for wo in range(W):
                for s in range(3):
                    wi = wo + 1 - s
                    if wo == 1 and wi == 2: wi = W
                    elif wo == W - 2 and wi == W - 3: wi = W + 1
                    elif wi >= W: wi = -1
                    if wi < 0:
                        continue
                    dx[:, ho, wo] += big[:, hi, wi] @ wd[:, :, r, s]
    return dx.permute(0, 3, 1, 2)
