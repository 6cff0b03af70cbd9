"""The helper of the exact integer-operand conv tests (tests/_exact.py), checked on the CPU: for every row of the case table the
float32 reference equals the float64 reference bit for bit, the three conditions hold (partial sums inside the format, half
of the outputs non-zero, every tap and channel weighted), and the input- / weight-gradient references equal torch autograd of
the forward reference.  Plus the sensitivity statement: corruptions of the kind an index bug makes, which the relative-L2
bounds of tests/test_gpu_conv.py let through, fail the bit comparison."""
import numpy as np
import pytest
import torch

import _exact as X
from conftest import rel_err

TABLE = X.case_table()


@pytest.mark.parametrize("layer,calls", TABLE, ids=[l.name + ":" + "+".join(c) for l, c in TABLE])
def test_reference_is_exact_and_meets_the_conditions(layer, calls):
    for call in calls:
        o = X.operands(layer, call)                                   # asserts the three conditions (check_conditions)
        ops = {k: v for k, v in o.items() if k not in ("want", "bound", "density", "abs")}
        want64 = X.reference(layer, call, ops, torch.float64)
        for a, b in zip(*[(t if isinstance(t, tuple) else (t,)) for t in (o["want"], want64)]):
            assert torch.equal(a.double(), b), (layer.name, call, "float32 reference != float64 reference")
        assert o["bound"] <= (X.LIMIT32 - 1 if call == "wgrad" else X.LIMIT16)
        # the gradient references against autograd of the forward reference (float64 on small layers, else float32: both exact)
        big = np.prod(layer.shape) * layer.cin * layer.cout * layer.k ** 2 > 2e9
        dt = torch.float32 if big else torch.float64
        if call in ("dgrad", "dgrad_add"):
            x = torch.zeros((layer.shape[0], layer.cin) + layer.shape[1:], dtype=dt, requires_grad=True)
            y = X.conv_reference(layer, x, ops["w"].to(dt), None)
            (gx,) = torch.autograd.grad(y, x, ops["dy"].to(dt))
            if "addend" in ops:
                gx = gx + ops["addend"].to(dt)
            assert torch.equal(gx.double(), want64), (layer.name, call)
        if call == "wgrad":
            w = torch.zeros(X.w_shape(layer), dtype=dt, requires_grad=True)
            b = torch.zeros(layer.cout, dtype=dt, requires_grad=True)
            y = X.conv_reference(layer, ops["x"].to(dt), w, b)
            gw, gb = torch.autograd.grad(y, [w, b], ops["dy"].to(dt))
            assert torch.equal((gw + ops["dw0"]).double(), want64[0]) and torch.equal((gb + ops["db0"]).double(), want64[1])


def test_e4m3_operands_are_e4m3_values():
    """x in -8..8 and w / 2^-6 (w from {0, +-1, +-2, +-4, +-7}, max 7: the device-side scale max|w| / 448 is 2^-6) survive the
    round trip through torch's OCP e4m3 type unchanged."""
    for layer in X.FP8:
        o = X.operands(layer, "fwd8")
        assert float(o["w"].abs().max()) == 7.0
        for t in (o["x"], o["w"] * 64.0):
            assert torch.equal(t.to(torch.float8_e4m3fn).float(), t)


# the three corruptions of the issue's table: (layer, densities are those `operands` picks, corruption)
S2 = X.L("s2_48to96", 48, 96, 3, 2, 1, 0, 0, 0, (2, 512, 256))
TRUNK = X.L("trunk_768_n32", 768, 768, 3, 1, 1, 1, 0, 0, (32, 32, 16))


def _corrupt(kind, layer, o):
    y = o["want"].clone()
    if kind == "centre_tap_at_corners":          # the centre tap dropped at the four corner pixels of every plane
        N, H, W = layer.shape
        for (ho, wo) in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
            hi, wi = (0 if ho == 0 else (y.shape[2] - 1) * 2), (0 if wo == 0 else (y.shape[3] - 1) * 2)
            y[:, :, ho, wo] -= torch.einsum("nc,kc->nk", o["x"][:, :, hi, wi], o["w"][:, :, 1, 1])
    elif kind == "last_pixel_from_previous_sample":
        y[-1, :, -1, -1] = y[-2, :, -1, -1]
    else:                                         # 64 of 768 channels of one corner pixel (of one sample) zero
        y[5, 64:128, 0, -1] = 0
    return y


@pytest.mark.parametrize("kind,layer", [("centre_tap_at_corners", S2), ("last_pixel_from_previous_sample", S2),
                                        ("channel_group_of_a_corner_pixel", TRUNK)])
def test_bit_comparison_catches_what_the_relative_l2_bounds_let_through(kind, layer):
    """The gap the exact suite closes: each corruption stays below test_conv_block's bf16 bound on y (1e-2 relative L2) and
    fails assert_bits_equal, whose message names the place."""
    o = X.operands(layer, "fwd")
    bad = _corrupt(kind, layer, o)
    assert not torch.equal(bad, o["want"])
    e = rel_err(bad.numpy(), o["want"].numpy())
    print(f"{kind}: rel L2 {e:.2e}, abs bound {o['bound']}, density {o['density']}")
    assert 0 < e < 1e-2, e
    got = X.to_nhwc(bad, torch.bfloat16)
    with pytest.raises(AssertionError) as info:
        X.assert_bits_equal(got, o["want"], "nhwc", kind)
    msg = str(info.value)
    assert "histograms" in msg and "'h':" in msg and "c%64" in msg
    X.assert_bits_equal(X.to_nhwc(o["want"], torch.bfloat16), o["want"], "nhwc", kind)      # and the uncorrupted tensor passes


def test_assert_bits_equal_sees_pad_channels_and_ignores_the_sign_of_zero():
    want = torch.tensor([[[[1.0, 0.0], [-2.0, 3.0]]]])               # N = 1, C = 1, 2 x 2
    got = X.to_nhwc(want, torch.bfloat16)
    got[0, 0, 1, 0] = -0.0
    X.assert_bits_equal(got, want, "nhwc", "zero sign")
    got[0, 1, 1, 5] = 1.0                                            # a pad channel
    with pytest.raises(AssertionError, match="pad_channels': 1"):
        X.assert_bits_equal(got, want, "nhwc", "pad channel")
    near = X.to_nhwc(want, torch.float16)
    near[0, 0, 0, 0] = 1.0 + 2.0 ** -10                              # one ulp of fp16
    with pytest.raises(AssertionError, match="1 of 32 elements"):
        X.assert_bits_equal(near, want, "nhwc", "one ulp")


@pytest.mark.parametrize("shape", [(2, 4, 4), (1, 5, 7), (2, 6, 4)])
def test_reflection_extras_builder_reproduces_the_reflect_input_gradient(shape):
    """The host builder of the extras block + the pad_mode 3 gather rule = the adjoint of ReflectionPad2d(1) + Conv3x3."""
    layer = X.L("rx", 8, 16, 3, 1, 1, 1, 0, 0, shape)
    o = X.operands(layer, "dgrad")
    dy = X.to_nhwc(o["dy"], torch.float32)
    ex = X.reflect_extras(dy)
    N, H, W = shape
    assert tuple(ex.shape) == (N, 2 * (W + 2) + 2 * H, 16)
    dx = X.reflect_dgrad_from_extras(layer, dy, ex, o["w"])
    assert torch.equal(dx, o["want"].double())


def test_mean_bound_holds_for_fp32_summation_in_another_order():
    """sum_bound is a statement about ANY summation order: a blocked fp32 mean of integer planes stays inside it."""
    gen = torch.Generator().manual_seed(3)
    y = X.int_tensor((2, 5, 32, 16), -200, 200, 0.8, gen)
    mean, m2, bm, b2 = X.stats_reference(y)
    mean32 = (y.reshape(2, 5, 8, 64).sum(-1) / 64).mean(-1)          # per-block means, then their mean: fp32 throughout
    assert bool(((mean32.double() - mean).abs() <= bm).all()) and bool((b2 <= 1e-4 * m2).all())
