"""GPU parity of the fused conv block (HIP implicit-GEMM conv + InstanceNorm/act kernels, through the C ABI)
against the same layer expressed with torch-CPU fp32 functional ops (the oracle's building blocks), for every
conv geometry the generator / discriminator use: forward, input gradient, weight and bias gradients."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err, assert_grad_close

pytestmark = pytest.mark.gpu

ACT = {0: lambda v: v, 1: lambda v: F.leaky_relu(v, 0.2), 2: torch.tanh, 3: F.relu}

# name, cin, cout, k, stride, pad, pad_mode, transposed, opad, norm, act, (N,H,W), residual
CASES = [
    ("c7_reflect_in_relu", 2, 8, 7, 1, 3, 1, False, 0, True, 3, (2, 20, 12), False),      # G first layer
    ("c7_reflect_tanh", 8, 2, 7, 1, 3, 1, False, 0, False, 2, (2, 12, 20), False),        # G head
    ("c3_s2_in_relu", 8, 16, 3, 2, 1, 0, False, 0, True, 3, (2, 16, 10), False),          # downsample
    ("c3_s2_odd", 16, 24, 3, 2, 1, 0, False, 0, True, 3, (1, 15, 9), False),
    ("c3_reflect_in_relu", 16, 16, 3, 1, 1, 1, False, 0, True, 3, (2, 6, 5), False),      # resblock conv 1
    ("c3_reflect_in_res", 16, 16, 3, 1, 1, 1, False, 0, True, 0, (2, 6, 5), True),        # resblock conv 2 + skip
    ("c3_reflect_2x2", 32, 32, 3, 1, 1, 1, False, 0, True, 3, (2, 2, 2), False),          # smallest trunk
    ("ct3_s2_in_relu", 16, 8, 3, 2, 1, 0, True, 1, True, 3, (2, 5, 7), False),            # upsample
    ("c4_s2_lrelu", 4, 8, 4, 2, 2, 0, False, 0, False, 1, (2, 16, 10), False),            # D layer 0
    ("c4_s2_in_lrelu", 8, 16, 4, 2, 2, 0, False, 0, True, 1, (2, 9, 7), False),           # D layer 1-2
    ("c4_s1_in_lrelu", 16, 32, 4, 1, 2, 0, False, 0, True, 1, (2, 5, 4), False),          # D layer 3
    ("c4_s1_to1", 32, 1, 4, 1, 2, 0, False, 0, False, 0, (2, 6, 5), False),               # D head
    ("wide_k200_c136", 136, 200, 3, 1, 1, 1, False, 0, True, 3, (1, 12, 12), False),      # >1 N tile, K not /64
    ("big_m_tiles", 8, 8, 3, 1, 1, 0, False, 0, True, 3, (2, 40, 33), False),             # several M tiles + tail
    ("wgrad_rows256", 72, 256, 3, 1, 1, 1, False, 0, True, 3, (2, 10, 9), False),         # 256-row weight-gradient tile
    ("ct_wgrad_rows256", 256, 40, 3, 2, 1, 0, True, 1, True, 3, (1, 6, 7), False),        # same, ConvTranspose (rows = x)
    ("kfold_norm_k3", 8, 3, 7, 1, 3, 1, False, 0, True, 3, (2, 14, 19), False),           # output fold + IN statistics
    ("kfold_c4_k4_zero", 4, 4, 3, 1, 1, 0, False, 0, False, 1, (2, 9, 11), False),        # both tiny: output fold, zero pad
    ("cfold_c3_zero", 3, 24, 5, 1, 2, 0, False, 0, True, 3, (1, 11, 13), False),          # input fold, zero pad
    # planes of > 16384 pixels: InstanceNorm sums go through the per-tile table + reduce instead of per-sample atomics
    ("bigplane_stats", 8, 16, 3, 1, 1, 0, False, 0, True, 3, (2, 160, 112), False),
    ("bigplane_cfold", 2, 8, 7, 1, 3, 1, False, 0, True, 3, (1, 136, 128), False),
    ("bigplane_ct", 16, 8, 3, 2, 1, 0, True, 1, True, 3, (1, 72, 120), False),
    # whole 8 x 128 tiles: bf16 takes the dedicated 2-channel 7x7 kernel (csrc/c7.hip), fp32 the generic W-fold path
    ("c7fast_2to48", 2, 48, 7, 1, 3, 1, False, 0, True, 3, (2, 16, 128), False),
    ("c7fast_2to96", 2, 96, 7, 1, 3, 1, False, 0, True, 3, (1, 8, 256), False),
    ("c7fast_2to64", 2, 64, 7, 1, 3, 1, False, 0, True, 3, (1, 8, 128), False),
    ("c7fast_2to32_noin", 2, 32, 7, 1, 3, 1, False, 0, False, 0, (1, 8, 128), False),
    # the generator head on whole tiles: bf16 input gradient = the same kernel with flipped weights + reflection fold of the frame
    ("c7fast_48to2_tanh", 48, 2, 7, 1, 3, 1, False, 0, False, 2, (2, 16, 128), False),
    ("c7fast_96to2_tanh", 96, 2, 7, 1, 3, 1, False, 0, False, 2, (1, 8, 256), False),
    ("c7fast_32to2_tanh", 32, 2, 7, 1, 3, 1, False, 0, False, 2, (1, 24, 128), False),
    # round 4: the generator's outermost stride-2 layers at ngf 48 on whole 64-pixel strips: bf16 takes the marching kernels
    # (csrc/march.hip) -- forward of the Conv2d, input gradient of the ConvTranspose2d --, fp32 the generic gather-GEMM
    ("march_s_48to96", 48, 96, 3, 2, 1, 0, False, 0, True, 3, (2, 16, 128), False),      # 1 strip x 2 segments of 4 rows
    ("march_s_48to96_2strips", 48, 96, 3, 2, 1, 0, False, 0, True, 3, (1, 24, 256), False),   # 2 strips x 3 segments
    ("march_ct_96to48", 96, 48, 3, 2, 1, 0, True, 1, True, 3, (2, 8, 64), False),        # its dgrad is the 48 -> 96 gather
    ("march_ct_96to48_2strips", 96, 48, 3, 2, 1, 0, True, 1, True, 3, (1, 12, 128), False),
    # round 4: merged sub-pixel launches of the 3x3 stride-2 layers that stop behind the taps of the tile's class (GDesc::cls_skip;
    # 16-bit types, >= 192 tiles of 256 x 192): ConvTranspose2d forward with class pitch 96 (two classes per tile) and 192 (one),
    # and the input gradient of the Conv2d
    ("skip_ct_192to96", 192, 96, 3, 2, 1, 0, True, 1, True, 3, (8, 64, 64), False),
    ("skip_ct_384to192", 384, 192, 3, 2, 1, 0, True, 1, True, 3, (4, 64, 64), False),
    ("skip_s2_96to192", 96, 192, 3, 2, 1, 0, False, 0, True, 3, (8, 128, 128), False),
    # round 4: the HALO main loop of the 256 x 192 tile (csrc/gconv_halo.inc; 16-bit types, 16-wide planes, >= 160 tiles):
    # forward behind ReflectionPad2d(1) (768 output channels: the tile's GEMM N), and the input gradient through the reflection
    # adjoint's extras (768 INPUT channels), two 64-channel chunks of K each; the 48-row plane has a tile with neither border
    ("halo_fwd_128to768", 128, 768, 3, 1, 1, 1, False, 0, True, 3, (28, 32, 16), False),
    ("halo_dgrad_768to128", 768, 128, 3, 1, 1, 1, False, 0, True, 3, (28, 32, 16), False),
    ("halo_both_768_rows48", 768, 768, 3, 1, 1, 1, False, 0, True, 3, (19, 48, 16), False),
    # round 5: the discriminator's first layer (4 -> 64, 4 x 4 stride 2, LeakyReLU, no statistics): 16-bit types take csrc/dfirst.hip
    # (pixels straight into MFMA fragments), fp32 the generic gather-GEMM; odd planes, a last block of fewer than 16 pixels
    ("dfirst_4to64", 4, 64, 4, 2, 2, 0, False, 0, False, 1, (3, 37, 50), False),
    ("dfirst_4to64_tiny", 4, 64, 4, 2, 2, 0, False, 0, False, 1, (1, 5, 3), False),
    ("dfirst_2to64_noact", 2, 64, 4, 2, 2, 0, False, 0, False, 0, (2, 16, 24), False),
    # round 5: the discriminator's head (C -> 1, 4 x 4 stride 1, no norm, no activation): 16-bit types take csrc/dlast.hip for the
    # forward and the input gradient (16 taps as an MFMA dimension), fp32 the W-fold path
    ("dlast_512to1", 512, 1, 4, 1, 2, 0, False, 0, False, 0, (3, 21, 13), False),
    ("dlast_128to1_tiny", 128, 1, 4, 1, 2, 0, False, 0, False, 0, (2, 3, 5), False),
    ("dlast_384to1", 384, 1, 4, 1, 2, 0, False, 0, False, 0, (1, 40, 36), False),
    # round 5: the 128 x 192 tile of planes too small for 256-row tiles (the 1536-channel trunk of the two-scale generator at
    # 16 x 8, 16-bit types, >= 192 tiles): forward with InstanceNorm partial sums, and the input gradient through the reflection
    # adjoint's extras
    ("tile128x192_fwd_64to1152", 64, 1152, 3, 1, 1, 1, False, 0, True, 3, (32, 16, 8), False),
    ("tile128x192_dgrad_1152to64", 1152, 64, 3, 1, 1, 1, False, 0, True, 3, (32, 16, 8), False),
]


SLOPE = {1: 0.2, 3: 0.0}


def _oracle(x, w, b, res, c, mask=None, pre_only=False):
    """The layer with torch-CPU fp32 functional ops.  `mask` (bool, output shape): take the (Leaky)ReLU branch decision
    from the candidate's own output instead of from this computation's sign -- the two differ only where the
    pre-activation is within rounding of zero, and there a different branch is not an error of the candidate (the test
    checks exactly that: every flipped element's pre-activation, `pre_only`, must be within rounding of zero)."""
    name, cin, cout, k, stride, pad, pad_mode, transposed, opad, norm, act, _, _ = c
    if transposed:
        y = F.conv_transpose2d(x, w, b, stride=stride, padding=pad, output_padding=opad)
    elif pad_mode:
        y = F.conv2d(F.pad(x, (pad,) * 4, mode="reflect"), w, b, stride=stride)
    else:
        y = F.conv2d(x, w, b, stride=stride, padding=pad)
    if norm:
        y = F.instance_norm(y, eps=1e-5)
    if pre_only:
        return y
    if mask is not None and act in SLOPE:
        y = y * torch.where(mask, torch.ones(()), torch.full((), SLOPE[act]))
    else:
        y = ACT[act](y)
    if res is not None:
        y = y + res
    return y


def conv_case_errors(case, dtype, seed):
    """Run one layer on the HIP path and against the oracle; returns {quantity: relative L2 error}.
    fp32: oracle on the same fp32 operands.  bf16: the oracle gets what the kernels actually consume -- x, w and the
    residual rounded to bf16 (bias and accumulation stay fp32) -- and the activation branch of every element from the
    HIP output, so what remains is accumulation order, the bf16 rounding of the stored intermediates (y, dy) and of the
    output, NOT the quantisation of the inputs or a (Leaky)ReLU branch that flipped at |pre-activation| ~ 1e-3."""
    from pix2pixhdaudiosr_amd import _ops
    name, cin, cout, k, stride, pad, pad_mode, transposed, opad, norm, act, (N, H, W), use_res = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=g)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = torch.randn(wshape, generator=g) * 0.1
    b = torch.randn(cout, generator=g) * 0.1
    yo_shape = _oracle(x, w, b, None, case).shape
    res = torch.randn(yo_shape, generator=g) if use_res else None
    cot = torch.randn(yo_shape, generator=g)

    spec = _ops.ConvSpec(cin, cout, k, stride, pad, pad_mode, transposed, opad, norm, act)
    xd = x.cuda().requires_grad_(True)
    wd = w.cuda().requires_grad_(True)
    bd = b.cuda().requires_grad_(True)
    xp = _ops.ToPhysical.apply(dtype, xd)
    rp = None
    if use_res:
        rd = res.cuda().requires_grad_(True)
        rp = _ops.ToPhysical.apply(dtype, rd)
    yp = _ops.conv_block(xp, wd, bd, spec, rp)
    assert yp.shape[-1] == _ops.cpitch(cout)
    if yp.shape[-1] > cout:
        assert float(yp.detach()[..., cout:].float().abs().max()) == 0.0      # pad channels stay zero
    y = _ops.FromPhysical.apply(yp, cout)
    assert tuple(y.shape) == tuple(yo_shape)
    grd = torch.autograd.grad((y * cot.cuda()).sum(), [xd, wd, bd] + ([rd] if use_res else []))

    q = (lambda t: t.to(dtype).float()) if dtype in (torch.bfloat16, torch.float16) else (lambda t: t)
    xo, wo, bo = (t.clone().requires_grad_(True) for t in (q(x), q(w), b))
    res_o = q(res).clone().requires_grad_(True) if use_res else None
    mask = (y.detach().cpu() > 0) if act in SLOPE else None
    yo = _oracle(xo, wo, bo, res_o, case, mask)
    gro = torch.autograd.grad((yo * cot).sum(), [xo, wo, bo] + ([res_o] if use_res else []))
    err = {"y": rel_err(y.detach().cpu().numpy(), yo.detach().numpy()),
           "dx": rel_err(grd[0].cpu().numpy(), gro[0].numpy()),
           "dw": rel_err(grd[1].cpu().numpy(), gro[1].numpy()),
           "db_abs": float(np.linalg.norm(grd[2].cpu().numpy() - gro[2].numpy())),
           "db_ref": float(np.linalg.norm(gro[2].numpy())), "out_elems": int(yo.numel())}
    if use_res:
        err["dres"] = rel_err(grd[3].cpu().numpy(), gro[3].numpy())
    if mask is not None:
        # branch decisions that differ from the oracle's own: how many, and how far from the kink the worst one is (relative
        # to the RMS of the pre-activation) -- a kernel that wrongly zeroes (or keeps) an output shows up here, since the
        # comparison above follows the candidate's branches
        assert res_o is None, "activation + residual in one block: the candidate's output sign is not its branch"
        pre = _oracle(xo.detach(), wo.detach(), bo.detach(), None, case, pre_only=True)
        flipped = (pre > 0).ne(mask)
        err["flips"] = int(flipped.sum())
        rms = float(pre.pow(2).mean().sqrt())
        err["flip_pre_max"] = float(pre[flipped].abs().max() / rms) if err["flips"] else 0.0
    return err


# Tolerances (relative L2 unless noted).  fp32: north_star's 1e-4 on activations, 3e-4 on gradients.  bf16 (the
# throughput mode): the oracle consumes the same bf16-rounded operands and the candidate's own activation branches
# (conv_case_errors), so the bound covers only the bf16 rounding of stored intermediates and accumulation order --
# measured over 20 seeds per case with tools/probe_conv_errors.py (profiles/r02_conv_error_table.txt: worst y 3.5e-3,
# gradients 3.5e-3, 8e-3 on the 2x2 plane), bound = 3x the worst seen.
# Bias gradients are column sums of dy over all pixels: their rounding noise grows like sqrt(pixels x channels), so the
# absolute floor does too (coefficient = 3x the worst seen); a bias in front of InstanceNorm has a true gradient of
# exactly 0 and holds ONLY that noise, on both sides.
# Activation branches: the comparison follows the CANDIDATE'S (Leaky)ReLU branches, so the branches themselves are checked
# separately: an element may sit on the other side of the kink than the oracle's only if its oracle pre-activation is
# within the rounding of the path of zero -- fp32: 1e-5 of the RMS pre-activation (accumulation order; at most a handful
# of elements), bf16: 3e-2 (the raw conv output is stored in bf16 before the normalisation: 2^-8 relative on values up to
# several RMS) and at most 2 % of the elements.
# fp16 storage (round 4: the fp16 build of the library, 11 significand bits): an eighth of the bf16 bounds, measured the same way.
TOL = {torch.float32: dict(y=1e-4, g=3e-4, g_tiny=3e-4, db=1e-6, db_norm=1e-4, flip_pre=1e-5, flip_share=1e-4),
       torch.bfloat16: dict(y=1e-2, g=1.2e-2, g_tiny=2.5e-2, db=8e-3, db_norm=2.5e-2, flip_pre=3e-2, flip_share=2e-2),
       torch.float16: dict(y=1.5e-3, g=2e-3, g_tiny=4e-3, db=1e-3, db_norm=4e-3, flip_pre=4e-3, flip_share=3e-3)}
TINY_PLANES = {"c3_reflect_2x2"}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_block(case, dtype):
    name, norm = case[0], case[9]
    t = TOL[dtype]
    e = conv_case_errors(case, dtype, zlib.crc32(name.encode()) % 1000)   # stable across processes (hash() is salted)
    gt = t["g_tiny"] if name in TINY_PLANES else t["g"]
    assert e["y"] < t["y"], (name, e)
    assert e["dx"] < gt, (name, e)
    assert e["dw"] < gt, (name, e)
    if "dres" in e:
        assert e["dres"] < gt, (name, e)
    if "flips" in e:
        assert e["flip_pre_max"] <= t["flip_pre"], (name, e)
        assert e["flips"] <= max(2, int(t["flip_share"] * e["out_elems"])), (name, e)
    noise = np.sqrt(e["out_elems"])                                # sqrt(pixels x channels)
    if norm:
        assert e["db_abs"] <= t["db_norm"] * noise, (name, e)
    else:
        assert e["db_abs"] <= gt * e["db_ref"] + t["db"] * noise, (name, e)


def test_dedicated_c7_kernel_equals_generic_path():
    """The 2-channel 7x7 layer on whole 8 x 128 tiles: dedicated kernel (csrc/c7.hip) vs the generic W-fold gather conv
    it replaces, same bf16 inputs: outputs equal to bf16 rounding of the store, statistics-dependent normalised output too."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 2, 24, 256, generator=g)
    x[:, 1] += 7.0                                                  # a channel with |mean| >> sigma (the dB spectrogram case)
    w = torch.randn(48, 2, 7, 7, generator=g) * 0.1
    b = torch.randn(48, generator=g)
    res = []
    for generic in (0, 1):
        _lib.check(L.p2phd_set_option(b"c7_generic", generic))
        try:
            spec = _ops.ConvSpec(2, 48, 7, 1, 3, 1, False, 0, True, _ops.ACT_RELU)
            with torch.no_grad():
                yp = _ops.conv_block(_ops.ToPhysical.apply(torch.bfloat16, x.cuda()), w.cuda(), b.cuda(), spec)
            res.append(yp.float().cpu())
        finally:
            _lib.check(L.p2phd_set_option(b"c7_generic", 0))
    assert rel_err(res[0].numpy(), res[1].numpy()) < 6e-3            # two bf16 roundings of values that agree to fp32 accumulation order
    assert float((res[0] - res[1]).abs().max()) < 0.1


@pytest.mark.parametrize("bm", [128, 256, 192, 512])
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)])
def test_tile_heights_agree_with_oracle(bm, dtype, tol):
    """Both M-tile heights of the gather conv (128 rows / 2-slot ring, 256 rows / 3-slot ring with counted vmcnt) on
    layers big enough to run many K steps, several N tiles and ragged M tails."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    cases = [(96, 136, 3, 1, 1, 1, (2, 24, 20)),      # reflect 3x3, K not a multiple of 64, 2 N tiles
             (64, 264, 3, 1, 1, 1, (2, 20, 18)),      # > 256 output channels: two 256-wide N tiles with a ragged tail
             (72, 384, 3, 1, 1, 1, (2, 18, 16)),      # 384 = 2 x 192: the 256x192 tile
             (64, 64, 4, 2, 2, 0, (2, 34, 30)),       # D-style 4x4 s2, BN 64
             (72, 128, 3, 2, 1, 0, (1, 47, 33))]      # odd sizes
    _lib.check(_lib.lib().p2phd_set_option(b"gconv_bm", bm))
    try:
        for (cin, cout, k, stride, pad, pad_mode, (N, H, W)) in cases:
            g = torch.Generator().manual_seed(cin + cout)
            x = torch.randn(N, cin, H, W, generator=g)
            w = torch.randn(cout, cin, k, k, generator=g) * 0.05
            b = torch.randn(cout, generator=g) * 0.1
            case = ("t", cin, cout, k, stride, pad, pad_mode, False, 0, True, 3, (N, H, W), False)
            xo = x.clone().requires_grad_(True)
            yo = _oracle(xo, w, b, None, case)
            cot = torch.randn(yo.shape, generator=g)
            (gxo,) = torch.autograd.grad((yo * cot).sum(), xo)
            spec = _ops.ConvSpec(cin, cout, k, stride, pad, pad_mode, False, 0, True, 3)
            xd = x.cuda().requires_grad_(True)
            y = _ops.FromPhysical.apply(_ops.conv_block(_ops.ToPhysical.apply(dtype, xd), w.cuda(), b.cuda(), spec), cout)
            assert rel_err(y.detach().cpu().numpy(), yo.detach().numpy()) < tol
            (gx,) = torch.autograd.grad((y * cot.cuda()).sum(), xd)
            assert rel_err(gx.cpu().numpy(), gxo.numpy()) < (1e-3 if dtype == torch.float32 else 0.2)   # through IN backward
    finally:
        _lib.check(_lib.lib().p2phd_set_option(b"gconv_bm", 0))


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.bfloat16, 1e-2)])
def test_avgpool(dtype, tol):
    from pix2pixhdaudiosr_amd import _ops
    for (N, C, H, W) in [(2, 4, 16, 10), (1, 2, 7, 5), (2, 16, 2, 2)]:
        x = torch.randn(N, C, H, W)
        xo = x.clone().requires_grad_(True)
        yo = F.avg_pool2d(xo, 3, stride=2, padding=[1, 1], count_include_pad=False)
        cot = torch.randn_like(yo)
        (gxo,) = torch.autograd.grad((yo * cot).sum(), xo)
        xd = x.cuda().requires_grad_(True)
        y = _ops.FromPhysical.apply(_ops.avgpool(_ops.ToPhysical.apply(dtype, xd), C), C)
        assert tuple(y.shape) == tuple(yo.shape)
        assert rel_err(y.detach().cpu().numpy(), yo.detach().numpy()) < tol
        (gx,) = torch.autograd.grad((y * cot.cuda()).sum(), xd)
        assert rel_err(gx.cpu().numpy(), gxo.numpy()) < tol * 2


def test_losses_and_adam():
    from pix2pixhdaudiosr_amd import _ops, _lib
    torch.manual_seed(0)
    a = torch.randn(2, 3, 5, 4)
    b = torch.randn(2, 3, 5, 4)
    for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 2e-2)):
        ad = a.cuda().requires_grad_(True)
        ap = _ops.ToPhysical.apply(dtype, ad)
        bp = _ops.ToPhysical.apply(dtype, b.cuda())
        l_mse = _ops.mse_const_loss(ap, 3, 1.0)
        l_l1 = _ops.l1_loss(ap, bp, 3, 2.5)
        ao = a.clone().requires_grad_(True)
        ro_mse = F.mse_loss(ao, torch.ones_like(ao))
        ro_l1 = 2.5 * F.l1_loss(ao, b)
        assert abs(float(l_mse) - float(ro_mse)) < tol * 5 and abs(float(l_l1) - float(ro_l1)) < tol * 5
        (gd,) = torch.autograd.grad(l_mse * 3.0 + l_l1, ad)
        (go,) = torch.autograd.grad(ro_mse * 3.0 + ro_l1, ao)
        assert rel_err(gd.cpu().numpy(), go.numpy()) < max(tol * 10, 1e-4)
    # Adam vs torch.optim.Adam over 3 steps
    n = 1003
    p0 = torch.randn(n)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=2e-4, betas=(0.5, 0.999))
    p = p0.clone().cuda()
    # 16-byte aligned flat buffers
    m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    for step in range(1, 4):
        gr = torch.randn(n)
        ref.grad = gr.clone()
        opt.step()
        _lib.check(_lib.lib().p2phd_adam_step(_lib.ptr(p), _lib.ptr(gr.cuda()), _lib.ptr(m), _lib.ptr(v), n, 2e-4, 0.5, 0.999, 1e-8,
                                              step, 1.0, _lib.stream_ptr()))
    assert float((p.cpu() - ref.detach()).abs().max()) < 1e-6


def test_device_state_adam_and_accumulating_entry_points():
    """The graph-capturable / in-place variants of the C ABI against their plain counterparts:
    p2phd_adam_step_dev (learning rate + step counter in device memory) == torch.optim.Adam over steps with an LR change;
    p2phd_conv_wgrad_acc, p2phd_instnorm_act_bwd_acc and p2phd_act_bwd_db add into (or fill) caller buffers."""
    import ctypes as C
    from pix2pixhdaudiosr_amd import _ops, _lib
    L = _lib.lib()
    torch.manual_seed(5)
    # --- Adam with device-side state
    n = 1003
    p0 = torch.randn(n)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=2e-4, betas=(0.5, 0.999))
    p = p0.clone().cuda()
    m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    lr_dev = torch.tensor([2e-4], device="cuda"); step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    for step in range(1, 6):
        if step == 4:
            opt.param_groups[0]["lr"] = 1e-4
            lr_dev.fill_(1e-4)
        gr = torch.randn(n)
        ref.grad = gr.clone()
        opt.step()
        _lib.check(L.p2phd_adam_step_dev(_lib.ptr(p), _lib.ptr(gr.cuda()), _lib.ptr(m), _lib.ptr(v), n, _lib.ptr(lr_dev),
                                         _lib.ptr(step_dev), 0.5, 0.999, 1e-8, 1.0, _lib.stream_ptr()))
    assert int(step_dev.item()) == 5
    assert float((p.cpu() - ref.detach()).abs().max()) < 1e-6
    # --- wgrad_acc: twice into a zeroed buffer == 2 x the overwriting entry point; bias gradient likewise
    spec = _ops.ConvSpec(24, 40, 3, 1, 1, 0, False, 0, False, _ops.ACT_NONE)
    N, H, W = 2, 12, 10
    x = torch.randn(N, H, W, _ops.cpitch(24), device="cuda"); x[..., 24:] = 0
    d = spec.desc(N, H, W, torch.float32)
    Ho, Wo = spec.out_size(d)
    dy = torch.randn(N, Ho, Wo, _ops.cpitch(40), device="cuda"); dy[..., 40:] = 0
    ws = torch.empty(max(L.p2phd_conv_wgrad_workspace_bytes(C.byref(d)), 16), dtype=torch.uint8, device="cuda")
    dw = torch.empty(40, 24, 3, 3, device="cuda"); db = torch.empty(40, device="cuda")
    _lib.check(L.p2phd_conv_wgrad(C.byref(d), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), _lib.stream_ptr()))
    acc_w = torch.zeros_like(dw); acc_b = torch.zeros_like(db)
    for _ in range(2):
        _lib.check(L.p2phd_conv_wgrad_acc(C.byref(d), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(acc_w), _lib.ptr(acc_b), _lib.ptr(ws),
                                          _lib.stream_ptr()))
    assert rel_err(acc_w.cpu().numpy(), 2 * dw.cpu().numpy()) < 1e-6 and rel_err(acc_b.cpu().numpy(), 2 * db.cpu().numpy()) < 1e-5
    centre = torch.einsum("nhwk,nhwc->kc", dy[..., :40].cpu().double(), x[..., :24].cpu().double())      # tap (1,1): output pixel == input pixel
    assert rel_err(dw[:, :, 1, 1].cpu().numpy(), centre.numpy()) < 1e-4
    # --- act_bwd_db: dx and the column sums in one pass, fill and accumulate modes
    a = torch.randn(N, Ho, Wo, _ops.cpitch(40), device="cuda"); g = torch.randn_like(a)
    dx = torch.empty_like(a); dbb = torch.full((40,), 7.0, device="cuda")
    _lib.check(L.p2phd_act_bwd_db(_lib.F32, _lib.ptr(g), _lib.ptr(a), _lib.ptr(dx), N * Ho * Wo, 40, _ops.ACT_LRELU, _lib.ptr(dbb), 0,
                                  _lib.stream_ptr()))
    want = g * torch.where(a > 0, torch.ones_like(a), torch.full_like(a, 0.2))
    assert rel_err(dx.cpu().numpy(), want.cpu().numpy()) < 1e-6
    assert rel_err(dbb.cpu().numpy(), want[..., :40].sum((0, 1, 2)).cpu().numpy()) < 1e-5
    _lib.check(L.p2phd_act_bwd_db(_lib.F32, _lib.ptr(g), _lib.ptr(a), _lib.ptr(dx), N * Ho * Wo, 40, _ops.ACT_LRELU, _lib.ptr(dbb), 1,
                                  _lib.stream_ptr()))
    assert rel_err(dbb.cpu().numpy(), 2 * want[..., :40].sum((0, 1, 2)).cpu().numpy()) < 1e-5
    # --- instnorm_act_bwd_acc: same dy as the overwriting entry point, db added on top of what was there
    y = torch.randn(N, Ho, Wo, _ops.cpitch(40), device="cuda"); y[..., 40:] = 0
    mean = y.mean((1, 2))
    stats = torch.stack([mean, ((y - mean[:, None, None]) ** 2).sum((1, 2))], dim=-1).contiguous()   # (mean, M2) per (n, c)
    bst = torch.empty(N, _ops.cpitch(40), 2, device="cuda")
    dy1 = torch.empty_like(y); dy2 = torch.empty_like(y)
    db1 = torch.empty(40, device="cuda"); db2 = torch.full((40,), 3.0, device="cuda")
    _lib.check(L.p2phd_instnorm_act_bwd(_lib.F32, _lib.ptr(g), _lib.ptr(y), _lib.ptr(stats), _lib.ptr(bst), _lib.ptr(dy1), _lib.ptr(db1), N,
                                        Ho * Wo, 40, 1e-5, _ops.ACT_RELU, _lib.stream_ptr()))
    _lib.check(L.p2phd_instnorm_act_bwd_acc(_lib.F32, _lib.ptr(g), _lib.ptr(y), _lib.ptr(stats), _lib.ptr(bst), _lib.ptr(dy2), _lib.ptr(db2), N,
                                            Ho * Wo, 40, 1e-5, _ops.ACT_RELU, _lib.stream_ptr()))
    assert rel_err(dy2.cpu().numpy(), dy1.cpu().numpy()) < 1e-5      # (the per-(n,c) sums are fixed-order; tests/test_gpu_companions.py compares their bits)
    assert float((db2 - 3.0 - db1).abs().max()) < 1e-3


def test_trunk_layer_at_baseline_size():
    """The dominant layer at its BASELINE geometry (Conv3x3 768->768 behind ReflectionPad2d(1) on 32x16 planes + InstanceNorm
    + ReLU): fp32 path against torch-CPU on a 4-sample batch (forward, input / weight gradients), then the full 32-sample
    bf16 launch (256x192 tiles, 256 workgroups) against the fp32 result of the same samples."""
    from pix2pixhdaudiosr_amd import _ops
    g = torch.Generator().manual_seed(11)
    cin = cout = 768
    case = ("trunk", cin, cout, 3, 1, 1, 1, False, 0, True, 3, (4, 32, 16), False)
    x = torch.randn(4, cin, 32, 16, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.02
    b = torch.randn(cout, generator=g) * 0.1
    xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    yo = _oracle(xo, wo, b, None, case)
    cot = torch.randn(yo.shape, generator=g)
    gxo, gwo = torch.autograd.grad((yo * cot).sum(), [xo, wo])
    spec = _ops.ConvSpec(cin, cout, 3, 1, 1, 1, False, 0, True, _ops.ACT_RELU)
    xd, wd, bd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = _ops.FromPhysical.apply(_ops.conv_block(_ops.ToPhysical.apply(torch.float32, xd), wd, bd, spec), cout)
    assert rel_err(y.detach().cpu().numpy(), yo.detach().numpy()) < 1e-4
    gx, gw = torch.autograd.grad((y * cot.cuda()).sum(), [xd, wd])
    # through InstanceNorm + ReLU after a 6912-term fp32 reduction: a handful of ReLU masks flip at |y_hat| ~ 1e-6 and the
    # two fp32 summation orders differ; tolerance 3e-3 relative L2 (element errors ~2e-5 on O(1) values)
    assert rel_err(gx.cpu().numpy(), gxo.numpy()) < 3e-3
    assert rel_err(gw.cpu().numpy(), gwo.numpy()) < 3e-3
    # full batch, bf16 throughput mode: every sample is independent, so samples 0..3 of the 32-sample launch must
    # reproduce the fp32 result up to bf16 rounding
    x32 = torch.cat([x, torch.randn(28, cin, 32, 16, generator=g)]).cuda()
    with torch.no_grad():
        y32 = _ops.FromPhysical.apply(_ops.conv_block(_ops.ToPhysical.apply(torch.bfloat16, x32), wd.detach(), bd.detach(), spec), cout)
    assert tuple(y32.shape) == (32, cout, 32, 16) and torch.isfinite(y32).all()
    assert rel_err(y32[:4].float().cpu().numpy(), yo.detach().numpy()) < 3e-2


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 6e-3)], ids=["f32", "bf16"])
@pytest.mark.parametrize("consumer", ["s2_conv", "s1_conv", "conv_transpose", "s1_256wide", "head_to1", "march_conv_transpose", "march_s2_conv", "dlast_head"])
def test_instnorm_backward_sums_fused_into_the_consumers_dgrad(consumer, dtype, tol, monkeypatch):
    """p2phd_conv_dgrad_bsum: the input-gradient kernel of the consumer leaves the (sum g', sum g' yhat) of the producer's
    InstanceNorm backward, which then runs its apply pass only.  Same gradients as the two-pass form (P2PHD_BSUM=0) up to
    the summation order of the statistics, for the plain launch, the merged sub-pixel launch (stride-2 conv) and the
    stride-2 gather (transposed conv), and against the fp32 oracle."""
    from pix2pixhdaudiosr_amd import _ops
    N, C0, C1, H, W = 2, 16, 24, 48, 40                            # producer plane 48 x 40 = 1920 px: the two-pass form
    if consumer == "s1_256wide":
        C1 = 256
    if consumer == "march_conv_transpose":                         # bf16: the input gradient is the marching kernel (csrc/march.hip)
        C1, H, W = 96, 16, 64
    if consumer == "march_s2_conv":                                # bf16: ... and here its transposed form
        C1, H, W = 48, 16, 128
    if consumer == "dlast_head":                                   # round 5, bf16: the discriminator's 4 x 4 head on csrc/dlast.hip (fp32: W-fold path); odd plane
        C1, H, W = 256, 33, 17
    c2 = {"march_conv_transpose": (C1, 48, 3, 2, 1, 0, True, 1), "march_s2_conv": (C1, 96, 3, 2, 1, 0, False, 0), "s2_conv": (C1, 32, 3, 2, 1, 0, False, 0), "s1_conv": (C1, 40, 3, 1, 1, 0, False, 0),
          "conv_transpose": (C1, 16, 3, 2, 1, 0, True, 1), "s1_256wide": (C1, 256, 3, 1, 1, 0, False, 0),
          "head_to1": (C1, 1, 3, 1, 1, 0, False, 0), "dlast_head": (C1, 1, 4, 1, 2, 0, False, 0)}[consumer]      # 1-channel head: output W-fold in front of the launch
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, C0, H, W, generator=g)
    w1 = torch.randn(C1, C0, 3, 3, generator=g) * 0.1
    w2 = torch.randn((c2[0], c2[1], c2[2], c2[2]) if c2[6] else (c2[1], c2[0], c2[2], c2[2]), generator=g) * 0.05
    specP = _ops.ConvSpec(C0, C1, 3, 1, 1, 0, False, 0, True, _ops.ACT_RELU)
    head = consumer in ("head_to1", "dlast_head")
    specL = _ops.ConvSpec(*c2, not head, _ops.ACT_RELU if not head else _ops.ACT_NONE)

    def run(flag):
        monkeypatch.setenv("P2PHD_BSUM", flag)
        xd = x.cuda().requires_grad_(True)
        w1d, w2d = w1.cuda().requires_grad_(True), w2.cuda().requires_grad_(True)
        h = _ops.conv_block(_ops.ToPhysical.apply(dtype, xd), w1d, None, specP)
        o = _ops.conv_block(h, w2d, None, specL, exclusive=True)   # h goes nowhere else
        out = _ops.FromPhysical.apply(o, c2[1])
        cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).cuda()
        n0 = _ops._BSUM_CALLS[0]
        out.backward(cot)
        torch.cuda.synchronize()
        return out.detach().float().cpu(), xd.grad.cpu(), w1d.grad.cpu(), w2d.grad.cpu(), _ops._BSUM_CALLS[0] - n0

    o1, gx1, gw1, gv1, used = run("1")
    o0, gx0, gw0, gv0, unused = run("0")
    assert used == 1 and unused == 0
    assert torch.equal(o1, o0)
    assert rel_err(gv1.numpy(), gv0.numpy()) < tol                 # (the consumer's own two-pass backward sums with float atomics)
    assert rel_err(gx1.numpy(), gx0.numpy()) < tol and rel_err(gw1.numpy(), gw0.numpy()) < tol
    if dtype == torch.float32:                                     # and against the oracle
        xr, w1r, w2r = x.clone().requires_grad_(True), w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
        hr = F.relu(F.instance_norm(F.conv2d(xr, w1r, padding=1), eps=1e-5))
        if c2[6]:
            orr = F.conv_transpose2d(hr, w2r, stride=2, padding=1, output_padding=1)
        else:
            orr = F.conv2d(hr, w2r, stride=c2[3], padding=c2[4])
        if not head:
            orr = F.relu(F.instance_norm(orr, eps=1e-5))
        orr.backward(torch.randn(orr.shape, generator=torch.Generator().manual_seed(5)))
        assert rel_err(o1.numpy(), orr.detach().numpy()) < 1e-4
        assert rel_err(gx1.numpy(), xr.grad.numpy()) < 3e-4 and rel_err(gw1.numpy(), w1r.grad.numpy()) < 3e-4


def test_fused_backward_sums_need_the_callers_exclusive_flag():
    """Without exclusive=True the producer's sums are never taken from the consumer, whatever autograd does with the
    gradient: a second consumer made of plain torch ops (a view of the tensor) accumulates into the same buffer."""
    from pix2pixhdaudiosr_amd import _ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 16, 48, 40, generator=g).cuda().requires_grad_(True)
    w1 = (torch.randn(24, 16, 3, 3, generator=g) * 0.1).cuda().requires_grad_(True)
    w2 = (torch.randn(32, 24, 3, 3, generator=g) * 0.05).cuda().requires_grad_(True)
    specP = _ops.ConvSpec(16, 24, 3, 1, 1, 0, False, 0, True, _ops.ACT_RELU)
    specL = _ops.ConvSpec(24, 32, 3, 2, 1, 0, False, 0, True, _ops.ACT_RELU)
    h = _ops.conv_block(_ops.ToPhysical.apply(torch.float32, x), w1, None, specP)
    o = _ops.conv_block(h, w2, None, specL)
    n0 = _ops._BSUM_CALLS[0]
    (o.float().sum() + (h[..., :24].float() ** 2).sum()).backward()
    assert _ops._BSUM_CALLS[0] == n0
    xr, w1r, w2r = (t.detach().cpu().requires_grad_(True) for t in (x, w1, w2))
    hr = F.relu(F.instance_norm(F.conv2d(xr, w1r, padding=1), eps=1e-5))
    orr = F.relu(F.instance_norm(F.conv2d(hr, w2r, stride=2, padding=1), eps=1e-5))
    (orr.sum() + (hr ** 2).sum()).backward()
    assert rel_err(x.grad.cpu().numpy(), xr.grad.numpy()) < 3e-4 and rel_err(w1.grad.cpu().numpy(), w1r.grad.numpy()) < 3e-4


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 6e-3)], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 16, 24, 4, 4), (2, 24, 16, 5, 7), (3, 40, 72, 32, 16), (1, 8, 8, 3, 9)])
def test_reflect3x3_input_gradient_on_the_exact_grid_equals_padded_grid_form(shape, dtype, tol):
    """Input gradient of Conv3x3 behind ReflectionPad2d(1) (the residual trunk): the exact-grid form (dy extended by the
    pair-sum rows / columns the mirrored taps read, pad_mode 2 gather, no fold pass) against the general padded-grid + fold
    form (`reflect_generic`), with a skip-gradient addend, incl. planes where rows 1 and H-2 coincide or neighbour (H = 3, 4)
    -- H = 3 takes the general form by itself -- and against the fp32 oracle."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    import ctypes as C
    L = _lib.lib()
    N, cin, cout, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    dy = torch.randn(N, cout, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    add = torch.randn(N, cin, H, W, generator=g)
    spec = _ops.ConvSpec(cin, cout, 3, 1, 1, 1, False, 0, True, _ops.ACT_RELU)
    d = spec.desc(N, H, W, dtype)
    dyp = _ops.to_physical(dy.cuda(), dtype); addp = _ops.to_physical(add.cuda(), dtype)
    wp = spec.packed(w.cuda(), 1, d)
    ws = torch.empty(max(L.p2phd_conv_dgrad_workspace_bytes(C.byref(d)), 256), dtype=torch.uint8, device="cuda")
    outs = []
    for generic in (0, 1):
        _lib.check(L.p2phd_set_option(b"reflect_generic", generic))
        try:
            gx = torch.empty_like(addp)
            _ops.check(L.p2phd_conv_dgrad(C.byref(d), _ops.ptr(dyp), _ops.ptr(wp), _ops.ptr(addp), _ops.ptr(gx), _ops.ptr(ws), _ops.stream_ptr()))
            outs.append(_ops.from_physical(gx, cin).cpu())
        finally:
            _lib.check(L.p2phd_set_option(b"reflect_generic", 0))
    assert rel_err(outs[0].numpy(), outs[1].numpy()) < tol
    if dtype == torch.float32:
        x = torch.zeros(N, cin, H, W, requires_grad=True)
        F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w).backward(dy)
        assert rel_err(outs[0].numpy(), (x.grad + add).numpy()) < 1e-5


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 6e-3)], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", [(8, 256, 512, 8, 16), (16, 64, 512, 4, 5), (8, 128, 512, 20, 32)], ids=["8x16", "4x5", "20x32"])
def test_reflection_extras_written_by_the_instancenorm_backward(geom, dtype, tol):
    """Round 4: on planes that take the single-launch InstanceNorm backward (the residual trunk: 32 x 16), the kernel that
    writes dy appends the pair-sum rows / columns the reflect-padded 3x3 input gradient reads (p2phd_instnorm_act_bwd_rx,
    p2phd_conv_dgrad_rx: gather pad_mode 3) -- no expansion pass.  Whole block (ReflectionPad + Conv3x3 + InstanceNorm + ReLU)
    forward / backward against the padded-grid + fold form (option reflect_generic, which has no extras form) and, in fp32,
    against the oracle; planes down to 4 x 5 (rows 1 and H-2 neighbours)."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    import ctypes as C
    L = _lib.lib()
    N, cin, cout, H, W = geom
    gen = torch.Generator().manual_seed(H * 100 + W + cin)
    x = torch.randn(N, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) * 0.05
    b = torch.randn(cout, generator=gen) * 0.1
    cot = torch.randn(N, cout, H, W, generator=gen)
    spec = _ops.ConvSpec(cin, cout, 3, 1, 1, 1, False, 0, True, _ops.ACT_RELU)
    d = spec.desc(N, H, W, dtype)
    assert L.p2phd_conv_reflect_extras_elems(C.byref(d)) == N * (2 * (W + 2) + 2 * H) * _ops.cpitch(cout)
    outs = []
    for generic in (0, 1):
        _lib.check(L.p2phd_set_option(b"reflect_generic", generic))
        try:
            assert (L.p2phd_conv_reflect_extras_elems(C.byref(d)) > 0) == (generic == 0)
            xd, wd, bd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
            y = _ops.FromPhysical.apply(_ops.conv_block(_ops.ToPhysical.apply(dtype, xd), wd, bd, spec), cout)
            g = torch.autograd.grad((y * cot.cuda()).sum(), [xd, wd])
            torch.cuda.synchronize()
            outs.append((y.detach().cpu(), g[0].cpu(), g[1].cpu()))
        finally:
            _lib.check(L.p2phd_set_option(b"reflect_generic", 0))
    assert torch.equal(outs[0][0], outs[1][0])
    assert rel_err(outs[0][1].numpy(), outs[1][1].numpy()) < tol               # input gradient: extras form vs padded grid + fold
    assert rel_err(outs[0][2].numpy(), outs[1][2].numpy()) < tol               # weight gradient: reads the plain part of dy
    if dtype == torch.float32:
        xo, wo = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        yo = F.relu(F.instance_norm(F.conv2d(F.pad(xo, (1, 1, 1, 1), mode="reflect"), wo, b), eps=1e-5))
        go = torch.autograd.grad((yo * cot).sum(), [xo, wo])
        assert rel_err(outs[0][0].numpy(), yo.detach().numpy()) < 1e-4
        assert rel_err(outs[0][1].numpy(), go[0].numpy()) < 3e-4 and rel_err(outs[0][2].numpy(), go[1].numpy()) < 3e-4


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("geom", [(32, 32, 768), (56, 16, 768), (10, 96, 768), (16, 32, 768)],
                         ids=["trunk_32x16x768", "16rows", "96rows_forward_only", "batch16_on_256x128_tiles"])
def test_halo_loop_equals_the_generic_loop(geom, dtype):
    """Round 4: the HALO main loop of the 256 x 192 tile (csrc/gconv_halo.inc, option gconv_halo) against the generic loop
    on the same launches -- the residual-trunk layer at its real size, forward (ReflectionPad2d(1) gather) with statistics
    and input gradient through the reflection extras --, on a 16-row plane (one tile holds both borders) and, forward only, on a
    96-row plane (tiles with no image border; planes above 640 pixels take the two-pass InstanceNorm backward, which has no extras);
    at batch 16 the grid takes 256 x 128 tiles (round 5: the HALO loop's second instantiation -- configs[4]'s 2048-channel trunk at B = 8).
    The two loops add the same products in a different order (chunk-tap-channel against tap-channel): outputs agree to
    the rounding of the 16-bit store, the fp32 statistics to accumulation noise."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    import ctypes as C
    L = _ops.lib_for(dtype)
    N, H, CH = geom
    W = 16
    gen = torch.Generator().manual_seed(H + CH)
    spec = _ops.ConvSpec(CH, CH, 3, 1, 1, 1, False, 0, True, _ops.ACT_RELU)
    d = spec.desc(N, H, W, dtype)
    x = torch.randn(N, H, W, CH, generator=gen).cuda().to(dtype)
    w = (torch.randn(CH, CH, 3, 3, generator=gen) * 0.02).cuda()
    g = torch.randn(N, H, W, CH, generator=gen).cuda().to(dtype)
    y = torch.empty_like(x); gx = torch.empty_like(x)
    stats = torch.zeros(N, CH, 2, device="cuda")
    wp0, wp1 = spec.packed(w, 0, d), spec.packed(w, 1, d)
    ws = _ops.workspace(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), 1 << 20), "cuda")
    n_rx = L.p2phd_conv_reflect_extras_elems(C.byref(d))
    assert n_rx == (N * (2 * (W + 2) + 2 * H) * CH if H * W <= 640 else 0)
    if n_rx:
        buf = torch.empty(x.numel() + n_rx, device="cuda", dtype=dtype)
        dy, rx = buf[:x.numel()].view(x.shape), buf[x.numel():]
        st = torch.zeros(N, CH, 2, device="cuda"); st[..., 1] = H * W
        db = torch.zeros(CH, device="cuda")
        _ops.check(L.p2phd_instnorm_act_bwd_rx(d.dtype, _ops.ptr(g), _ops.ptr(x), _ops.ptr(st), _ops.ptr(dy), _ops.ptr(db), 1, N, H, W, CH, 1e-5,
                                               _ops.ACT_RELU, _ops.ptr(rx), _ops.stream_ptr()))
    res = {}
    try:
        for halo in (0, 1):
            _lib.check(L.p2phd_set_option(b"gconv_halo", halo))
            _ops.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(x), _ops.ptr(wp0), None, 0, _ops.ptr(y), _ops.ptr(stats), _ops.ptr(ws), _ops.stream_ptr()))
            if n_rx:
                _ops.check(L.p2phd_conv_dgrad_rx(C.byref(d), _ops.ptr(dy), _ops.ptr(wp1), None, _ops.ptr(gx), _ops.stream_ptr()))
            else:
                gx.copy_(y)
            torch.cuda.synchronize()
            res[halo] = (y.float().cpu().numpy(), stats.cpu().numpy().copy(), gx.float().cpu().numpy())
        # the HALO loop counts its LDS-DMA waits by hand: 200 more launches of each must reproduce the first bit for bit (the
        # stale-fragment race this test once caught showed up in one launch of a few hundred: -DP2PHD_ABL_HALO_RACE brings it back)
        y0, g0, s0 = y.clone(), gx.clone(), stats.clone()
        for _ in range(200):
            _ops.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(x), _ops.ptr(wp0), None, 0, _ops.ptr(y), _ops.ptr(stats), _ops.ptr(ws), _ops.stream_ptr()))
            if n_rx:
                _ops.check(L.p2phd_conv_dgrad_rx(C.byref(d), _ops.ptr(dy), _ops.ptr(wp1), None, _ops.ptr(gx), _ops.stream_ptr()))
            assert torch.equal(y, y0) and torch.equal(stats, s0) and (not n_rx or torch.equal(gx, g0))
    finally:
        _lib.check(L.p2phd_set_option(b"gconv_halo", 1))
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    assert rel_err(res[1][0], res[0][0]) < ulp and rel_err(res[1][2], res[0][2]) < ulp
    assert np.abs(res[1][0] - res[0][0]).max() <= 2 * ulp * np.abs(res[0][0]).max()
    assert np.abs(res[1][2] - res[0][2]).max() <= 2 * ulp * np.abs(res[0][2]).max()
    assert rel_err(res[1][1], res[0][1]) < 1e-5                      # (mean, M2) per sample and channel, fp32
    assert not np.array_equal(res[1][1], res[0][1])                  # ... and not the same bits: the other loop really ran
    assert float(np.linalg.norm(res[0][0])) > 0 and float(np.linalg.norm(res[0][2])) > 0


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 6e-3)], ids=["f32", "bf16"])
def test_activation_backward_fused_into_the_consumers_dgrad(dtype, tol, monkeypatch):
    """Producer without InstanceNorm (Conv + LeakyReLU, the discriminator's first layer): the exclusive consumer's
    input-gradient kernel multiplies dx by act'(x) (p2phd_conv_dgrad_act) and the producer skips its activation-backward
    pass; bias and weight gradients of the producer come out the same, also with a parked loss gradient as addend."""
    from pix2pixhdaudiosr_amd import _ops
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 4, 66, 34, generator=g)
    w1 = torch.randn(16, 4, 4, 4, generator=g) * 0.2; b1 = torch.randn(16, generator=g) * 0.1
    w2 = torch.randn(32, 16, 4, 4, generator=g) * 0.05
    ref_feat = torch.randn(2, 16, 34, 18, generator=g)
    specP = _ops.ConvSpec(4, 16, 4, 2, 2, 0, False, 0, False, _ops.ACT_LRELU)
    specL = _ops.ConvSpec(16, 32, 4, 2, 2, 0, False, 0, True, _ops.ACT_LRELU)

    def run(flag):
        monkeypatch.setenv("P2PHD_BSUM", flag)
        xd = x.cuda().requires_grad_(True)
        w1d, b1d, w2d = (t.cuda().requires_grad_(True) for t in (w1, b1, w2))
        h = _ops.conv_block(_ops.ToPhysical.apply(dtype, xd), w1d, b1d, specP)
        o = _ops.conv_block(h, w2d, None, specL, exclusive=True)
        fm = _ops.l1_loss(h, _ops.to_physical(ref_feat.cuda(), dtype), 16, 3.0, park=True)     # second gradient source of h, parked
        n0 = _ops._BSUM_CALLS[0]
        (_ops.FromPhysical.apply(o, 32).sum() * 0.01 + fm).backward()
        torch.cuda.synchronize()
        return xd.grad.cpu(), w1d.grad.cpu(), b1d.grad.cpu(), w2d.grad.cpu(), _ops._BSUM_CALLS[0] - n0

    a = run("1"); b = run("0")
    assert a[4] == 1 and b[4] == 0
    for u, v in zip(a[:4], b[:4]):
        assert rel_err(u.numpy(), v.numpy()) < tol
    if dtype == torch.float32:
        xr, w1r, b1r, w2r = (t.clone().requires_grad_(True) for t in (x, w1, b1, w2))
        hr = F.leaky_relu(F.conv2d(xr, w1r, b1r, stride=2, padding=2), 0.2)
        orr = F.leaky_relu(F.instance_norm(F.conv2d(hr, w2r, stride=2, padding=2), eps=1e-5), 0.2)
        (orr.sum() * 0.01 + 3.0 * (hr - ref_feat).abs().mean()).backward()
        assert rel_err(a[0].numpy(), xr.grad.numpy()) < 3e-4 and rel_err(a[1].numpy(), w1r.grad.numpy()) < 3e-4
        assert rel_err(a[2].numpy(), b1r.grad.numpy()) < 3e-4


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.bfloat16, 6e-3)], ids=["f32", "bf16"])
def test_parked_gradient_that_arrives_after_the_consumers_dgrad(dtype, tol, monkeypatch):
    """Round-2 advisor finding: the loss node is created BEFORE the consumer conv, so autograd runs the consumer's backward
    first (p2phd_conv_dgrad_act applies act'(h) to the conv path of dL/dh and marks it), then the loss parks its gradient on
    the producer.  The producer must give act' to the parked part ONLY (the earlier code re-applied it to the sum:
    LeakyReLU slope 0.04 instead of 0.2 on the conv path).  Reference: the same graph without parking / fusion."""
    from pix2pixhdaudiosr_amd import _ops
    g = torch.Generator().manual_seed(22)
    x = torch.randn(2, 4, 66, 34, generator=g)
    w1 = torch.randn(16, 4, 4, 4, generator=g) * 0.2; b1 = torch.randn(16, generator=g) * 0.1
    w2 = torch.randn(32, 16, 4, 4, generator=g) * 0.05
    ref_feat = torch.randn(2, 16, 34, 18, generator=g)
    specP = _ops.ConvSpec(4, 16, 4, 2, 2, 0, False, 0, False, _ops.ACT_LRELU)
    specL = _ops.ConvSpec(16, 32, 4, 2, 2, 0, False, 0, True, _ops.ACT_LRELU)

    def run(flag, park):
        monkeypatch.setenv("P2PHD_BSUM", flag)
        xd = x.cuda().requires_grad_(True)
        w1d, b1d, w2d = (t.cuda().requires_grad_(True) for t in (w1, b1, w2))
        h = _ops.conv_block(_ops.ToPhysical.apply(dtype, xd), w1d, b1d, specP)
        fm = _ops.l1_loss(h, _ops.to_physical(ref_feat.cuda(), dtype), 16, 3.0, park=park)     # created FIRST: its backward runs LAST
        o = _ops.conv_block(h, w2d, None, specL, exclusive=park)
        n0 = _ops._BSUM_CALLS[0]
        (_ops.FromPhysical.apply(o, 32).sum() * 0.01 + fm).backward()
        torch.cuda.synchronize()
        return xd.grad.cpu(), w1d.grad.cpu(), b1d.grad.cpu(), w2d.grad.cpu(), _ops._BSUM_CALLS[0] - n0

    a = run("1", True); b = run("0", False)
    assert a[4] == 1, "the fused activation backward did not run: the test no longer covers the late-park order"
    for u, v in zip(a[:4], b[:4]):
        assert rel_err(u.numpy(), v.numpy()) < tol
    if dtype == torch.float32:
        xr, w1r, b1r, w2r = (t.clone().requires_grad_(True) for t in (x, w1, b1, w2))
        hr = F.leaky_relu(F.conv2d(xr, w1r, b1r, stride=2, padding=2), 0.2)
        orr = F.leaky_relu(F.instance_norm(F.conv2d(hr, w2r, stride=2, padding=2), eps=1e-5), 0.2)
        (orr.sum() * 0.01 + 3.0 * (hr - ref_feat).abs().mean()).backward()
        assert rel_err(a[0].numpy(), xr.grad.numpy()) < 3e-4 and rel_err(a[1].numpy(), w1r.grad.numpy()) < 3e-4
        assert rel_err(a[2].numpy(), b1r.grad.numpy()) < 3e-4


def test_second_consumer_of_a_fused_activation_gradient_raises(monkeypatch):
    """When the consumer's kernel applied act' and the gradient that reaches the producer is NOT the tensor it wrote (a
    second, un-parked consumer: autograd summed into a new tensor), the producer raises instead of re-applying act'."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    monkeypatch.setenv("P2PHD_BSUM", "1")
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 4, 66, 34, generator=g).cuda().requires_grad_(True)
    w1 = (torch.randn(16, 4, 4, 4, generator=g) * 0.2).cuda().requires_grad_(True)
    w2 = (torch.randn(32, 16, 4, 4, generator=g) * 0.05).cuda().requires_grad_(True)
    specP = _ops.ConvSpec(4, 16, 4, 2, 2, 0, False, 0, False, _ops.ACT_LRELU)
    specL = _ops.ConvSpec(16, 32, 4, 2, 2, 0, False, 0, True, _ops.ACT_LRELU)
    h = _ops.conv_block(_ops.ToPhysical.apply(torch.float32, x), w1, None, specP)
    side = h.float().square().sum() * 1e-3                        # plain torch consumer created first: its gradient is summed in last
    o = _ops.conv_block(h, w2, None, specL, exclusive=True)       # (a false promise)
    with pytest.raises(_lib.P2PHDError):
        (_ops.FromPhysical.apply(o, 32).sum() * 0.01 + side).backward()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", [(64, 96, 3, 1, 1, 1, (3, 40, 28)),      # 15 M tiles x 1: tail = whole grid, deep split
                                  (256, 512, 4, 1, 2, 0, (9, 34, 18)),    # D 256 -> 512 k4 s1 (one sample = 630 pixels)
                                  (128, 128, 3, 2, 1, 0, (5, 33, 47))],   # stride 2, odd sizes
                         ids=["c3_64to96", "d_256to512", "c3s2_odd"])
def test_split_k_tail_equals_whole_tiles(dtype, geom):
    """Round 3: the tiles of the last, almost empty round of a grid are cut along K into parts that fill the CUs; the part
    that finishes last adds the partials in a fixed order (gconv_kernel / launch_gconv_cfg).  Same values as one workgroup
    per tile up to fp32 summation order, the same bits from run to run, statistics included."""
    import ctypes as C
    from pix2pixhdaudiosr_amd import _ops, _lib
    cin, cout, k, stride, pad, pad_mode, (N, H, W) = geom
    L = _ops.lib()
    g = torch.Generator().manual_seed(5)
    x = _ops.to_physical(torch.randn(N, cin, H, W, generator=g).cuda(), dtype)
    w = (torch.randn(cout, cin, k, k, generator=g) * 0.05).cuda()
    b = (torch.randn(cout, generator=g) * 0.1).cuda()
    spec = _ops.ConvSpec(cin, cout, k, stride, pad, pad_mode, False, 0, True, _ops.ACT_RELU)
    d = spec.desc(N, H, W, dtype)
    Ho, Wo = spec.out_size(d)
    wp = spec.packed(w, 0, d)
    ws = torch.empty(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), 256), dtype=torch.uint8, device="cuda")

    def run(split):
        _lib.check(L.p2phd_set_option(b"splitk_tail", split))
        try:
            y = torch.empty(N, Ho, Wo, _ops.cpitch(cout), dtype=dtype, device="cuda")
            stats = torch.zeros(N, _ops.cpitch(cout), 2, device="cuda")
            _lib.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(x), _ops.ptr(wp), _ops.ptr(b), 0, _ops.ptr(y), _ops.ptr(stats), _ops.ptr(ws),
                                        _ops.stream_ptr()), "conv_fwd")
            torch.cuda.synchronize()
            return y.float().cpu(), stats.cpu()
        finally:
            _lib.check(L.p2phd_set_option(b"splitk_tail", 1))

    y1, s1 = run(2)                                                # 2 = split as deep as allowed (the default, 1, asks a cost model)
    y0, s0 = run(0)
    y1b, s1b = run(2)
    assert torch.equal(y1, y1b) and torch.equal(s1, s1b)           # fixed summation order: run-to-run identical
    tol = 2e-6 if dtype == torch.float32 else 4e-3                 # bf16: the output rounding may flip on a last-bit difference
    assert rel_err(y1.numpy(), y0.numpy()) < tol
    assert rel_err(s1[..., 0].numpy(), s0[..., 0].numpy()) < 1e-5 and rel_err(s1[..., 1].numpy(), s0[..., 1].numpy()) < 1e-4


@pytest.mark.parametrize("geom", [(256, 256, 3, 1, 1, (2, 32, 16)), (256, 512, 4, 2, 0, (2, 17, 9))], ids=["trunk256", "d256to512"])
def test_fp8_forward_against_an_oracle_fed_the_quantised_operands(geom):
    """BASELINE configs[4] (round-2 review item 5): the e4m3 forward is checked against an fp32 conv of the SAME quantised
    operands -- activations rounded to OCP e4m3 at scale 1, weights to e4m3 at the per-layer scale max|w| / 448 -- so what is
    left is fp32 accumulation order and the bf16 rounding of the output: tolerance 1e-2 (measured ~2e-3), not the 0.2 the
    comparison with the bf16 path needs (that one measures the quantisation itself)."""
    import ctypes as C
    from pix2pixhdaudiosr_amd import _ops, _lib
    cin, cout, k, pad, pad_mode, (N, H, W) = geom
    L = _ops.lib()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * 0.02
    b = torch.randn(cout, generator=g) * 0.1
    spec = _ops.ConvSpec(cin, cout, k, 1, pad, pad_mode, False, 0, False, _ops.ACT_NONE)
    d = spec.desc(N, H, W, torch.bfloat16)
    assert L.p2phd_conv_fp8_eligible(C.byref(d)) == 1
    Ho, Wo = spec.out_size(d)
    xq = x.to(torch.float8_e4m3fn)                                 # RNE, |x| << 448
    x8 = xq.view(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()          # NHWC bytes, channel pitch = cin
    wd = w.cuda()
    wp8 = spec.packed_fp8(wd, d)
    amax = float(w.abs().max())
    wq = (w * (448.0 / amax)).to(torch.float8_e4m3fn).float() * (amax / 448.0)
    y = torch.empty(N, Ho, Wo, _ops.cpitch(cout), dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), 256), dtype=torch.uint8, device="cuda")
    bd = b.cuda()
    _lib.check(L.p2phd_conv_fwd_fp8(C.byref(d), _ops.ptr(x8), _ops.ptr(wp8), _ops.ptr(bd), 0, _ops.ptr(y), None, _ops.ptr(ws),
                                    _ops.stream_ptr()), "conv_fwd_fp8")
    torch.cuda.synchronize()
    xin = xq.float()
    if pad_mode:
        ref = F.conv2d(F.pad(xin, (pad,) * 4, mode="reflect"), wq, b)
    else:
        ref = F.conv2d(xin, wq, b, padding=pad)
    got = y.float().cpu().permute(0, 3, 1, 2)[:, :cout]
    e = rel_err(got.numpy(), ref.numpy())
    print(f"fp8 forward vs oracle on quantised operands: rel L2 {e:.2e}")
    assert e < 1e-2, e


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 1.2e-2)], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", [(64, 128, 3, 1, 1, (2, 12, 10)), (128, 64, 4, 2, 0, (2, 9, 7)), (192, 96, 3, 1, 1, (1, 8, 8))],
                         ids=["c3_reflect", "k4_zero", "odd_channels"])
def test_kmajor_master_weights(dtype, tol, geom):
    """Round 3: optim.FlatAdam keeps the master weights of the big stride-1 layers K-major ([K][R][S][C]) and hands torch a
    permuted view; p2phd_conv_desc.w_layout = 1 selects the cast / per-tap-transpose packs and the row-wise weight-gradient
    landing.  Same layer, same numbers as the PyTorch layout: forward, input gradient, weight gradient (written straight into
    the optimiser's K-major gradient buffer), one Adam step."""
    import ctypes as C
    from pix2pixhdaudiosr_amd import _ops
    from pix2pixhdaudiosr_amd.optim import FlatAdam
    cin, cout, k, pad, pad_mode, (N, H, W) = geom
    spec = _ops.ConvSpec(cin, cout, k, 1, pad, pad_mode, False, 0, True, _ops.ACT_RELU)
    assert _ops.lib().p2phd_conv_kmajor_ok(C.byref(spec.desc(N, H, W, dtype))) == 1
    g = torch.Generator().manual_seed(13)
    x = torch.randn(N, cin, H, W, generator=g)
    w0 = torch.randn(cout, cin, k, k, generator=g) * 0.05
    cot = None
    res = {}
    for layout in (0, 1):
        w = torch.nn.Parameter(w0.clone().cuda())
        if layout:
            w._p2phd_kmajor = True
        opt = FlatAdam([w], lr=1e-3)
        assert _ops.w_layout(w) == layout and _ops.w_layout(w.grad) == layout
        assert torch.equal(w.detach().cpu(), w0)                                   # the view shows the same tensor
        spec = _ops.ConvSpec(cin, cout, k, 1, pad, pad_mode, False, 0, True, _ops.ACT_RELU)
        xd = x.cuda().requires_grad_(True)
        y = _ops.FromPhysical.apply(_ops.conv_block(_ops.ToPhysical.apply(dtype, xd), w, None, spec), cout)
        if cot is None:
            cot = torch.randn(y.shape, generator=g).cuda()
        opt.zero_grad()
        (y * cot).sum().backward()
        gw = w.grad.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        res[layout] = (y.detach().cpu(), xd.grad.cpu(), gw.cpu(), w.detach().cpu().clone())
    for a, b, name in zip(res[1], res[0], ("y", "dx", "dw", "w_after")):
        assert a.shape == b.shape
        e = rel_err(a.numpy(), b.numpy())
        assert e < (tol if name != "w_after" else 1e-3), (name, e)
    if dtype == torch.float32:                                                      # ... and both equal the oracle
        xo, wo = x.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        yo = F.relu(F.instance_norm(F.conv2d(F.pad(xo, (pad,) * 4, mode="reflect") if pad_mode else xo, wo,
                                             padding=0 if pad_mode else pad), eps=1e-5))
        go = torch.autograd.grad((yo * cot.cpu()).sum(), [xo, wo])
        assert rel_err(res[1][0].numpy(), yo.detach().numpy()) < 1e-4
        assert rel_err(res[1][1].numpy(), go[0].numpy()) < 3e-4 and rel_err(res[1][2].numpy(), go[1].numpy()) < 3e-4




@pytest.mark.parametrize("layer", ["conv_transpose_fwd", "conv_s2_dgrad"])
def test_one_spec_at_two_batch_sizes_never_reuses_a_pack_of_the_other_tap_order(layer):
    """Advisor (round 4, high): a tap-skipping merged launch (GDesc::cls_skip) reads the taps of half its sub-pixel classes in
    another order than the plain merged launch, and which of the two a call takes depends on N.  One ConvSpec serving the
    B = 8 training batch, then a B = 1 evaluation batch (train.py:206 -> eval_model), then B = 8 again WITHOUT a weight update
    must give, each time, what a fresh ConvSpec gives; the two packs must be distinct buffers (p2phd_conv_pack_layout)."""
    from pix2pixhdaudiosr_amd import _ops
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    if layer == "conv_transpose_fwd":
        mk = lambda: _ops.ConvSpec(192, 96, 3, 2, 1, 0, True, 1, True, 3)
        w = (torch.randn(192, 96, 3, 3, generator=g) * 0.1).cuda().requires_grad_(True)
        b = (torch.randn(96, generator=g) * 0.1).cuda().requires_grad_(True)
        xs = {n: torch.randn(n, 192, 64, 64, generator=g).cuda() for n in (8, 1)}
    else:
        mk = lambda: _ops.ConvSpec(96, 192, 3, 2, 1, 0, False, 0, True, 3)
        w = (torch.randn(192, 96, 3, 3, generator=g) * 0.1).cuda().requires_grad_(True)
        b = (torch.randn(192, generator=g) * 0.1).cuda().requires_grad_(True)
        xs = {n: torch.randn(n, 96, 128, 128, generator=g).cuda() for n in (8, 1)}

    def run(spec, x):
        xd = x.clone().requires_grad_(True)
        yp = _ops.conv_block(_ops.ToPhysical.apply(dtype, xd), w, b, spec)
        y = _ops.FromPhysical.apply(yp, spec.cout)
        gx, = torch.autograd.grad(y.square().sum(), [xd])
        return y.detach().float(), gx.float()

    shared = mk()
    ids = set()
    for n in (8, 1, 8, 1):
        d = shared.desc(n, xs[n].shape[2], xs[n].shape[3], dtype)
        ids.add(_ops.lib_for(dtype).p2phd_conv_pack_layout(_ops.C.byref(d), 0 if layer == "conv_transpose_fwd" else 1))
        got = run(shared, xs[n])
        want = run(mk(), xs[n])
        for a, e, what in zip(got, want, ("y", "dx")):
            assert torch.equal(a, e), (layer, n, what, rel_err(a.cpu().numpy(), e.cpu().numpy()))
    assert ids == {0, 1}, ids                   # the case does exercise both layouts
    which = 0 if layer == "conv_transpose_fwd" else 1
    bufs = [v[1].data_ptr() for k, v in shared._packed.items() if k[0] == which]
    assert len(bufs) == 2 and bufs[0] != bufs[1]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_dfirst_kernel_equals_the_generic_path(dtype):
    """Round 5: csrc/dfirst.hip (option dfirst = 1: the discriminator's 4 -> 64 first layer with the input pixels loaded straight
    into MFMA fragments) against the generic gather-GEMM path it replaces (option 0), at the layer's real plane of the second
    scale (256 x 128 -> 129 x 65) and on an odd plane: same products, fp32 accumulation in another order -> equal to the 16-bit
    rounding of the output; and against the fp32 oracle.  The kernel has no tanh: a tanh layer of that shape takes the generic
    path under both settings."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    import ctypes as C
    L = _ops.lib_for(dtype)
    for (N, H, W, act) in ((4, 256, 128, _ops.ACT_LRELU), (3, 37, 51, _ops.ACT_LRELU), (3, 37, 51, _ops.ACT_TANH)):
        gen = torch.Generator().manual_seed(H)
        spec = _ops.ConvSpec(4, 64, 4, 2, 2, 0, False, 0, False, act)
        d = spec.desc(N, H, W, dtype)
        Ho, Wo = spec.out_size(d)
        xc = torch.randn(N, 4, H, W, generator=gen)
        x = _ops.ToPhysical.apply(dtype, xc.cuda())
        w = (torch.randn(64, 4, 4, 4, generator=gen) * 0.1).cuda()
        b = (torch.randn(64, generator=gen) * 0.1).cuda()
        y = torch.empty(N, Ho, Wo, 64, device="cuda", dtype=dtype)
        wp = spec.packed(w, 0, d)
        ws = _ops.workspace(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), 1 << 20), "cuda")
        res = {}
        try:
            for opt in (0, 1):
                _lib.check(L.p2phd_set_option(b"dfirst", opt))
                y.fill_(7.0)
                _ops.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(x), _ops.ptr(wp), _ops.ptr(b), act, _ops.ptr(y), None, _ops.ptr(ws), _ops.stream_ptr()))
                torch.cuda.synchronize()
                res[opt] = y.float().cpu().numpy().copy()
        finally:
            _lib.check(L.p2phd_set_option(b"dfirst", 1))
        q = lambda t: t.to(dtype).float()
        z = F.conv2d(q(xc), q(w.cpu()), b.cpu(), stride=2, padding=2)
        ref = (F.leaky_relu(z, 0.2) if act == _ops.ACT_LRELU else torch.tanh(z)).permute(0, 2, 3, 1).numpy()
        ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        assert rel_err(res[1], res[0]) < ulp, rel_err(res[1], res[0])
        assert rel_err(res[1], ref) < 2 * ulp and rel_err(res[0], ref) < 2 * ulp, (rel_err(res[1], ref), rel_err(res[0], ref))
        assert np.abs(res[1] - ref).max() <= 4 * ulp * np.abs(ref).max()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_dlast_kernels_equal_the_wfold_path(dtype):
    """Round 5: csrc/dlast.hip (option dlast = 1) against the W-fold gather-GEMM launches it replaces (0) on the discriminator's
    head at its real second-scale plane (512 channels, 33 x 17 -> 34 x 18) and an odd one: forward with bias, input gradient with
    an addend, and the input gradient carrying the producer's InstanceNorm-backward sums (p2phd_conv_dgrad_bsum): outputs equal
    to the 16-bit rounding (other summation order over the 8192 products), the fp32 sums to accumulation noise."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    import ctypes as C
    L = _ops.lib_for(dtype)
    for (N, H, W, CH) in ((6, 33, 17, 512), (2, 9, 23, 256)):
        gen = torch.Generator().manual_seed(H + CH)
        spec = _ops.ConvSpec(CH, 1, 4, 1, 2, 0, False, 0, False, _ops.ACT_NONE)
        d = spec.desc(N, H, W, dtype)
        Ho, Wo = spec.out_size(d)
        x = torch.randn(N, H, W, CH, generator=gen).cuda().to(dtype)
        w = (torch.randn(1, CH, 4, 4, generator=gen) * 0.05).cuda()
        b = (torch.randn(1, generator=gen)).cuda()
        dy = torch.zeros(N, Ho, Wo, 8, device="cuda", dtype=dtype)
        dy[..., 0] = torch.randn(N, Ho, Wo, generator=gen).cuda().to(dtype)
        addend = torch.randn(N, H, W, CH, generator=gen).cuda().to(dtype)
        prev_y = torch.randn(N, H, W, CH, generator=gen).cuda().to(dtype)
        prev_stats = torch.zeros(N, CH, 2, device="cuda"); prev_stats[..., 0] = 0.1; prev_stats[..., 1] = H * W * 1.3
        y = torch.empty(N, Ho, Wo, 8, device="cuda", dtype=dtype)
        gx = torch.empty_like(x); gx2 = torch.empty_like(x)
        bst = torch.zeros(N, CH, 2, device="cuda")
        wp0, wp1 = spec.packed(w, 0, d), spec.packed(w, 1, d)
        ws = _ops.workspace(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), L.p2phd_conv_dgrad_workspace_bytes(C.byref(d)),
                                L.p2phd_conv_dgrad_bsum_workspace_bytes(C.byref(d)), 1 << 20), "cuda")
        res = {}
        try:
            for opt in (0, 1):
                _lib.check(L.p2phd_set_option(b"dlast", opt))
                y.fill_(3.0); gx.fill_(3.0); gx2.fill_(3.0)
                _ops.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(x), _ops.ptr(wp0), _ops.ptr(b), 0, _ops.ptr(y), None, _ops.ptr(ws), _ops.stream_ptr()))
                _ops.check(L.p2phd_conv_dgrad(C.byref(d), _ops.ptr(dy), _ops.ptr(wp1), _ops.ptr(addend), _ops.ptr(gx), _ops.ptr(ws), _ops.stream_ptr()))
                _ops.check(L.p2phd_conv_dgrad_bsum(C.byref(d), _ops.ptr(dy), _ops.ptr(wp1), None, _ops.ptr(gx2), _ops.ptr(prev_y), _ops.ptr(prev_stats),
                                                   _ops.ACT_LRELU, 1e-5, _ops.ptr(bst), _ops.ptr(ws), _ops.stream_ptr()))
                torch.cuda.synchronize()
                res[opt] = (y.float().cpu().numpy().copy(), gx.float().cpu().numpy().copy(), gx2.float().cpu().numpy().copy(), bst.cpu().numpy().copy())
        finally:
            _lib.check(L.p2phd_set_option(b"dlast", 1))
        ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
        assert np.abs(res[1][0][..., 1:]).max() == 0.0                   # pad channels of the 1-channel output stay zero
        for i, what in ((0, "y"), (1, "dx + addend"), (2, "dx (fused sums)")):
            assert rel_err(res[1][i], res[0][i]) < ulp, (what, rel_err(res[1][i], res[0][i]))
            assert np.abs(res[1][i] - res[0][i]).max() <= 2 * ulp * np.abs(res[0][i]).max(), what
        assert rel_err(res[1][3], res[0][3]) < 2e-2 * (1 if dtype == torch.bfloat16 else 0.2), rel_err(res[1][3], res[0][3])   # sums of ROUNDED gradients that differ in the last bit
        # against the fp32 oracle on the rounded operands
        q = lambda t: t.float().cpu()
        xr = q(x).permute(0, 3, 1, 2)
        wq = w.cpu().to(dtype).float()
        yo = F.conv2d(xr, wq, b.cpu(), padding=2)
        assert rel_err(res[1][0][..., 0], yo[:, 0].numpy()) < 2 * ulp
        gxo = F.conv_transpose2d(q(dy)[..., 0].unsqueeze(1), wq, padding=2).permute(0, 2, 3, 1)
        assert rel_err(res[1][2], gxo.numpy()) < 2 * ulp


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dfirst_and_dlast_on_random_planes(seed):
    """Round 5: csrc/dfirst.hip / csrc/dlast.hip on planes of random size (odd, tiny, non-multiples of the 16-pixel block; batches that do
    not fill a wave's run of blocks) against torch's fp32 convolution of the bf16-rounded operands: forward of both, input gradient
    of the head with and without an addend.  The kernels index a FLATTENED pixel axis (dfirst, dlast forward) or per-sample runs of
    16-pixel blocks (dlast input gradient): every boundary between rows, samples and the padded tail is hit somewhere here."""
    from pix2pixhdaudiosr_amd import _ops
    import ctypes as C
    dtype = torch.bfloat16
    L = _ops.lib_for(dtype)
    rng = np.random.RandomState(100 + seed)
    q = lambda t: t.to(dtype).float()
    ulp = 2.0 ** -8
    for _ in range(6):
        N, H, W = int(rng.randint(1, 5)), int(rng.randint(2, 40)), int(rng.randint(2, 40))
        gen = torch.Generator().manual_seed(int(rng.randint(1 << 30)))
        # first layer: C in {1..4} -> 64, 4 x 4 stride 2 pad 2, LeakyReLU
        cin = int(rng.randint(1, 5))
        spec = _ops.ConvSpec(cin, 64, 4, 2, 2, 0, False, 0, False, _ops.ACT_LRELU)
        d = spec.desc(N, H, W, dtype)
        Ho, Wo = spec.out_size(d)
        xc = torch.randn(N, cin, H, W, generator=gen)
        w = torch.randn(64, cin, 4, 4, generator=gen) * 0.1
        b = torch.randn(64, generator=gen) * 0.1
        x = _ops.ToPhysical.apply(dtype, xc.cuda())
        y = torch.full((N, Ho, Wo, 64), 9.0, device="cuda", dtype=dtype)
        ws = _ops.workspace(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), 1 << 16), "cuda")
        _ops.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(x), _ops.ptr(spec.packed(w.cuda(), 0, d)), _ops.ptr(b.cuda()), _ops.ACT_LRELU, _ops.ptr(y), None,
                                    _ops.ptr(ws), _ops.stream_ptr()))
        ref = F.leaky_relu(F.conv2d(q(xc), q(w), b, stride=2, padding=2), 0.2).permute(0, 2, 3, 1).numpy()
        assert rel_err(y.float().cpu().numpy(), ref) < 2 * ulp, ("dfirst", N, H, W, cin)
        # head: C in {128, 256, 384, 512} -> 1, 4 x 4 stride 1 pad 2
        ch = int(rng.choice([128, 256, 384, 512]))
        spec = _ops.ConvSpec(ch, 1, 4, 1, 2, 0, False, 0, False, _ops.ACT_NONE)
        d = spec.desc(N, H, W, dtype)
        Ho, Wo = spec.out_size(d)
        xh = torch.randn(N, H, W, ch, generator=gen).cuda().to(dtype)
        wh = torch.randn(1, ch, 4, 4, generator=gen) * 0.05
        bh = torch.randn(1, generator=gen)
        yh = torch.full((N, Ho, Wo, 8), 9.0, device="cuda", dtype=dtype)
        ws = _ops.workspace(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), L.p2phd_conv_dgrad_workspace_bytes(C.byref(d)), 1 << 16), "cuda")
        _ops.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(xh), _ops.ptr(spec.packed(wh.cuda(), 0, d)), _ops.ptr(bh.cuda()), 0, _ops.ptr(yh), None, _ops.ptr(ws),
                                    _ops.stream_ptr()))
        refh = F.conv2d(xh.float().cpu().permute(0, 3, 1, 2), q(wh), bh, padding=2)[:, 0].numpy()
        got = yh.float().cpu().numpy()
        assert np.abs(got[..., 1:]).max() == 0.0
        assert rel_err(got[..., 0], refh) < 2 * ulp, ("dlast fwd", N, H, W, ch)
        dy = torch.zeros(N, Ho, Wo, 8, device="cuda", dtype=dtype)
        dyc = torch.randn(N, Ho, Wo, generator=gen)
        dy[..., 0] = dyc.cuda().to(dtype)
        addend = torch.randn(N, H, W, ch, generator=gen).cuda().to(dtype)
        for add in (None, addend):
            gx = torch.full((N, H, W, ch), 9.0, device="cuda", dtype=dtype)
            _ops.check(L.p2phd_conv_dgrad(C.byref(d), _ops.ptr(dy), _ops.ptr(spec.packed(wh.cuda(), 1, d)), _ops.ptr(add), _ops.ptr(gx), _ops.ptr(ws),
                                          _ops.stream_ptr()))
            refg = q(F.conv_transpose2d(q(dyc).unsqueeze(1), q(wh), padding=2).permute(0, 2, 3, 1))
            if add is not None:
                refg = refg + add.float().cpu()
            assert rel_err(gx.float().cpu().numpy(), refg.numpy()) < 2 * ulp, ("dlast dgrad", N, H, W, ch, add is not None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_tile128x192_equals_the_128x128_tile(dtype):
    """Round 5: the 128 x 192 tile (option tile128x192 = 1) that the 1536-channel trunk of the two-scale generator takes on its
    16 x 8 plane (configs[2]/[3]) against the 128 x 128 tile (0): the K order of every output element is the same in both, so the
    outputs and the InstanceNorm partial sums are equal BIT FOR BIT; the launch counter shows which tile ran."""
    from pix2pixhdaudiosr_amd import _ops, _lib
    import ctypes as C
    L = _ops.lib_for(dtype)
    N, H, W, cin, cout = 32, 16, 8, 192, 1536
    gen = torch.Generator().manual_seed(5)
    spec = _ops.ConvSpec(cin, cout, 3, 1, 1, 1, False, 0, True, _ops.ACT_RELU)
    d = spec.desc(N, H, W, dtype)
    x = torch.randn(N, H, W, cin, generator=gen).to(dtype).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * 0.05).cuda()
    y = torch.empty(N, H, W, cout, device="cuda", dtype=dtype)
    stats = torch.zeros(N, cout, 2, device="cuda")
    wp = spec.packed(w, 0, d)
    ws = _ops.workspace(max(L.p2phd_conv_fwd_workspace_bytes(C.byref(d)), 1 << 20), "cuda")
    res, cnt = {}, {}
    try:
        _lib.check(L.p2phd_set_option(b"splitk_tail", 0))        # (a split-K tail of the 128 x 128 grid would sum K in two parts)
        for opt in (0, 1):
            _lib.check(L.p2phd_set_option(b"tile128x192", opt))
            L.p2phd_launch_count(None, 1)
            y.fill_(7.0); stats.zero_()
            _ops.check(L.p2phd_conv_fwd(C.byref(d), _ops.ptr(x), _ops.ptr(wp), None, 0, _ops.ptr(y), _ops.ptr(stats), _ops.ptr(ws), _ops.stream_ptr()))
            torch.cuda.synchronize()
            cnt[opt] = L.p2phd_launch_count(b"tile128x192", 0)
            res[opt] = (y.clone(), stats.clone())
    finally:
        _lib.check(L.p2phd_set_option(b"tile128x192", 1))
        _lib.check(L.p2phd_set_option(b"splitk_tail", 1))
    assert cnt == {0: 0, 1: 1}, cnt
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    ref = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect"), w.to(dtype).float()).permute(0, 2, 3, 1)
    assert rel_err(res[1][0].float().cpu().numpy(), ref.cpu().numpy()) < (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -10)
