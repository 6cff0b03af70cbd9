"""Exact integer-operand tests of every conv kernel family, per element (tests/_exact.py states the argument).

Straight through the C ABI, one launch per check: operands are small integers chosen so that every partial sum is an integer
the storage format holds, the expected output is that integer -- one bit pattern per element, pad channels included --, the
output / workspace / gradient buffers sit between canaries, the workspace has exactly the size the library reports, and the
launch counters prove which kernel family ran.  The packed weights of every forward and input-gradient call come from the C
entry, into a guarded buffer of exactly the reported size that held 0xFF (NaN in every float type, a non-zero e4m3 byte) before
the pack: a launch that reads a byte the pack left unwritten cannot produce the integers.  Where an option selects between a dedicated kernel and the path behind it,
both settings run: both equal the integers, hence each other.  InstanceNorm statistics and the fused backward sums are not
exact; their bounds are derived in the helper."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import _exact as X
import _wpack as P

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
HALF = ["bf16", "f16"]
FAMILIES = ("gconv", "halo", "cls_skip", "splitk", "tile256", "tile128x192", "march", "march_w", "wgrad", "dfirst", "dlast", "c7",
            "thin_wgrad")
DEFAULTS = dict(march=1, dfirst=1, dlast=1, c7_generic=0, reflect_generic=0, gconv_halo=1, cls_skip=1, tile128x192=1,
                splitk_tail=1, gconv_bm=0, wgrad_tm=0, wgrad_xcd=1)
NONE, LRELU, RELU = 0, 1, 3


def _ops():
    from pix2pixhdaudiosr_amd import _ops
    return _ops


@contextlib.contextmanager
def options(Lb, **kw):
    """p2phd_set_option for the block, defaults restored behind it."""
    ops = _ops()
    try:
        for k, v in kw.items():
            ops.check(Lb.p2phd_set_option(k.encode(), v), k)
        yield
    finally:
        for k in kw:
            ops.check(Lb.p2phd_set_option(k.encode(), DEFAULTS[k]), k)


def _setup(l, dtype):
    ops = _ops()
    spec = ops.ConvSpec(l.cin, l.cout, l.k, l.stride, l.pad, l.pad_mode, l.transposed, l.opad, False, NONE)
    N, H, W = l.shape
    return ops, ops.lib_for(dtype), spec


def _count(Lb):
    return {f: int(Lb.p2phd_launch_count(f.encode(), 0)) for f in FAMILIES}


def _vp(g):
    return C.c_void_p(g.ptr())


def _packed(ops, Lb, d, which, w, bufs):
    """The layer's pack for the launch: p2phd_conv_pack_weights into a 0xFF-prefilled guarded buffer (which = "fp8": the e4m3
    pack), entered into `bufs` so that its guards are checked with the others."""
    g = P.pack_guarded_fp8(ops, Lb, d, w) if which == "fp8" else P.pack_guarded(ops, Lb, d, which, w)
    X.check_guards({"packed": g}, f"pack_weights which={which}")
    bufs["packed"] = g
    return g


def _check_stats(st, y_want, what):
    mean, m2, bm, b2 = X.stats_reference(y_want)
    K = y_want.shape[1]
    got = st.cpu().double()[:, :K]
    em, e2 = (got[..., 0] - mean).abs(), (got[..., 1] - m2).abs()
    assert bool((em <= bm).all()), (what, "mean", float((em - bm).max()))
    assert bool((e2 <= b2).all()), (what, "M2", float((e2 - b2).max()))


def run_fwd(l, dt, act=NONE, stats=False, layout=0):
    """p2phd_conv_fwd on the integer operands of (l, "fwd"); returns the launch counters of the call."""
    dtype = DT[dt]
    ops, Lb, spec = _setup(l, dtype)
    o = X.operands(l, "fwd")
    N, H, W = l.shape
    d = spec.desc(N, H, W, dtype, layout)
    Ho, Wo = spec.out_size(d)
    assert (Ho, Wo) == X.out_hw(l)
    x = X.to_nhwc(o["x"], dtype).cuda()
    w = o["w"].cuda()
    if layout == 1:
        w = w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                       # K-major master weights
    b = o["b"].cuda()
    ws = X.guarded(Lb.p2phd_conv_fwd_workspace_bytes(C.byref(d)))
    gy, y = X.guarded_like((N, Ho, Wo, X.cpitch(l.cout)), dtype)
    bufs = {"y": gy, "workspace": ws}
    wp = _packed(ops, Lb, d, 0, w, bufs)
    st = None
    if stats:
        bufs["stats"], st = X.guarded_like((N, X.cpitch(l.cout), 2), torch.float32)
    what = f"fwd {l.name} {dt} act={act} stats={stats}"
    Lb.p2phd_launch_count(None, 1)
    ops.check(Lb.p2phd_conv_fwd(C.byref(d), ops.ptr(x), _vp(wp), ops.ptr(b), act, ops.ptr(y), ops.ptr(st), _vp(ws), ops.stream_ptr()), what)
    torch.cuda.synchronize()
    cnt = _count(Lb)
    X.check_guards(bufs, what)
    want = o["want"].clamp(min=0) if act == RELU else o["want"]
    X.assert_bits_equal(y, want, "nhwc", what)
    if stats:
        _check_stats(st, o["want"], what)
    return cnt


def run_dgrad(l, dt, add=False, mode="plain", prev_act=RELU, layout=0):
    """p2phd_conv_dgrad (mode "plain"), _dgrad_rx ("rx": extras built on the host), _dgrad_act ("act") or _dgrad_bsum ("bsum")."""
    dtype = DT[dt]
    ops, Lb, spec = _setup(l, dtype)
    o = X.operands(l, "dgrad_add" if add else "dgrad")
    N, H, W = l.shape
    d = spec.desc(N, H, W, dtype, layout)
    Ho, Wo = spec.out_size(d)
    dyh = X.to_nhwc(o["dy"], dtype)
    w = o["w"].cuda()
    if layout == 1:
        w = w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                       # K-major master weights
    addend = X.to_nhwc(o["addend"], dtype).cuda() if add else None
    Cp = X.cpitch(l.cin)
    gx, dx = X.guarded_like((N, H, W, Cp), dtype)
    bufs = {"dx": gx}
    wp = _packed(ops, Lb, d, 1, w, bufs)
    what = f"dgrad[{mode}] {l.name} {dt} addend={add}"
    want = o["want"]
    gen = torch.Generator().manual_seed(N * H + W)
    Lb.p2phd_launch_count(None, 1)
    if mode == "plain":
        dy = dyh.cuda()
        ws = bufs["workspace"] = X.guarded(Lb.p2phd_conv_dgrad_workspace_bytes(C.byref(d)))
        ops.check(Lb.p2phd_conv_dgrad(C.byref(d), ops.ptr(dy), _vp(wp), ops.ptr(addend), ops.ptr(dx), _vp(ws), ops.stream_ptr()), what)
    elif mode == "rx":
        ex = X.reflect_extras(dyh)                                                       # pair sums of integers: integers, exact in 16 bits
        n_rx = Lb.p2phd_conv_reflect_extras_elems(C.byref(d))
        assert n_rx == ex.numel() == N * (2 * (W + 2) + 2 * H) * X.cpitch(l.cout), (what, n_rx, ex.numel())
        dy = torch.cat([dyh.reshape(-1), ex.to(dtype).reshape(-1)]).cuda()
        ops.check(Lb.p2phd_conv_dgrad_rx(C.byref(d), ops.ptr(dy), _vp(wp), ops.ptr(addend), ops.ptr(dx), ops.stream_ptr()), what)
    else:
        dy = dyh.cuda()
        assert Lb.p2phd_conv_dgrad_bsum_ok(C.byref(d)) == 1, what
        ws = bufs["workspace"] = X.guarded(Lb.p2phd_conv_dgrad_bsum_workspace_bytes(C.byref(d)))
        prev = X.int_tensor((N, l.cin, H, W), -3, 3, 0.8, gen)
        prev_p = X.to_nhwc(prev, dtype).cuda()
        if mode == "act":
            ops.check(Lb.p2phd_conv_dgrad_act(C.byref(d), ops.ptr(dy), _vp(wp), ops.ptr(addend), ops.ptr(dx), ops.ptr(prev_p), prev_act, _vp(ws),
                                              ops.stream_ptr()), what)
        else:
            mean = X.int_tensor((N, l.cin), -1, 1, 0.5, gen)
            m2 = (H * W) * (0.5 + 3.0 * torch.rand((N, l.cin), generator=gen))
            pst = torch.zeros(N, Cp, 2)
            pst[:, :l.cin, 0], pst[:, :l.cin, 1] = mean, m2
            pst = pst.cuda()
            bufs["bstats"], bst = X.guarded_like((N, Cp, 2), torch.float32)
            ops.check(Lb.p2phd_conv_dgrad_bsum(C.byref(d), ops.ptr(dy), _vp(wp), ops.ptr(addend), ops.ptr(dx), ops.ptr(prev_p), ops.ptr(pst), prev_act,
                                               1e-5, ops.ptr(bst), _vp(ws), ops.stream_ptr()), what)
    torch.cuda.synchronize()
    cnt = _count(Lb)
    X.check_guards(bufs, what)
    if mode == "act":
        slope = 0.0 if prev_act == RELU else 0.2
        exp = X.act_bwd_reference(X.to_nhwc(want, torch.float32), X.to_nhwc(prev, torch.float32), slope, dtype)
        X.assert_bits_equal(dx, exp, "flat", what)
        return cnt
    X.assert_bits_equal(dx, want, "nhwc", what)
    if mode == "bsum":
        slope = {RELU: 0.0, LRELU: 0.2, NONE: 1.0}[prev_act]
        s1, s2, b1, b2 = X.bsum_reference(want, prev, pst[:, :l.cin, 0].cpu(), pst[:, :l.cin, 1].cpu(), 1e-5, slope)
        got = bst.cpu().double()
        e1, e2 = (got[:, :l.cin, 0] - s1).abs(), (got[:, :l.cin, 1] - s2).abs()
        assert bool((e1 <= b1).all()), (what, "sum g'", float((e1 - b1).max()))
        assert bool((e2 <= b2).all()), (what, "sum g' yhat", float((e2 - b2).max()))
        assert float(got[:, l.cin:].abs().max()) == 0.0 if Cp > l.cin else True, (what, "pad channels of bstats")
    return cnt


def run_wgrad(l, dt, acc=False, layout=0):
    """p2phd_conv_wgrad / _wgrad_acc (onto an integer prefill) with db."""
    dtype = DT[dt]
    ops, Lb, spec = _setup(l, dtype)
    o = X.operands(l, "wgrad")
    N, H, W = l.shape
    d = spec.desc(N, H, W, dtype, layout)
    x = X.to_nhwc(o["x"], dtype).cuda()
    dy = X.to_nhwc(o["dy"], dtype).cuda()
    want_w, want_b = o["want"]
    dw0, db0 = o["dw0"], o["db0"]
    if not acc:
        want_w, want_b = want_w - dw0, want_b - db0
    mem = (lambda t: t.permute(0, 2, 3, 1).contiguous()) if layout == 1 else (lambda t: t.contiguous())
    gw, dw = X.guarded_like(tuple(mem(dw0).shape), torch.float32)
    gb, db = X.guarded_like((l.cout,), torch.float32)
    if acc:
        dw.copy_(mem(dw0)); db.copy_(db0)
    ws = X.guarded(Lb.p2phd_conv_wgrad_workspace_bytes(C.byref(d)))
    what = f"wgrad{'_acc' if acc else ''} {l.name} {dt} w_layout={layout}"
    fn = Lb.p2phd_conv_wgrad_acc if acc else Lb.p2phd_conv_wgrad
    Lb.p2phd_launch_count(None, 1)
    ops.check(fn(C.byref(d), ops.ptr(x), ops.ptr(dy), ops.ptr(dw), ops.ptr(db), _vp(ws), ops.stream_ptr()), what)
    torch.cuda.synchronize()
    cnt = _count(Lb)
    X.check_guards({"dw": gw, "db": gb, "workspace": ws}, what)
    X.assert_bits_equal(dw, mem(want_w), "flat", what + " dw")
    X.assert_bits_equal(db, want_b, "flat", what + " db")
    return cnt


def _dedicated_idle(cnt, what):
    for f in ("march", "march_w", "dfirst", "dlast", "c7", "thin_wgrad"):
        assert cnt[f] == 0, (what, f, cnt)


# ----------------------------------------------------------------------------------------------------------------------
# generic gather-GEMM
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("l", X.GENERIC, ids=lambda l: l.name)
def test_generic_gather_gemm(l, dt):
    Lb = _ops().lib_for(DT[dt])
    big_plane = l.shape[1] * l.shape[2] >= 64
    for act, stats in ((NONE, False), (RELU, False)) + (((NONE, True),) if big_plane else ()):
        cnt = run_fwd(l, dt, act, stats)
        assert cnt["gconv"] >= 1, (l.name, cnt)
        _dedicated_idle(cnt, l.name)
    for add in (False, True):
        for generic in ((0, 1) if l.pad_mode else (0,)):                                   # exact-grid reflect gradient and padded grid + fold
            with options(Lb, reflect_generic=generic):
                cnt = run_dgrad(l, dt, add)
            assert cnt["gconv"] >= 1, (l.name, cnt)
            _dedicated_idle(cnt, l.name)
    if not l.pad_mode:
        for mode, act in (("act", RELU), ("act", LRELU), ("bsum", RELU), ("bsum", LRELU)):
            if mode == "bsum" and not big_plane:
                continue
            for add in (False, True):
                cnt = run_dgrad(l, dt, add, mode, act)
                assert cnt["gconv"] >= 1, (l.name, mode, cnt)


@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("bm", [128, 192, 256, 258, 512])
def test_every_forced_tile_height(bm, dt):
    Lb = _ops().lib_for(DT[dt])
    by_name = {l.name: l for l in X.GENERIC}
    for name in ("tile_72to384", "wide_k200_c136", "tile_64to64_s2", "big_m_tiles"):
        l = by_name[name]
        with options(Lb, gconv_bm=bm):
            cf = run_fwd(l, dt, NONE, True)
            cg = run_dgrad(l, dt, True)
        assert cf["gconv"] >= 1 and cg["gconv"] >= 1, (name, bm, cf, cg)
        if bm == 512 and dt != "f32" and name == "tile_72to384":
            assert cf["tile256"] == 1, (name, cf)


# ----------------------------------------------------------------------------------------------------------------------
# HALO loop, 128 x 192 / 256 x 256 tiles, split-K tail, tap-skipping merged launches
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.HALO_FWD, ids=lambda l: l.name)
def test_halo_loop_forward(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for halo in (1, 0):
        with options(Lb, gconv_halo=halo):
            cnt = run_fwd(l, dt, NONE, True)
        assert cnt["halo"] == halo and cnt["gconv"] == 1, (l.name, halo, cnt)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.HALO_DGRAD, ids=lambda l: l.name)
def test_halo_loop_input_gradient_through_the_reflection_extras(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for halo in (1, 0):
        with options(Lb, gconv_halo=halo):
            for add in (False, True):
                cnt = run_dgrad(l, dt, add, "rx")
                assert cnt["halo"] == halo and cnt["gconv"] == 1, (l.name, halo, cnt)


@pytest.mark.parametrize("dt", HALF)
def test_tile128x192(dt):
    Lb = _ops().lib_for(DT[dt])
    for on in (1, 0):
        with options(Lb, tile128x192=on, splitk_tail=0):
            cf = run_fwd(X.TILE128X192_FWD, dt, NONE, True)
            cg = run_dgrad(X.TILE128X192_DGRAD, dt, False, "bsum", RELU)
        assert cf["tile128x192"] == on and cg["tile128x192"] == on, (on, cf, cg)


@pytest.mark.parametrize("dt", HALF)
def test_tile256(dt):
    Lb = _ops().lib_for(DT[dt])
    for bm in (512, 0):
        with options(Lb, gconv_bm=bm):
            cf = run_fwd(X.TILE256, dt, RELU, False)
            cg = run_dgrad(X.TILE256, dt, False)
        if bm == 512:
            assert cf["tile256"] == 1 and cg["tile256"] == 1, (cf, cg)


@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("l", X.SPLITK, ids=lambda l: l.name)
def test_split_k_tail(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for split in (2, 0):
        with options(Lb, splitk_tail=split):
            cnt = run_fwd(l, dt, NONE, True)
            run_dgrad(l, dt, False)
        assert (cnt["splitk"] >= 1) == (split == 2), (l.name, split, cnt)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.CLS_SKIP_FWD + X.CLS_SKIP_DGRAD, ids=lambda l: l.name)
def test_tap_skipping_merged_stride2_launches(l, dt):
    ops = _ops()
    Lb = ops.lib_for(DT[dt])
    fwd = l.transposed
    for n, skip in ((l.shape[0], 1), (l.shape[0], 0), (1, 1)):
        ll = l if n == l.shape[0] else X.at_batch(l, 1)
        with options(Lb, cls_skip=skip):
            spec = ops.ConvSpec(l.cin, l.cout, l.k, l.stride, l.pad, l.pad_mode, l.transposed, l.opad, False, NONE)
            d = spec.desc(n, l.shape[1], l.shape[2], DT[dt])
            layout = Lb.p2phd_conv_pack_layout(C.byref(d), 0 if fwd else 1)
            cnt = run_fwd(ll, dt, NONE, True) if fwd else run_dgrad(ll, dt, False)
        expect = 1 if (skip and n > 1) else 0                                              # N = 1: too few tiles, the other pack layout
        assert layout == expect and cnt["cls_skip"] == expect and cnt["gconv"] >= 1, (ll.name, skip, layout, cnt)


# ----------------------------------------------------------------------------------------------------------------------
# marching kernels, weight gradients
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.MARCH_CONV + X.MARCH_CONVT, ids=lambda l: l.name)
def test_marching_kernels(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for march in (1, 0):
        with options(Lb, march=march):
            for stats in (True, False):
                cnt = run_fwd(l, dt, NONE, stats)
                assert cnt["march"] == march and (cnt["gconv"] >= 1) == (march == 0), (l.name, "fwd", march, cnt)
            cnt = run_dgrad(l, dt, False)
            assert cnt["march"] == march, (l.name, "dgrad", march, cnt)
            cnt = run_dgrad(l, dt, False, "bsum", RELU)
            assert cnt["march"] == march, (l.name, "dgrad_bsum", march, cnt)
            cnt = run_dgrad(l, dt, True)                                                   # with an addend: always the gather-GEMM
            assert cnt["march"] == 0 and cnt["gconv"] >= 1, (l.name, "dgrad + addend", cnt)
            for acc in (False, True):
                cnt = run_wgrad(l, dt, acc)
                assert cnt["march_w"] == march and cnt["wgrad"] == 1 - march, (l.name, "wgrad", march, cnt)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.THIN, ids=lambda l: l.name)
def test_thin_weight_gradient(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for generic in (0, 1):
        with options(Lb, c7_generic=generic):
            for acc in (False, True):
                cnt = run_wgrad(l, dt, acc)
                assert cnt["thin_wgrad"] == 1 - generic and cnt["wgrad"] == generic, (l.name, generic, cnt)


@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("l", X.WGRAD, ids=lambda l: l.name)
def test_mfma_weight_gradient(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for tm, xcd in ((0, 1), (128, 1), (0, 0)):
        with options(Lb, wgrad_tm=tm, wgrad_xcd=xcd):
            for acc in (False, True):
                cnt = run_wgrad(l, dt, acc)
                assert cnt["wgrad"] == 1 and cnt["thin_wgrad"] == 0 and cnt["march_w"] == 0, (l.name, tm, xcd, cnt)


@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("l", X.WGRAD_KMAJOR, ids=lambda l: l.name)
def test_kmajor_master_weights(l, dt):
    """w_layout = 1: the cast / per-tap-transpose packs copy small integers exactly (forward on the packed K-major weights),
    and the weight gradient lands K-major."""
    Lb = _ops().lib_for(DT[dt])
    for layout in (1, 0):
        for acc in (False, True):
            cnt = run_wgrad(l, dt, acc, layout)
            assert cnt["wgrad"] == 1, (l.name, layout, cnt)
    small = X.at_batch(l, 2)
    assert Lb.p2phd_conv_kmajor_ok(C.byref(_setup(small, DT[dt])[2].desc(*small.shape, DT[dt]))) == 1
    assert run_fwd(small, dt, NONE, True, layout=1)["gconv"] == 1
    for add in (False, True):
        assert run_dgrad(small, dt, add, layout=1)["gconv"] >= 1


# ----------------------------------------------------------------------------------------------------------------------
# dedicated single-layer kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.DFIRST, ids=lambda l: l.name)
def test_dfirst(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for on in (1, 0):
        with options(Lb, dfirst=on):
            for act in (NONE, RELU):
                cnt = run_fwd(l, dt, act, False)
                assert cnt["dfirst"] == on and (cnt["gconv"] >= 1) == (on == 0), (l.name, on, cnt)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.DLAST, ids=lambda l: l.name)
def test_dlast(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for on in (1, 0):
        with options(Lb, dlast=on):
            cnt = run_fwd(l, dt, NONE, False)
            assert cnt["dlast"] == on and (cnt["gconv"] >= 1) == (on == 0), (l.name, "fwd", on, cnt)
            for add in (False, True):
                cnt = run_dgrad(l, dt, add)
                assert cnt["dlast"] == on, (l.name, "dgrad", on, cnt)
                cnt = run_dgrad(l, dt, add, "bsum", LRELU)
                assert cnt["dlast"] == on, (l.name, "dgrad_bsum", on, cnt)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("l", X.C7_IN + X.C7_OUT, ids=lambda l: l.name)
def test_c7(l, dt):
    Lb = _ops().lib_for(DT[dt])
    for generic in (0, 1):
        with options(Lb, c7_generic=generic):
            cnt = run_fwd(l, dt, NONE, l.cin == 2)                                         # 2 -> K with statistics; K -> 2: act NONE
            assert cnt["c7"] == 1 - generic and (cnt["gconv"] >= 1) == (generic == 1), (l.name, "fwd", generic, cnt)
            if l.cout == 2:
                cnt = run_dgrad(l, dt, False)
                assert cnt["c7"] == 1 - generic, (l.name, "dgrad", generic, cnt)


# ----------------------------------------------------------------------------------------------------------------------
# e4m3 forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", X.FP8, ids=lambda l: l.name)
def test_e4m3_forward(l):
    """x: integers in -8..8 as e4m3 bytes; w from {0, +-1, +-2, +-4, +-7}: the device-side scale max|w| / 448 is 2^-6, w / scale an
    e4m3 value, every product and sum an integer multiple of 2^-6 below 2^24 of them: the bf16 output is the integer."""
    dtype = torch.bfloat16
    ops, Lb, spec = _setup(l, dtype)
    o = X.operands(l, "fwd8")
    N, H, W = l.shape
    d = spec.desc(N, H, W, dtype)
    assert Lb.p2phd_conv_fp8_eligible(C.byref(d)) == 1
    Ho, Wo = spec.out_size(d)
    x8 = o["x"].to(torch.float8_e4m3fn).view(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
    packed = {}
    wp8 = _packed(ops, Lb, d, "fp8", o["w"].cuda(), packed)
    b = o["b"].cuda()
    for stats in (False, True):
        ws = X.guarded(Lb.p2phd_conv_fwd_workspace_bytes(C.byref(d)))
        gy, y = X.guarded_like((N, Ho, Wo, X.cpitch(l.cout)), dtype)
        bufs = {"y": gy, "workspace": ws, **packed}
        st = None
        if stats:
            bufs["stats"], st = X.guarded_like((N, X.cpitch(l.cout), 2), torch.float32)
        what = f"fwd_fp8 {l.name} stats={stats}"
        Lb.p2phd_launch_count(None, 1)
        ops.check(Lb.p2phd_conv_fwd_fp8(C.byref(d), ops.ptr(x8), _vp(wp8), ops.ptr(b), NONE, ops.ptr(y), ops.ptr(st), _vp(ws), ops.stream_ptr()), what)
        torch.cuda.synchronize()
        cnt = _count(Lb)
        X.check_guards(bufs, what)
        assert cnt["gconv"] == 1, cnt
        X.assert_bits_equal(y, o["want"], "nhwc", what)
        if stats:
            _check_stats(st, o["want"], what)


# ----------------------------------------------------------------------------------------------------------------------
# hand-over of the reflection extras between the InstanceNorm backward and the input gradient
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("geom", [(8, 32, 16, 508), (16, 4, 5, 512), (8, 20, 32, 512)], ids=lambda g: "x".join(map(str, g)))
def test_extras_written_by_the_instancenorm_backward_equal_the_builder(geom, dt):
    """p2phd_instnorm_act_bwd_rx reads back the dy it stored, adds the <= 4 values of an entry in fp32 and rounds once to the
    storage type (csrc/norm.hip).  The builder adds the same stored values in float64.  An fp32 sum of 4 terms is within
    3 u sum|t| of the exact sum S (u = 2^-24); rounding to a type with p significand bits adds at most half an ulp,
    <= 2^-p |value|.  Hence |extras - S| <= 2^-p (|S| + 3 u sum|t|) + 3 u sum|t|  (p = 8 bf16, 11 fp16, 24 fp32)."""
    dtype = DT[dt]
    ops = _ops()
    Lb = ops.lib_for(dtype)
    N, H, W, K = geom
    Cp = X.cpitch(K)
    gen = torch.Generator().manual_seed(H * W + K)
    g = torch.randn(N, H, W, Cp, generator=gen); g[..., K:] = 0
    y = torch.randn(N, H, W, Cp, generator=gen); y[..., K:] = 0
    mean = y.mean((1, 2))
    stats = torch.stack([mean, ((y - mean[:, None, None]) ** 2).sum((1, 2))], dim=-1).contiguous().cuda()
    EX = 2 * (W + 2) + 2 * H
    gb, buf = X.guarded_like((N * H * W * Cp + N * EX * Cp,), dtype)
    dy, rx = buf[:N * H * W * Cp], buf[N * H * W * Cp:]
    gd, y_d = g.to(dtype).cuda(), y.to(dtype).cuda()
    ops.check(Lb.p2phd_instnorm_act_bwd_rx(ops.dt_code(dtype), ops.ptr(gd), ops.ptr(y_d), ops.ptr(stats), ops.ptr(dy), None, 0, N, H, W, K, 1e-5, RELU,
                                           ops.ptr(rx), ops.stream_ptr()), "instnorm_act_bwd_rx")
    torch.cuda.synchronize()
    X.check_guards({"dy + extras": gb}, "instnorm_act_bwd_rx")
    dyh = dy.cpu().view(N, H, W, Cp)
    assert float(dyh.float().abs().max()) > 0 and float(dyh[..., K:].float().abs().max() if Cp > K else 0.0) == 0.0
    S = X.reflect_extras(dyh)
    A = X.reflect_extras(dyh.abs())
    p = {"bf16": 8, "f16": 11, "f32": 24}[dt]
    bound = 2.0 ** -p * (S.abs() + 3 * X.U32 * A) + 3 * X.U32 * A
    err = (rx.cpu().view(N, EX, Cp).double() - S).abs()
    assert bool((err <= bound).all()), (dt, geom, float((err - bound).max()), int((err > bound).sum()))


# ----------------------------------------------------------------------------------------------------------------------
# layout converters
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("geom", [(2, 3, 35, 16, 5), (1, 6, 7, 8, 2), (3, 8, 64, 8, 0), (2, 1, 129, 24, 17)],
                         ids=lambda g: "x".join(map(str, g)))
def test_layout_converters_move_integers_exactly(geom, dt):
    """p2phd_nchw_to_nhwc / p2phd_nhwc_to_nchw with a channel offset into a wider tensor, HW not a multiple of the vector
    width: the addressed channels carry the integers, every other channel keeps what it held."""
    dtype = DT[dt]
    ops = _ops()
    Lb = ops.lib_for(dtype)
    N, Cc, HW, Cp, off = geom
    gen = torch.Generator().manual_seed(HW)
    src = X.int_tensor((N, Cc, HW), -200, 200, 0.9, gen)
    gd, dst = X.guarded_like((N, HW, Cp), dtype, sentinel=0.0)
    base = X.int_tensor((N, HW, Cp), -7, 7, 1.0, gen).to(dtype)
    dst.copy_(base)
    sd = src.cuda()
    ops.check(Lb.p2phd_nchw_to_nhwc(ops.dt_code(dtype), ops.ptr(sd), ops.ptr(dst), N, Cc, HW, Cp, off, ops.stream_ptr()), "nchw_to_nhwc")
    torch.cuda.synchronize()
    X.check_guards({"dst": gd}, "nchw_to_nhwc")
    exp = base.clone().float()
    exp[..., off:off + Cc] = src.permute(0, 2, 1)
    X.assert_bits_equal(dst, exp, "flat", f"nchw_to_nhwc {geom} {dt}")
    gb, back = X.guarded_like((N, Cc, HW), torch.float32)
    ops.check(Lb.p2phd_nhwc_to_nchw(ops.dt_code(dtype), ops.ptr(dst), ops.ptr(back), N, Cc, HW, Cp, off, ops.stream_ptr()), "nhwc_to_nchw")
    torch.cuda.synchronize()
    X.check_guards({"dst": gb}, "nhwc_to_nchw")
    X.assert_bits_equal(back, src, "flat", f"nhwc_to_nchw {geom} {dt}")


@pytest.mark.parametrize("dt", HALF + ["f32"])
@pytest.mark.parametrize("chans,HW", [((2, 1), 35), ((3,), 64), ((1, 2, 1, 2), 129), ((4, 4, 3), 7), ((8, 8), 33)])
def test_cat_to_nhwc_moves_integers_exactly_and_zeroes_the_pad_channels(chans, HW, dt):
    dtype = DT[dt]
    ops = _ops()
    Lb = ops.lib_for(dtype)
    N = 2
    gen = torch.Generator().manual_seed(HW + len(chans))
    srcs = [X.int_tensor((N, c, HW), -200, 200, 0.9, gen) for c in chans]
    Cp = X.cpitch(sum(chans))
    gd, dst = X.guarded_like((N, HW, Cp), dtype)
    dev = [s.cuda() for s in srcs]
    ptrs = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
    cc = (C.c_int32 * len(dev))(*chans)
    ops.check(Lb.p2phd_nchw_cat_to_nhwc(ops.dt_code(dtype), ptrs, cc, len(dev), ops.ptr(dst), N, HW, Cp, ops.stream_ptr()), "nchw_cat_to_nhwc")
    torch.cuda.synchronize()
    X.check_guards({"dst": gd}, "nchw_cat_to_nhwc")
    X.assert_bits_equal(dst.view(N, HW, 1, Cp), torch.cat(srcs, 1).view(N, sum(chans), HW, 1), "nhwc", f"cat {chans} {HW} {dt}")
