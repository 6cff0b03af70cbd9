"""Per-element tests of the kernels around the convs (csrc/norm.hip, csrc/loss.hip), straight through the C ABI: InstanceNorm +
activation forward / backward in all four dispatch forms, the e4m3 twin, the activation backward with and without the bias
gradient, AvgPool, the losses, the three Adam entry points, the device GradScaler and p2phd_zero_segments.

Every output and scratch buffer sits between canaries and is prefilled with a non-integer sentinel, inputs come from a seeded CPU
generator, and every element is compared with the float64 reference of tests/_companions.py under the bound derived there (or bit
for bit where the operation is a single rounding).  tests/test_companions_host.py shows on the CPU that those bounds hold for a
float32 emulation of the kernels and reject the listed mutants, and pins which backward form each InstanceNorm case takes.

The launches that shrink their grid to fit the library's reduction scratch (`rows_max` of the InstanceNorm backward's reduce pass
and of p2phd_act_bwd_db) have cases of their own, K.IN_CLAMP_CASES and K.ACT_DB_CLAMP_CASES: each asks p2phd_reduction_rows
(pinned on the host by tests/test_reduction_rows.py) and asserts that it IS clamped before it launches.  The same clamp of the
column sum (csrc/convaux.hip, launch_colsum) is NOT tested: it engages from about 134 M elements (Cp = 4096 on more than 32 k
pixels), out of reach of a test of seconds.

Every case here stays under the workgroup caps of the grid-stride loops or just beyond them; the loops' later trips -- AvgPool's
(8192 workgroups = 2 M pieces), act_bwd's, the losses' and the Adam entries' with the scaler's scan -- are the subject of
tests/test_gpu_long.py, at 2.5 trips, with the grids pinned by tests/test_long_host.py.  Left out on purpose: the statistics
merges (reached through the conv epilogue, covered by tests/test_gpu_conv_exact.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _companions as K
from _companions import NONE, LRELU, TANH, RELU, DT

pytestmark = pytest.mark.gpu

DTS = ["bf16", "f16", "f32"]
HALF = ["bf16", "f16"]
EINVAL = -1
F32 = torch.float32


def _ops():
    from pix2pixhdaudiosr_amd import _ops
    return _ops


def _setup(dt):
    ops = _ops()
    return ops, ops.lib_for(DT[dt]), (0 if dt == "f32" else 1), (4 if dt == "f32" else 8)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f"{what}: {int(_bits(a).ne(_bits(b)).sum())} elements differ in their bits"


def _sentinel_left(t, what):
    ref = torch.full((1,), K.SENTINEL, dtype=t.dtype)
    assert bool((_bits(t) == _bits(ref)).all()), f"{what}: written"


def _done(bufs, what):
    torch.cuda.synchronize()
    K.check_guards(bufs, what)


# ----------------------------------------------------------------------------------------------------------------------
# InstanceNorm + activation
# ----------------------------------------------------------------------------------------------------------------------
def _in_dev(case, dt):
    d = K.in_data(case, dt)
    return d, {k: v.cuda() for k, v in d.items()}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.IN_CASES, ids=K.IN_IDS)
def test_instnorm_forward(case, dt):
    ops, Lb, code, _ = _setup(dt)
    N, HW, Cc = case[:3]
    d, g = _in_dev(case, dt)
    go, out = K.guarded_like(d["y"].shape, DT[dt], sentinel=K.SENTINEL)
    for act in (NONE, RELU, LRELU):
        for residual in (False, True):
            what = f"instnorm_act_fwd {case[:3]} {dt} act {act} residual {residual}"
            out.fill_(K.SENTINEL)
            ops.check(Lb.p2phd_instnorm_act_fwd(code, ops.ptr(g["y"]), ops.ptr(g["stats"]), ops.ptr(g["res"] if residual else None), ops.ptr(out),
                                                N, HW, Cc, K.EPS, act, ops.stream_ptr()), what)
            _done({"out": go}, what)
            want, b32 = K.instnorm_fwd_reference(d["y"], d["stats"], d["res"] if residual else None, HW, Cc, K.EPS, act)
            K.assert_within(out, want, K.stored_bound(want, b32, DT[dt]), what, Cc)


@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("case", K.IN_CASES, ids=K.IN_IDS)
def test_instnorm_forward_e4m3_twin(case, dt):
    """out has the bits of the plain entry; every byte of out8 is the e4m3 code of the fp32 value within its bound.  Two pixels of
    the constant channel (rstd = 1 / sqrt(eps) = 316) are moved by +-2: f = +-632 pins the saturation at +-448."""
    ops, Lb, code, _ = _setup(dt)
    N, HW, Cc = case[:3]
    d = dict(K.in_data(case, dt))
    if HW >= 3:
        y = d["y"].clone()
        y[:, 1, K.CH_CONST], y[:, 2, K.CH_CONST] = K.CONST + 2.0, K.CONST - 2.0
        d["y"] = y
    g = {k: v.cuda() for k, v in d.items()}
    go, out = K.guarded_like(d["y"].shape, DT[dt], sentinel=K.SENTINEL)
    gp, plain = K.guarded_like(d["y"].shape, DT[dt], sentinel=K.SENTINEL)
    g8 = K.Guarded(d["y"].numel(), "cuda", 0x7F)                        # 0x7F: NaN in e4m3fn -- a byte that is not written fails
    out8 = g8.view(torch.uint8, tuple(d["y"].shape))
    for act, residual in ((NONE, False), (RELU, True), (LRELU, False)):
        what = f"instnorm_act_fwd_q8 {case[:3]} {dt} act {act} residual {residual}"
        out.fill_(K.SENTINEL); plain.fill_(K.SENTINEL); out8.fill_(0x7F)
        r = ops.ptr(g["res"] if residual else None)
        ops.check(Lb.p2phd_instnorm_act_fwd_q8(code, ops.ptr(g["y"]), ops.ptr(g["stats"]), r, ops.ptr(out), C.c_void_p(g8.ptr()), N, HW, Cc,
                                               K.EPS, act, ops.stream_ptr()), what)
        ops.check(Lb.p2phd_instnorm_act_fwd(code, ops.ptr(g["y"]), ops.ptr(g["stats"]), r, ops.ptr(plain), N, HW, Cc, K.EPS, act,
                                            ops.stream_ptr()), what)
        _done({"out": go, "out8": g8, "plain": gp}, what)
        want, b32 = K.instnorm_fwd_reference(d["y"], d["stats"], d["res"] if residual else None, HW, Cc, K.EPS, act)
        if HW >= 3 and act == NONE:
            assert float(want.max()) > 448 and float(want.min()) < -448
        _same_bits(out, plain, what + " out against the plain entry")
        K.assert_within(out, want, K.stored_bound(want, b32, DT[dt]), what, Cc)
        K.assert_q8_neighbours(out8, want, b32, what + " out8", Cc)


def test_instnorm_forward_e4m3_twin_is_refused_for_f32():
    ops, Lb, code, _ = _setup("f32")
    case = K.IN_CASES[7]
    d, g = _in_dev(case, "f32")
    go, out = K.guarded_like(d["y"].shape, F32, sentinel=K.SENTINEL)
    g8 = K.Guarded(d["y"].numel(), "cuda", 0x7F)
    rc = Lb.p2phd_instnorm_act_fwd_q8(code, ops.ptr(g["y"]), ops.ptr(g["stats"]), None, ops.ptr(out), C.c_void_p(g8.ptr()), case[0], case[1],
                                      case[2], K.EPS, NONE, ops.stream_ptr())
    assert rc == EINVAL
    _done({"out": go, "out8": g8}, "q8 f32")
    _sentinel_left(out, "out of a refused call")


def _run_bwd(Lb, ops, code, entry, g, shape, dtype, N, HW, Cc, act, prefill, bstats_in=None):
    """One backward call into fresh guarded buffers; returns (dy, bstats, db, guards, rc)."""
    Cp = shape[2]
    gdy, dy = K.guarded_like(shape, dtype, sentinel=K.SENTINEL)
    gbs, bst = K.guarded_like((N, Cp, 2), F32, sentinel=K.SENTINEL)
    gdb, db = K.guarded_like((Cc,), F32, sentinel=K.SENTINEL)
    if prefill is not None:
        db.copy_(prefill)
    a = (code, ops.ptr(g["g"]), ops.ptr(g["y"]), ops.ptr(g["stats"]))
    if entry == "apply":
        bst.copy_(bstats_in)
        rc = Lb.p2phd_instnorm_act_bwd_apply(*a, ops.ptr(bst), ops.ptr(dy), ops.ptr(db), 0 if prefill is None else 1, N, HW, Cc, K.EPS, act,
                                             ops.stream_ptr())
    else:
        fn = Lb.p2phd_instnorm_act_bwd_acc if entry == "acc" else Lb.p2phd_instnorm_act_bwd
        rc = fn(*a, ops.ptr(bst), ops.ptr(dy), ops.ptr(db), N, HW, Cc, K.EPS, act, ops.stream_ptr())
    guards = {"dy": gdy, "bstats": gbs, "db": gdb}
    _done(guards, f"instnorm backward {entry}")
    return dy, bst, db, guards, rc


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.IN_CASES, ids=K.IN_IDS)
def test_instnorm_backward(case, dt):
    """p2phd_instnorm_act_bwd and _acc: dy per element, the two sums of the two-pass form (the single launch leaves bstats alone:
    with the query pinned on the host this shows which form ran), db against the column sums of the stored dy, and dy / bstats bit
    for bit on a second run (fixed-order sums; db is a float-atomic sum of rounding noise and exempt)."""
    ops, Lb, code, _ = _setup(dt)
    N, HW, Cc, two_pass = case[:4]
    assert Lb.p2phd_instnorm_act_bwd_two_pass(code, N, HW, Cc) == two_pass
    d, g = _in_dev(case, dt)
    gen = torch.Generator().manual_seed(77)
    for entry, act in (("bwd", RELU), ("bwd", NONE), ("acc", LRELU)):
        what = f"instnorm_act_bwd[{entry}] {case[:3]} {dt} act {act}"
        prefill = torch.randn(Cc, generator=gen) if entry == "acc" else None
        dy, bst, db, _, rc = _run_bwd(Lb, ops, code, entry, g, d["y"].shape, DT[dt], N, HW, Cc, act, prefill)
        ops.check(rc, what)
        ref = K.instnorm_bwd_reference(d["g"], d["y"], d["stats"], HW, Cc, K.EPS, act)
        K.assert_within(dy, ref["dy"], K.stored_bound(ref["dy"], ref["b32"], DT[dt]), what + " dy", Cc)
        if two_pass:
            K.bstats_check(bst, ref, Cc, what + " bstats")
        else:
            _sentinel_left(bst, what + " bstats of the single-launch form")
        K.colsum_check(dy, db, Cc, what + " db", prefill)
        dy2, bst2, _, _, rc = _run_bwd(Lb, ops, code, entry, g, d["y"].shape, DT[dt], N, HW, Cc, act, prefill)
        ops.check(rc, what)
        _same_bits(dy2, dy, what + " dy, second run")
        _same_bits(bst2, bst, what + " bstats, second run")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.IN_CASES, ids=K.IN_IDS)
def test_instnorm_backward_apply_alone(case, dt):
    """p2phd_instnorm_act_bwd_apply fed the reference sums rounded to fp32 (one rounding: inside the sums' own bound): dy within the
    same bound; on a plane that takes the single launch it is refused."""
    ops, Lb, code, _ = _setup(dt)
    N, HW, Cc, two_pass = case[:4]
    d, g = _in_dev(case, dt)
    what = f"instnorm_act_bwd_apply {case[:3]} {dt}"
    ref = K.instnorm_bwd_reference(d["g"], d["y"], d["stats"], HW, Cc, K.EPS, LRELU)
    sums = torch.stack([ref["s1"], ref["s2"]], -1).float().cuda()
    dy, bst, db, _, rc = _run_bwd(Lb, ops, code, "apply", g, d["y"].shape, DT[dt], N, HW, Cc, LRELU, None, sums)
    if not two_pass:
        assert rc == EINVAL
        _sentinel_left(dy, what + " dy of a refused call")
        return
    ops.check(rc, what)
    _same_bits(bst, sums, what + " bstats is an input")
    K.assert_within(dy, ref["dy"], K.stored_bound(ref["dy"], ref["b32"], DT[dt]), what + " dy", Cc)
    K.colsum_check(dy, db, Cc, what + " db")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.IN_CLAMP_CASES, ids=K.IN_CLAMP_IDS)
def test_instnorm_backward_with_the_reduce_grid_clamped_to_the_scratch(case, dt):
    """The two-pass form where the reduce pass runs on FEWER workgroups per sample than the apply pass, because one partial row
    per workgroup has to fit the reduction scratch (the configs[4] trunk at its benchmarked batch runs here).  p2phd_reduction_rows
    proves the clamp before anything is launched.  Then as test_instnorm_backward: `bwd` and `acc` with two activations, dy per
    element, both sums, db, guard bands, dy and bstats bit for bit on a second run; and the apply pass alone (it keeps the
    unclamped grid) fed the reference sums, as test_instnorm_backward_apply_alone.  The float64 reference of each activation is
    built once and serves the entries that use it."""
    ops, Lb, code, epp = _setup(dt)
    N, HW, Cc = case[:3]
    assert Lb.p2phd_instnorm_act_bwd_two_pass(code, N, HW, Cc) == 1
    wanted, used = K.clamped_rows(Lb, "instnorm_bwd", code, N, HW, Cc, epp)
    print(f"instnorm_bwd {case[:3]} {dt}: rows wanted {wanted}, used {used}")
    d, g = _in_dev(case, dt)
    gen = torch.Generator().manual_seed(77)
    ref = None
    for entry, act in (("bwd", RELU), ("acc", LRELU)):
        what = f"instnorm_act_bwd[{entry}] {case[:3]} {dt} act {act}, reduce grid {used} of {wanted}"
        prefill = torch.randn(Cc, generator=gen) if entry == "acc" else None
        dy, bst, db, _, rc = _run_bwd(Lb, ops, code, entry, g, d["y"].shape, DT[dt], N, HW, Cc, act, prefill)
        ops.check(rc, what)
        ref = K.instnorm_bwd_reference(d["g"], d["y"], d["stats"], HW, Cc, K.EPS, act)
        bound = K.stored_bound(ref["dy"], ref["b32"], DT[dt])
        K.bstats_check(bst, ref, Cc, what + " bstats")
        K.assert_within(dy, ref["dy"], bound, what + " dy", Cc)
        K.colsum_check(dy, db, Cc, what + " db", prefill)
        dy2, bst2, _, _, rc = _run_bwd(Lb, ops, code, entry, g, d["y"].shape, DT[dt], N, HW, Cc, act, prefill)
        ops.check(rc, what)
        _same_bits(dy2, dy, what + " dy, second run")
        _same_bits(bst2, bst, what + " bstats, second run")
        del dy, dy2
    what = f"instnorm_act_bwd_apply {case[:3]} {dt}, grid {wanted}"              # (ref, bound: those of LRELU)
    sums = torch.stack([ref["s1"], ref["s2"]], -1).float().cuda()
    dy, bst, db, _, rc = _run_bwd(Lb, ops, code, "apply", g, d["y"].shape, DT[dt], N, HW, Cc, LRELU, None, sums)
    ops.check(rc, what)
    _same_bits(bst, sums, what + " bstats is an input")
    K.assert_within(dy, ref["dy"], bound, what + " dy", Cc)
    K.colsum_check(dy, db, Cc, what + " db")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", [c for c in K.IN_CASES if not c[3]], ids=[i for i, c in zip(K.IN_IDS, K.IN_CASES) if not c[3]])
def test_instnorm_backward_single_launch_in_both_workgroup_orders(case, dt):
    ops, Lb, code, _ = _setup(dt)
    N, HW, Cc = case[:3]
    d, g = _in_dev(case, dt)
    ref = K.instnorm_bwd_reference(d["g"], d["y"], d["stats"], HW, Cc, K.EPS, RELU)
    got = {}
    try:
        for order in (0, 1):
            what = f"instnorm_act_bwd {case[:3]} {dt} wgrad_xcd {order}"
            ops.check(Lb.p2phd_set_option(b"wgrad_xcd", order), what)
            dy, _, db, _, rc = _run_bwd(Lb, ops, code, "bwd", g, d["y"].shape, DT[dt], N, HW, Cc, RELU, None)
            ops.check(rc, what)
            K.assert_within(dy, ref["dy"], K.stored_bound(ref["dy"], ref["b32"], DT[dt]), what + " dy", Cc)
            K.colsum_check(dy, db, Cc, what + " db")
            got[order] = dy
    finally:
        ops.check(Lb.p2phd_set_option(b"wgrad_xcd", 1), "restore wgrad_xcd")
    _same_bits(got[0], got[1], f"{case[:3]} {dt}: dy under the two workgroup orders")


# ----------------------------------------------------------------------------------------------------------------------
# activation backward
# ----------------------------------------------------------------------------------------------------------------------
def _act_operands(shape, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.tanh(torch.randn(shape, generator=gen))
    a[torch.rand(shape, generator=gen) < 0.05] = 0.0                    # o == 0 takes the slope branch
    return torch.randn(shape, generator=gen).to(dtype), a.to(dtype)


def _check_act(dx, g, a, act, dtype, what):
    want, bound = K.act_bwd_reference(g, a, act, dtype)
    if bound is None:
        K.assert_bits_equal(dx, want, "flat", what)
    else:
        K.assert_within(dx, want, bound, what)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pieces", [1, 255, 8192 * 256 + 5])
def test_act_bwd(pieces, dt):
    """One piece, less than a workgroup, and five pieces more than the grid cap of 8192 workgroups holds (the grid-stride loop)."""
    ops, Lb, code, epp = _setup(dt)
    n = pieces * epp
    g, a = _act_operands((n,), DT[dt], pieces)
    gd, ad = g.cuda(), a.cuda()
    gdx, dx = K.guarded_like((n,), DT[dt], sentinel=K.SENTINEL)
    for act in (NONE, LRELU, TANH, RELU):
        what = f"act_bwd {pieces} pieces {dt} act {act}"
        dx.fill_(K.SENTINEL)
        ops.check(Lb.p2phd_act_bwd(code, ops.ptr(gd), ops.ptr(ad), ops.ptr(dx), n, act, ops.stream_ptr()), what)
        _done({"dx": gdx}, what)
        _check_act(dx, g, a, act, DT[dt], what)
    dx.fill_(K.SENTINEL)
    assert Lb.p2phd_act_bwd(code, ops.ptr(gd), ops.ptr(ad), ops.ptr(dx), n + 1, RELU, ops.stream_ptr()) == EINVAL
    _done({"dx": gdx}, "act_bwd refused")
    _sentinel_left(dx, "dx of a refused call")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geom", K.ACT_DB_CASES + K.ACT_DB_CLAMP_CASES, ids=lambda g: "x".join(map(str, g)))
def test_act_bwd_db(geom, dt):
    """The K.ACT_DB_CLAMP_CASES run with the grid clamped to the reduction scratch (asserted through p2phd_reduction_rows before
    the first launch), the others on the grid the plane asks for."""
    ops, Lb, code, epp = _setup(dt)
    P, Cc = geom
    Cp = K.cpitch(Cc)
    if geom in K.ACT_DB_CLAMP_CASES:
        wanted, used = K.clamped_rows(Lb, "act_bwd_db", code, 1, P, Cc, epp)
        print(f"act_bwd_db {geom} {dt}: rows wanted {wanted}, used {used}")
    else:
        rc, wanted, used = K.reduction_rows(Lb, "act_bwd_db", code, 1, P, Cc)
        assert rc == 0 and used == wanted
    g, a = _act_operands((1, P, Cc), F32, P + Cc)
    g, a = K.physical(g, DT[dt]), K.physical(a, DT[dt])
    gd, ad = g.cuda(), a.cuda()
    prefill = torch.randn(Cc, generator=torch.Generator().manual_seed(P))
    for act in (TANH, LRELU, RELU):
        for acc in (0, 1):
            what = f"act_bwd_db {geom} {dt} act {act} accumulate {acc}"
            runs = []
            for _ in range(2):
                gdx, dx = K.guarded_like((1, P, Cp), DT[dt], sentinel=K.SENTINEL)
                gdb, db = K.guarded_like((Cc,), F32, sentinel=K.SENTINEL)
                if acc:
                    db.copy_(prefill)
                ops.check(Lb.p2phd_act_bwd_db(code, ops.ptr(gd), ops.ptr(ad), ops.ptr(dx), P, Cc, act, ops.ptr(db), acc, ops.stream_ptr()), what)
                _done({"dx": gdx, "db": gdb}, what)
                runs.append((dx, db))
            dx, db = runs[0]
            _check_act(dx, g, a, act, DT[dt], what + " dx")
            assert float(dx[..., Cc:].abs().max() if Cp > Cc else 0.0) == 0
            K.colsum_check(dx, db, Cc, what + " db", prefill if acc else None)
            _same_bits(runs[1][0], dx, what + " dx, second run")
            _same_bits(runs[1][1], db, what + " db, second run")
    for acc in (0, 1):                                                  # P = 0: db cleared, or left in accumulate mode
        gdb, db = K.guarded_like((Cc,), F32, sentinel=K.SENTINEL)
        ops.check(Lb.p2phd_act_bwd_db(code, None, None, None, 0, Cc, RELU, ops.ptr(db), acc, ops.stream_ptr()), "act_bwd_db P = 0")
        _done({"db": gdb}, "act_bwd_db P = 0")
        if acc:
            _sentinel_left(db, "db of an accumulating call without pixels")
        else:
            assert bool((_bits(db) == 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# AvgPool
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("geom", K.POOL_CASES, ids=lambda g: "x".join(map(str, g)))
def test_avgpool(geom, dt):
    ops, Lb, code, _ = _setup(dt)
    N, Cc, H, W = geom
    Ho, Wo, Cp = K.pool_out(H), K.pool_out(W), K.cpitch(Cc)
    gen = torch.Generator().manual_seed(H * 100 + W)
    x = K.physical(torch.randn(N, H * W, Cc, generator=gen), DT[dt]).reshape(N, H, W, Cp)
    cot = K.physical(torch.randn(N, Ho * Wo, Cc, generator=gen), DT[dt]).reshape(N, Ho, Wo, Cp)
    gy, y = K.guarded_like((N, Ho * Wo, Cp), DT[dt], sentinel=K.SENTINEL)
    gdx, dx = K.guarded_like((N, H * W, Cp), DT[dt], sentinel=K.SENTINEL)
    what = f"avgpool {geom} {dt}"
    ops.check(Lb.p2phd_avgpool3s2_fwd(code, ops.ptr(x.cuda()), ops.ptr(y), N, H, W, Cc, ops.stream_ptr()), what)
    ops.check(Lb.p2phd_avgpool3s2_bwd(code, ops.ptr(cot.cuda()), ops.ptr(dx), N, H, W, Cc, ops.stream_ptr()), what)
    _done({"y": gy, "dx": gdx}, what)
    want, b32 = K.avgpool_fwd_reference(x)
    K.assert_within(y, want, K.stored_bound(want, b32, DT[dt]), what + " forward", Cc)
    want, b32 = K.avgpool_bwd_reference(cot, H, W)
    K.assert_within(dx, want, K.stored_bound(want, b32, DT[dt]), what + " backward", Cc)


# ----------------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("geom", K.LOSS_CASES, ids=lambda g: "x".join(map(str, g)))
def test_losses(geom, kind, dt):
    ops, Lb, code, _ = _setup(dt)
    P, Cc = geom
    target, coeff, gup = 1.0, 2.5, 1.75
    a, b = K.loss_data(P, Cc, dt, kind)
    ad, bd = a.cuda(), (b.cuda() if kind == 1 else None)
    what = f"loss kind {kind} {geom} {dt}"
    want, bound = K.loss_fwd_reference(kind, a, b, target, Cc, coeff, K.OUT0)
    outs = []
    for _ in range(2):
        go, out = K.guarded_like((1,), F32, sentinel=K.OUT0)
        ops.check(Lb.p2phd_loss_fwd(kind, code, ops.ptr(ad), ops.ptr(bd), target, P, Cc, coeff, ops.ptr(out), ops.stream_ptr()), what)
        _done({"out": go}, what)
        outs.append(out)
    got = float(outs[0].cpu().double())
    assert abs(got - want) <= bound, (what, got, want, bound)
    _same_bits(outs[1], outs[0], what + " second run")
    gup_d = torch.tensor([gup], dtype=F32, device="cuda")
    gda, da = K.guarded_like(tuple(a.shape), DT[dt], sentinel=K.SENTINEL)
    ops.check(Lb.p2phd_loss_bwd(kind, code, ops.ptr(ad), ops.ptr(bd), target, P, Cc, coeff, ops.ptr(gup_d), ops.ptr(da), ops.stream_ptr()), what)
    _done({"da": gda}, what)
    if kind == 1:
        assert int((a[:, :Cc] == b[:, :Cc]).sum()) >= P * Cc // 20
    K.assert_bits_equal(da, K.loss_bwd_reference(kind, a, b, target, Cc, coeff, gup, DT[dt]), "flat", what + " backward")
    # P = 0: out untouched
    go, out = K.guarded_like((1,), F32, sentinel=K.OUT0)
    ops.check(Lb.p2phd_loss_fwd(kind, code, ops.ptr(ad), ops.ptr(bd), target, 0, Cc, coeff, ops.ptr(out), ops.stream_ptr()), what)
    _done({"out": go}, what)
    assert float(out.cpu()) == K.OUT0


# ----------------------------------------------------------------------------------------------------------------------
# Adam, GradScaler, zero_segments
# ----------------------------------------------------------------------------------------------------------------------
LR, B1, B2, AEPS, GSCALE = 3e-4, 0.5, 0.999, 1e-8, 0.25


def _adam_bufs(state):
    bufs, tens = {}, []
    for name, t in zip(("p", "g", "m", "v"), state):
        bufs[name], d = K.guarded_like(tuple(t.shape), F32, sentinel=K.SENTINEL)
        d.copy_(t)
        tens.append(d)
    return bufs, tens


def _check_adam(tens, state, t, gscale, what):
    p, g, m, v = state
    want, bounds = K.adam_reference(p, g, m, v, LR, B1, B2, AEPS, t, gscale)
    for name, got, w, b in zip("pmv", (tens[0], tens[2], tens[3]), want, bounds):
        K.assert_within(got, w, b, f"{what} {name}")
    _same_bits(tens[1], g, what + " gradient is an input")


@pytest.mark.parametrize("entry", ["step", "step_dev"])
@pytest.mark.parametrize("n", K.ADAM_SIZES)
def test_adam(n, entry):
    """One step from a random state at step counts 1 and 1000; the largest size takes a second trip of the grid-stride loop
    (4096 workgroups x 256 threads x 4 elements) and ends in the scalar tail."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(F32)
    for t in (1, 1000):
        what = f"adam_{entry} n {n} t {t}"
        state = K.adam_state(n, n + t)
        bufs, (p, g, m, v) = _adam_bufs(state)
        if entry == "step":
            ops.check(Lb.p2phd_adam_step(ops.ptr(p), ops.ptr(g), ops.ptr(m), ops.ptr(v), n, LR, B1, B2, AEPS, t, GSCALE, ops.stream_ptr()), what)
        else:
            bufs["lr"], lr_dev = K.guarded_like((1,), F32, sentinel=LR)                 # read from the device: no lr argument
            bufs["step"], step_dev = K.guarded_like((1,), torch.int64, sentinel=t - 1)
            ops.check(Lb.p2phd_adam_step_dev(ops.ptr(p), ops.ptr(g), ops.ptr(m), ops.ptr(v), n, ops.ptr(lr_dev), ops.ptr(step_dev), B1, B2, AEPS,
                                             GSCALE, ops.stream_ptr()), what)
        _done(bufs, what)
        _check_adam((p, g, m, v), state, t, GSCALE, what)
        if entry == "step_dev":
            assert int(step_dev.item()) == t and float(lr_dev.item()) == float(np.float32(LR))


SCALE = 1024.0


def _scaled_call(Lb, ops, tens, n, t0, scaler, found_index):
    p, g, m, v = tens
    lr_dev = torch.tensor([LR], dtype=F32, device="cuda")
    step_dev = torch.tensor([t0], dtype=torch.int64, device="cuda")
    ops.check(Lb.p2phd_adam_step_scaled(ops.ptr(p), ops.ptr(g), ops.ptr(m), ops.ptr(v), n, ops.ptr(lr_dev), ops.ptr(step_dev), B1, B2, AEPS,
                                        GSCALE, ops.ptr(scaler), found_index, ops.stream_ptr()), "adam_step_scaled")
    return step_dev


@pytest.mark.parametrize("n", [1003, K.ADAM_SIZES[-1]])
def test_scaled_adam_with_clean_gradients_unscales_by_the_state(n):
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(F32)
    p, g, m, v = K.adam_state(n, n)
    state = (p, g * SCALE, m, v)                                        # the gradients arrive multiplied by the scale (exact)
    for fi in (0, 1):
        bufs, tens = _adam_bufs(state)
        bufs["scaler"], scaler = K.guarded_like((5,), F32, sentinel=0.0)
        scaler.copy_(torch.tensor([SCALE, 1.0 / SCALE, 3.0, 0.0, 0.0]))
        step_dev = _scaled_call(Lb, ops, tens, n, 6, scaler, fi)
        _done(bufs, "adam_step_scaled clean")
        _check_adam(tens, state, 7, GSCALE / SCALE, f"adam_step_scaled clean n {n} found_index {fi}")
        assert int(step_dev.item()) == 7
        assert scaler.cpu().tolist() == [SCALE, 1.0 / SCALE, 3.0, 0.0, 0.0]


@pytest.mark.parametrize("n,pos", [(1003, 0), (1003, 498), (1003, 1002), (K.ADAM_SIZES[-1], K.ADAM_SIZES[-1] - 1)])
def test_scaled_adam_skips_the_step_on_a_non_finite_gradient(n, pos):
    """inf or NaN at index 0, inside the four-wide region, at n - 1 with n % 4 = 3 (the scalar tail of the scan), and at n - 1 of the
    size that takes the scan's grid-stride trip: p, m, v keep their bits, the step count does not move, only the flag of
    found_index is set."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(F32)
    assert n % 4 == 3
    p, g, m, v = K.adam_state(n, n)
    for fi, bad in ((0, float("inf")), (1, float("nan")), (1, float("-inf"))):
        g = g.clone()
        g[pos] = bad
        state = (p, g, m, v)
        bufs, tens = _adam_bufs(state)
        bufs["scaler"], scaler = K.guarded_like((5,), F32, sentinel=0.0)
        scaler.copy_(torch.tensor([SCALE, 1.0 / SCALE, 3.0, 0.0, 0.0]))
        step_dev = _scaled_call(Lb, ops, tens, n, 6, scaler, fi)
        _done(bufs, "adam_step_scaled dirty")
        for name, got, w in zip("pgmv", tens, state):
            _same_bits(got, w, f"adam_step_scaled n {n} {bad} at {pos}: {name}")
        assert int(step_dev.item()) == 6
        want = [SCALE, 1.0 / SCALE, 3.0, 0.0, 0.0]
        want[3 + fi] = 1.0
        assert scaler.cpu().tolist() == want


def test_scaler_update_transitions():
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(F32)
    for state, growth, backoff, interval in K.SCALER_TABLE:
        gs, dev = K.guarded_like((5,), F32, sentinel=0.0)
        dev.copy_(torch.tensor(state, dtype=F32))
        ops.check(Lb.p2phd_scaler_update(ops.ptr(dev), growth, backoff, interval, ops.stream_ptr()), "scaler_update")
        _done({"state": gs}, "scaler_update")
        want = torch.from_numpy(np.array(K.scaler_update_reference(state, growth, backoff, interval), dtype=np.float32))
        _same_bits(dev, want, f"scaler_update {state} interval {interval}")


def test_zero_segments():
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(F32)
    total = 8000
    segs = [(10, 1), (11, 256), (300, 0), (400, 257), (total - 5000, 5000)]     # (10, 1) and (11, 256) touch; the last ends the buffer
    gb, base = K.guarded_like((total,), F32, sentinel=K.SENTINEL)
    seg_dev = torch.tensor(segs, dtype=torch.int64).cuda()
    ops.check(Lb.p2phd_zero_segments(ops.ptr(base), ops.ptr(seg_dev), 0, ops.stream_ptr()), "zero_segments n = 0")
    _done({"base": gb}, "zero_segments n = 0")
    _sentinel_left(base, "n = 0")
    ops.check(Lb.p2phd_zero_segments(ops.ptr(base), ops.ptr(seg_dev), len(segs), ops.stream_ptr()), "zero_segments")
    _done({"base": gb}, "zero_segments")
    want = torch.full((total,), K.SENTINEL, dtype=F32)
    for off, ln in segs:
        want[off:off + ln] = 0.0
    _same_bits(base, want, "zero_segments")
