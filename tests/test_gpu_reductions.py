"""The shared state of the fixed-order reductions ("last workgroup folds", csrc/common.h, csrc/core.hip): one family of kernels
keeps its partial rows and arrival tickets in a region of a library-owned scratch ACROSS launches.  tests/test_gpu_companions.py
checks each kernel's values, one geometry at a time; here a family runs through changing geometry and on two streams.

* Re-arming: the workgroup that draws the last ticket stores 0, so a launch of one workgroup count must leave the family usable
  by the next launch of another count.  A, B, C, A, B on one stream after ONE p2phd_reduction_reset: A many workgroups (for the two
  families that clamp their grid to the scratch, a clamped case), B exactly one workgroup per sample, C a mid-size case (for the
  InstanceNorm, with another number of samples: other tickets are in use).  Runs 1 to 3 are checked against the float64 references
  as in tests/test_gpu_companions.py, runs 4 and 5 must repeat runs 1 and 2 bit for bit.
* Two streams: fold_scratch() orders two launches of one family that arrive on different streams by an event.

The clamp of the column sum (csrc/convaux.hip, launch_colsum) is not reached by any case here: it needs about 134 M elements."""
import pytest
import torch

import _companions as K
import _exact as X
import test_gpu_companions as G
import test_gpu_conv_exact as CE
from _companions import LRELU, RELU, DT

pytestmark = pytest.mark.gpu

F32 = torch.float32
IN_A, IN_B, IN_C = K.IN_CLAMP_CASES[0], K.IN_CASES[8], K.IN_CASES[9]          # (1, 2400, 4096), (1, 1, 3), (3, 1320, 24)
DB_A, DB_B, DB_C = K.ACT_DB_CLAMP_CASES[0], K.ACT_DB_CASES[0], K.ACT_DB_CASES[3]   # (1100, 4096), (1, 3), (700, 67)
LOSS_A, LOSS_B, LOSS_C = K.LOSS_CASES[3], K.LOSS_CASES[0], K.LOSS_CASES[1]    # (30000, 67), (40, 3), (700, 67)


def _reset(ops, Lb):
    ops.check(Lb.p2phd_reduction_reset(ops.stream_ptr()), "reduction_reset")


# ----------------------------------------------------------------------------------------------------------------------
# one family, changing geometry, no reset in between
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", G.DTS)
def test_instnorm_backward_rearms_across_geometries(dt):
    """db is left out of the bit comparison (and checked against its column sums in all five runs): the apply pass adds it with
    float atomics on purpose (csrc/norm.hip, in_act_bwd_apply_kernel), it is no output of the fixed-order reduction."""
    ops, Lb, code, epp = G._setup(dt)
    assert IN_A[:3] == (1, 2400, 4096) and IN_B[:3] == (1, 1, 3) and IN_C[0] != IN_A[0]
    K.clamped_rows(Lb, "instnorm_bwd", code, *IN_A[:3], epp)
    assert K.reduction_rows(Lb, "instnorm_bwd", code, *IN_B[:3]) == (0, 1, 1)
    _reset(ops, Lb)
    got = []
    for i, case in enumerate((IN_A, IN_B, IN_C, IN_A, IN_B)):
        N, HW, Cc = case[:3]
        what = f"run {i + 1} of A B C A B: instnorm_act_bwd {case[:3]} {dt}"
        d, g = G._in_dev(case, dt)
        dy, bst, db, _, rc = G._run_bwd(Lb, ops, code, "bwd", g, d["y"].shape, DT[dt], N, HW, Cc, RELU, None)
        ops.check(rc, what)
        K.colsum_check(dy, db, Cc, what + " db")
        if i < 3:
            ref = K.instnorm_bwd_reference(d["g"], d["y"], d["stats"], HW, Cc, K.EPS, RELU)
            K.bstats_check(bst, ref, Cc, what + " bstats")
            K.assert_within(dy, ref["dy"], K.stored_bound(ref["dy"], ref["b32"], DT[dt]), what + " dy", Cc)
            del ref
            got.append((dy, bst))
        else:
            G._same_bits(dy, got[i - 3][0], what + f" dy against run {i - 2}")
            G._same_bits(bst, got[i - 3][1], what + f" bstats against run {i - 2}")


@pytest.mark.parametrize("dt", G.DTS)
def test_act_bwd_db_rearms_across_geometries(dt):
    ops, Lb, code, epp = G._setup(dt)
    K.clamped_rows(Lb, "act_bwd_db", code, 1, *DB_A, epp)
    assert K.reduction_rows(Lb, "act_bwd_db", code, 1, *DB_B) == (0, 1, 1)
    _reset(ops, Lb)
    got = []
    for i, (P, Cc) in enumerate((DB_A, DB_B, DB_C, DB_A, DB_B)):
        what = f"run {i + 1} of A B C A B: act_bwd_db {(P, Cc)} {dt}"
        g, a = G._act_operands((1, P, Cc), F32, P + Cc)
        g, a = K.physical(g, DT[dt]), K.physical(a, DT[dt])
        prefill = torch.randn(Cc, generator=torch.Generator().manual_seed(P))
        gdx, dx = K.guarded_like((1, P, K.cpitch(Cc)), DT[dt], sentinel=K.SENTINEL)
        gdb, db = K.guarded_like((Cc,), F32, sentinel=K.SENTINEL)
        db.copy_(prefill)
        gd, ad = g.cuda(), a.cuda()
        ops.check(Lb.p2phd_act_bwd_db(code, ops.ptr(gd), ops.ptr(ad), ops.ptr(dx), P, Cc, LRELU, ops.ptr(db), 1, ops.stream_ptr()), what)
        G._done({"dx": gdx, "db": gdb}, what)
        if i < 3:
            G._check_act(dx, g, a, LRELU, DT[dt], what + " dx")
            K.colsum_check(dx, db, Cc, what + " db", prefill)
            got.append((dx, db))
        else:
            G._same_bits(dx, got[i - 3][0], what + f" dx against run {i - 2}")
            G._same_bits(db, got[i - 3][1], what + f" db against run {i - 2}")


@pytest.mark.parametrize("dt", G.DTS)
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_forward_rearms_across_geometries(kind, dt):
    """(40, 3) is 40 pieces: one workgroup; (30000, 67) takes the grid's cap of 1024 workgroups, (700, 67) 25."""
    ops, Lb, code, _ = G._setup(dt)
    target, coeff = 1.0, 2.5
    _reset(ops, Lb)
    got = []
    for i, (P, Cc) in enumerate((LOSS_A, LOSS_B, LOSS_C, LOSS_A, LOSS_B)):
        what = f"run {i + 1} of A B C A B: loss kind {kind} {(P, Cc)} {dt}"
        a, b = K.loss_data(P, Cc, dt, kind)
        ad, bd = a.cuda(), (b.cuda() if kind == 1 else None)
        go, out = K.guarded_like((1,), F32, sentinel=K.OUT0)
        ops.check(Lb.p2phd_loss_fwd(kind, code, ops.ptr(ad), ops.ptr(bd), target, P, Cc, coeff, ops.ptr(out), ops.stream_ptr()), what)
        G._done({"out": go}, what)
        if i < 3:
            want, bound = K.loss_fwd_reference(kind, a, b, target, Cc, coeff, K.OUT0)
            assert abs(float(out.cpu().double()) - want) <= bound, (what, float(out.cpu()), want, bound)
            got.append(out)
        else:
            G._same_bits(out, got[i - 3], what + f" against run {i - 2}")


@pytest.mark.parametrize("dt", G.DTS)
def test_split_k_tail_rearms_across_layers(dt):
    """The split-K tail of p2phd_conv_fwd (FOLD_GCONV): the three layers of _exact.SPLITK as A, B, C, A, B.  Integer operands: every
    run is compared bit for bit with the exact reference (run_fwd), statistics included, and must have taken the split-K path.
    (None of these layers has a one-workgroup launch.)"""
    ops, Lb = CE._ops(), CE._ops().lib_for(DT[dt])
    _reset(ops, Lb)
    with CE.options(Lb, splitk_tail=2):
        for i in (0, 1, 2, 0, 1):
            cnt = CE.run_fwd(X.SPLITK[i], dt, CE.NONE, True)
            assert cnt["splitk"] >= 1, (X.SPLITK[i].name, cnt)


# ----------------------------------------------------------------------------------------------------------------------
# one family on two streams
# ----------------------------------------------------------------------------------------------------------------------
CALLS = 16


def _in_bufs(shape, dtype, N, Cc):
    """Guarded outputs of one InstanceNorm backward operand set: dy, bstats, db."""
    bufs, t = {}, {}
    for name, shp, ty in (("dy", shape, dtype), ("bstats", (N, shape[2], 2), F32), ("db", (Cc,), F32)):
        bufs[name], t[name] = K.guarded_like(shp, ty, sentinel=K.SENTINEL)
    return bufs, t


def _in_launch(Lb, ops, code, grad, g, t, N, HW, Cc):
    """One p2phd_instnorm_act_bwd on the current stream, no synchronisation."""
    ops.check(Lb.p2phd_instnorm_act_bwd(code, ops.ptr(grad), ops.ptr(g["y"]), ops.ptr(g["stats"]), ops.ptr(t["bstats"]), ops.ptr(t["dy"]),
                                        ops.ptr(t["db"]), N, HW, Cc, K.EPS, RELU, ops.stream_ptr()), "instnorm_act_bwd")


def _two_streams(first, second, launch_x, launch_y):
    """CALLS launches of X on `first`, then -- with no host synchronisation in between -- one launch of Y on `second`."""
    torch.cuda.synchronize()
    with torch.cuda.stream(first):
        for _ in range(CALLS):
            launch_x()
    with torch.cuda.stream(second):
        launch_y()
    first.synchronize()
    second.synchronize()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", G.DTS)
def test_instnorm_backward_on_two_streams(dt):
    """Operand set X (a clamped two-pass case) 16 times back to back on one stream, then Y -- the same geometry, another gradient,
    its own output buffers -- once on another stream while X's launches are still queued; then the streams the other way round.
    Y's dy and bstats must have the bits of the same call alone, and so must X's.  If the event order of fold_scratch() were broken,
    the two reduce launches would share partial rows and tickets: wrong numbers, never a hang (fold_arrive_last does not spin), and
    the reset in `finally` keeps a failure from reaching later tests.

    What this cannot show: a pass does not prove the ordering -- the launches may have happened not to overlap --, the test only
    fails when the ordering is visibly broken.  Launches under graph capture neither wait nor record (csrc/core.hip, fold_scratch;
    ADVICE.md): two replayed graphs of one family on two streams are the caller's to order and out of scope here.  db (float
    atomics of the apply pass) is checked against its column sums only."""
    ops, Lb, code, epp = G._setup(dt)
    case = IN_A
    N, HW, Cc = case[:3]
    K.clamped_rows(Lb, "instnorm_bwd", code, N, HW, Cc, epp)
    d, g = G._in_dev(case, dt)
    shape = d["y"].shape
    gx, gy = g["g"], g["res"]                                                   # Y's gradient: the case's third random tensor
    try:
        _reset(ops, Lb)
        alone = {}
        for name, grad in (("X", gx), ("Y", gy)):                               # each alone, on one stream
            bufs, t = _in_bufs(shape, DT[dt], N, Cc)
            _in_launch(Lb, ops, code, grad, g, t, N, HW, Cc)
            G._done(bufs, f"instnorm_act_bwd {name} alone")
            K.colsum_check(t["dy"], t["db"], Cc, f"{name} alone: db")
            alone[name] = t
        assert not torch.equal(G._bits(alone["X"]["bstats"]), G._bits(alone["Y"]["bstats"]))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for first, second, order in ((s1, s2, "s1 then s2"), (s2, s1, "s2 then s1")):
            bx, tx = _in_bufs(shape, DT[dt], N, Cc)
            by, ty = _in_bufs(shape, DT[dt], N, Cc)
            _two_streams(first, second, lambda: _in_launch(Lb, ops, code, gx, g, tx, N, HW, Cc),
                         lambda: _in_launch(Lb, ops, code, gy, g, ty, N, HW, Cc))
            what = f"instnorm_act_bwd {case[:3]} {dt}, {order}"
            K.check_guards({**{"X " + k: v for k, v in bx.items()}, **{"Y " + k: v for k, v in by.items()}}, what)
            for name, t in (("Y", ty), ("X", tx)):
                G._same_bits(t["bstats"], alone[name]["bstats"], f"{what}: bstats of {name} against the call alone")
                G._same_bits(t["dy"], alone[name]["dy"], f"{what}: dy of {name} against the call alone")
                K.colsum_check(t["dy"], t["db"], Cc, f"{what}: db of {name}")
    finally:
        _reset(ops, Lb)
        torch.cuda.synchronize()


@pytest.mark.parametrize("dt", G.DTS)
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_forward_on_two_streams(kind, dt):
    """As test_instnorm_backward_on_two_streams (and with what it says a pass cannot show), for p2phd_loss_fwd on 1024 workgroups:
    X adds 16 times into one accumulator, Y once into its own; both must end with the bits of the same calls on one stream."""
    ops, Lb, code, _ = G._setup(dt)
    P, Cc = LOSS_A
    target, coeff = 1.0, 2.5
    xa, xb = (t.cuda() for t in K.loss_data(P, Cc, dt, kind))
    ya, yb = (t.cuda() for t in K.loss_data(P, Cc, dt, kind + 2))               # (another seed)

    def launch(a, b, out):
        ops.check(Lb.p2phd_loss_fwd(kind, code, ops.ptr(a), ops.ptr(b if kind == 1 else None), target, P, Cc, coeff, ops.ptr(out),
                                    ops.stream_ptr()), "loss_fwd")

    try:
        _reset(ops, Lb)
        gxo, xo = K.guarded_like((1,), F32, sentinel=K.OUT0)
        gyo, yo = K.guarded_like((1,), F32, sentinel=K.OUT0)
        for _ in range(CALLS):
            launch(xa, xb, xo)
        launch(ya, yb, yo)
        G._done({"X": gxo, "Y": gyo}, "loss_fwd alone")
        assert not torch.equal(G._bits(xo), G._bits(yo))
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for first, second, order in ((s1, s2, "s1 then s2"), (s2, s1, "s2 then s1")):
            gx2, xo2 = K.guarded_like((1,), F32, sentinel=K.OUT0)
            gy2, yo2 = K.guarded_like((1,), F32, sentinel=K.OUT0)
            _two_streams(first, second, lambda: launch(xa, xb, xo2), lambda: launch(ya, yb, yo2))
            what = f"loss kind {kind} {LOSS_A} {dt}, {order}"
            K.check_guards({"X": gx2, "Y": gy2}, what)
            G._same_bits(yo2, yo, what + ": Y against the call alone")
            G._same_bits(xo2, xo, what + ": X against the calls alone")
    finally:
        _reset(ops, Lb)
        torch.cuda.synchronize()
