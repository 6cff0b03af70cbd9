"""CPU checks of tests/_companions.py, the references and bounds of tests/test_gpu_companions.py:
  * the float64 references equal torch-CPU float64 autograd of the same operations;
  * the bounds are usable: a torch float32 emulation of each kernel expression, in the kernel's operation order and with the
    16-bit storage rounding, passes every bound on the GPU module's case table;
  * the bounds bite: every listed mutant of that emulation fails its check;
  * the host query p2phd_instnorm_act_bwd_two_pass answers what the case table says, for both element sizes and both libraries."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _companions as K
from _companions import NONE, LRELU, TANH, RELU, DT

DTS = ["bf16", "f16", "f32"]
F32 = torch.float32
ACTF = {NONE: lambda v: v, LRELU: lambda v: F.leaky_relu(v, K.SLOPE32), RELU: F.relu}


def f32(v):
    return torch.tensor(float(v), dtype=F32)


# ----------------------------------------------------------------------------------------------------------------------
# float32 emulations of the kernel expressions (torch CPU float32: every operation rounded once, no fma)
# ----------------------------------------------------------------------------------------------------------------------
def emu_consts(stats, HW, C, mut):
    inv = f32(1.0) / f32(HW - 1 if mut == "unbiased" else HW)
    arg = (stats[..., 1] * inv).clamp(min=0)
    if mut != "no_eps":
        arg = arg + f32(K.EPS)
    rstd = torch.rsqrt(arg)
    rstd[:, C:] = 0
    return stats[..., 0][:, None], rstd[:, None], inv


def emu_slope(act, mut):
    return f32(0.25 if (mut == "slope025" and act == LRELU) else K.slope_of(act))


def emu_in_fwd(d, HW, C, act, residual, dtype, mut=None):
    mean, rstd, _ = emu_consts(d["stats"], HW, C, mut)
    sl = emu_slope(act, mut)
    yh = (d["y"].float() - mean) * rstd
    if residual and mut == "res_before_act":
        yh = yh + d["res"].float()
    f = torch.where(yh > 0, yh, sl * yh)
    if residual and mut != "res_before_act":
        f = f + d["res"].float()
    f[..., C:] = 0
    return f.to(dtype), f


def emu_in_bwd(d, HW, C, act, dtype, mut=None):
    mean, rstd, inv = emu_consts(d["stats"], HW, C, mut)
    sl = emu_slope(act, mut)
    yh = (d["y"].float() - mean) * rstd
    gp = d["g"].float() * torch.where(yh > 0, f32(1.0), sl)
    s1, s2 = gp.sum(1), (gp * yh).sum(1)
    m1 = (s1 / f32(HW - 1) if mut == "m1_hw_minus_1" else s1 * inv)[:, None]
    m2 = (s2 * inv)[:, None]
    dy = rstd * (gp - m1 if mut == "drop_yh_m2" else gp - m1 - yh * m2)
    dy = dy.to(dtype)
    return dy, torch.stack([s1, s2], -1), dy.float().sum((0, 1))


def check_in_fwd(out, d, HW, C, act, residual, dtype, what):
    want, b32 = K.instnorm_fwd_reference(d["y"], d["stats"], d["res"] if residual else None, HW, C, K.EPS, act)
    K.assert_within(out, want, K.stored_bound(want, b32, dtype), what, C)


def check_in_bwd(dy, bst, db, d, HW, C, act, dtype, what):
    ref = K.instnorm_bwd_reference(d["g"], d["y"], d["stats"], HW, C, K.EPS, act)
    K.assert_within(dy, ref["dy"], K.stored_bound(ref["dy"], ref["b32"], dtype), what + " dy", C)
    K.bstats_check(bst, ref, C, what + " bstats")
    K.colsum_check(dy, db, C, what + " db")


def emu_tanh_bwd(g, a, dtype):
    o = a.float()
    return (g.float() * (f32(1.0) - o * o)).to(dtype)


def emu_pool_fwd(x, dtype, mut=None):
    N, H, W, Cp = x.shape
    acc = torch.zeros(N, K.pool_out(H), K.pool_out(W), Cp, dtype=F32)
    for a, b, hs, ws in K._windows(H, W):
        acc[:, hs[:, None], ws[None, :]] += x.float()[:, (2 * hs - 1 + a)[:, None], (2 * ws - 1 + b)[None, :]]
    cnt = torch.full_like(K.pool_counts(H, W), 9.0) if mut == "include_pad" else K.pool_counts(H, W)
    return (acc * (f32(1.0) / cnt.float())[None, :, :, None]).to(dtype)


def emu_pool_bwd(dy, H, W, dtype, mut=None):
    N, Ho, Wo, Cp = dy.shape
    cnt = K.pool_counts(H, W).float()
    dx = torch.zeros(N, H, W, Cp, dtype=F32)
    for a, b, hs, ws in K._windows(H, W):
        hi, wi = (2 * hs - 1 + a), (2 * ws - 1 + b)
        if mut == "input_count":        # the count looked up at the INPUT pixel's coordinates (clipped into the table)
            c = cnt[hi.clamp(max=Ho - 1)[:, None], wi.clamp(max=Wo - 1)[None, :]]
        else:
            c = cnt[hs[:, None], ws[None, :]]
        dx[:, hi[:, None], wi[None, :]] += dy.float()[:, hs[:, None], ws[None, :]] * (f32(1.0) / c)[None, :, :, None]
    return dx.to(dtype)


def emu_loss_fwd(kind, a, b, target, C, coeff, out0, mut=None):
    P, Cp = a.shape
    x = a.float()[:, :C]
    t = (x - f32(target)) ** 2 if kind == 0 else (x - b.float()[:, :C]).abs()
    return float(f32(out0) + t.sum() * f32(coeff) / f32(P * (Cp if mut == "div_cp" else C)))


def emu_loss_bwd(kind, a, b, target, C, coeff, gup, dtype, mut=None):
    P, Cp = a.shape
    s = f32(gup) * f32(coeff) / f32(P * C)
    x = a.float()
    if kind == 0:
        g = f32(2.0) * (x - f32(target)) * s
    else:
        d = x - b.float()
        g = torch.where(d > 0, s, torch.where(d < 0, -s, s if mut == "l1_plus_at_zero" else f32(0.0)))
    g = g.clone()
    g[:, C:] = 0
    return g.to(dtype)


def emu_adam(p, g, m, v, lr, b1, b2, eps, t, gscale, mut=None):
    b1, b2 = f32(b1), f32(b2)
    bc1 = f32(1.0 if mut == "no_bias_correction" else 1.0 - float(b1) ** t)
    bc2s = f32(1.0 if mut == "no_bias_correction" else (1.0 - float(b2) ** t) ** 0.5)
    gr = g * f32(gscale)
    m1 = b1 * m + (f32(1.0) - b1) * gr
    v1 = b2 * v + (f32(1.0) - b2) * gr * gr
    den = torch.sqrt(v1 + f32(eps)) / bc2s if mut == "eps_in_sqrt" else torch.sqrt(v1) / bc2s + f32(eps)
    return p - (f32(lr) / bc1) * m1 / den, m1, v1


def check_adam(got, p, g, m, v, t, what):
    want, bounds = K.adam_reference(p, g, m, v, 2e-4, 0.5, 0.999, 1e-8, t, 0.25)
    for name, a, w, b in zip("pmv", got, want, bounds):
        K.assert_within(a, w, b, f"{what} {name}")


# ----------------------------------------------------------------------------------------------------------------------
# the references are the operations torch computes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [NONE, LRELU, RELU])
def test_instnorm_references_equal_float64_autograd(act):
    gen = torch.Generator().manual_seed(act)
    N, C, H, W = 3, 5, 4, 7
    x = (torch.randn(N, C, H, W, generator=gen, dtype=torch.float64) * 2 + 1).requires_grad_(True)
    r = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    g = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    out = ACTF[act](F.instance_norm(x, eps=float(np.float32(K.EPS)))) + r
    (gx,) = torch.autograd.grad((ACTF[act](F.instance_norm(x, eps=float(np.float32(K.EPS)))) * g).sum(), x)
    phys = lambda t: K.physical(t.detach().permute(0, 2, 3, 1).reshape(N, H * W, C), torch.float64)
    xp = phys(x)
    mean = xp.mean(1)
    stats = torch.stack([mean, ((xp - mean[:, None]) ** 2).sum(1)], -1)
    want, _ = K.instnorm_fwd_reference(xp, stats, phys(r), H * W, C, K.EPS, act)
    assert float((want - phys(out)).abs().max()) < 1e-12
    assert float(want[..., C:].abs().max()) == 0
    ref = K.instnorm_bwd_reference(phys(g), xp, stats, H * W, C, K.EPS, act)
    assert float((ref["dy"] - phys(gx)).abs().max()) < 1e-11
    # M2 < 0 is clamped: the same result as M2 = 0
    neg, zero = stats.clone(), stats.clone()
    neg[..., 1], zero[..., 1] = -1e-3, 0.0
    assert torch.equal(K.instnorm_fwd_reference(xp, neg, None, H * W, C, K.EPS, act)[0], K.instnorm_fwd_reference(xp, zero, None, H * W, C, K.EPS, act)[0])


@pytest.mark.parametrize("geom", K.POOL_CASES, ids=lambda g: "x".join(map(str, g)))
def test_avgpool_references_equal_float64_autograd(geom):
    N, C, H, W = geom
    gen = torch.Generator().manual_seed(H * 16 + W)
    x = torch.randn(N, C, H, W, generator=gen, dtype=torch.float64).requires_grad_(True)
    y = F.avg_pool2d(x, 3, 2, [1, 1], count_include_pad=False)
    assert tuple(y.shape[2:]) == (K.pool_out(H), K.pool_out(W))
    cot = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (gx,) = torch.autograd.grad((y * cot).sum(), x)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    want, _ = K.avgpool_fwd_reference(nhwc(x))
    assert float((want - nhwc(y)).abs().max()) < 1e-13
    dx, _ = K.avgpool_bwd_reference(nhwc(cot), H, W)
    assert float((dx - nhwc(gx)).abs().max()) < 1e-13


def test_loss_references_equal_float64_autograd():
    P, C = 40, 3
    a, b = K.loss_data(P, C, "f32", 1)
    ad = a.double()[:, :C].clone().requires_grad_(True)
    bd = b.double()[:, :C]
    mse = F.mse_loss(ad, torch.full_like(ad, 1.0))
    l1 = F.l1_loss(ad, bd)
    want0, _ = K.loss_fwd_reference(0, a, None, 1.0, C, 2.5, K.OUT0)
    want1, _ = K.loss_fwd_reference(1, a, b, 0.0, C, 2.5, K.OUT0)
    assert abs(want0 - (K.OUT0 + 2.5 * float(mse.detach()))) < 1e-12 and abs(want1 - (K.OUT0 + 2.5 * float(l1.detach()))) < 1e-12
    (g0,) = torch.autograd.grad(1.75 * 2.5 * mse, ad)
    (g1,) = torch.autograd.grad(1.75 * 2.5 * l1, ad)
    r0 = K.loss_bwd_reference(0, a, None, 1.0, C, 2.5, 1.75, F32)
    r1 = K.loss_bwd_reference(1, a, b, 0.0, C, 2.5, 1.75, F32)
    assert float((r0[:, :C].double() - g0).abs().max()) < 4 * K.U32 * float(g0.abs().max())
    assert float((r1[:, :C].double() - g1).abs().max()) < 4 * K.U32 * float(g1.abs().max())
    assert bool((r1[:, :C][a[:, :C] == b[:, :C]] == 0).all()) and int((a[:, :C] == b[:, :C]).sum()) > 0
    assert float(r0[:, C:].abs().max()) == 0 and float(r1[:, C:].abs().max()) == 0


def test_adam_reference_equals_torch_adam_over_three_steps():
    f = lambda s: float(np.float32(s))
    n = 257
    p0, _, _, _ = K.adam_state(n, 3)
    ref = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=f(2e-4), betas=(0.5, f(0.999)), eps=f(1e-8))
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    gen = torch.Generator().manual_seed(4)
    for t in range(1, 4):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        ref.grad = g.clone()
        opt.step()
        (p, m, v), _ = K.adam_reference(p, g, m, v, 2e-4, 0.5, 0.999, 1e-8, t, 1.0)
    assert float((p - ref.detach()).abs().max()) < 1e-13
    st = opt.state[ref]
    assert float((m - st["exp_avg"]).abs().max()) < 1e-14 and float((v - st["exp_avg_sq"]).abs().max()) < 1e-14


def test_scaler_reference_is_the_gradscaler_update_rule():
    """torch.cuda.amp.GradScaler.update (torch/csrc: _amp_update_scale_): found -> scale *= backoff, tracker = 0; else the tracker
    counts up and at growth_interval the scale grows and the tracker restarts.  torch compares with ==, where its tracker can
    never pass the interval; the kernel's >= reads a tracker above it (a lowered interval) as due."""
    for state, growth, backoff, interval in K.SCALER_TABLE:
        scale, _, tracker, f0, f1 = state
        if f0 or f1:
            scale, tracker = scale * backoff, 0.0
        else:
            tracker += 1.0
            if tracker >= interval:
                scale, tracker = scale * growth, 0.0
        got = K.scaler_update_reference(state, growth, backoff, interval)
        assert [float(x) for x in got] == [float(np.float32(scale)), float(np.float32(1.0) / np.float32(scale)), tracker, 0.0, 0.0]
    kinds = {(bool(s[3]), bool(s[4])) for s, *_ in K.SCALER_TABLE}
    assert kinds == {(True, False), (False, True), (True, True), (False, False)}


# ----------------------------------------------------------------------------------------------------------------------
# the bounds are usable: the float32 emulation passes them on the whole case table
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", K.IN_CASES, ids=K.IN_IDS)
def test_instnorm_emulation_passes_its_bounds(case, dt):
    N, HW, C = case[:3]
    d, dtype = K.in_data(case, dt), DT[dt]
    assert float(d["y"][:, :, K.CH_7SIGMA].float().mean().abs()) > 0 and bool((d["y"][:, ::3, K.CH_ONMEAN].float() == K.ONMEAN).all())
    for act in (NONE, RELU, LRELU):
        for residual in (False, True):
            out, f = emu_in_fwd(d, HW, C, act, residual, dtype)
            check_in_fwd(out, d, HW, C, act, residual, dtype, f"fwd {case[:3]} {dt} act {act} res {residual}")
            if dt != "f32" and not residual:
                want, b32 = K.instnorm_fwd_reference(d["y"], d["stats"], None, HW, C, K.EPS, act)
                o8 = f.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
                K.assert_q8_neighbours(o8, want, b32, f"q8 {case[:3]} {dt} act {act}", C)
        dy, bst, db = emu_in_bwd(d, HW, C, act, dtype)
        check_in_bwd(dy, bst, db, d, HW, C, act, dtype, f"bwd {case[:3]} {dt} act {act}")


@pytest.mark.parametrize("dt", DTS)
def test_other_emulations_pass_their_bounds(dt):
    dtype = DT[dt]
    gen = torch.Generator().manual_seed(9)
    # TANH backward
    a = torch.tanh(torch.randn(700, 72, generator=gen)).to(dtype)
    g = torch.randn(700, 72, generator=gen).to(dtype)
    want, bound = K.act_bwd_reference(g, a, TANH, dtype)
    K.assert_within(emu_tanh_bwd(g, a, dtype), want, bound, "tanh")
    for act, sl in ((NONE, 1.0), (RELU, 0.0), (LRELU, 0.2)):
        exact, none = K.act_bwd_reference(g, a, act, dtype)
        assert none is None
        K.assert_bits_equal((g.float() * torch.where(a.float() > 0, f32(1.0), f32(sl))).to(dtype), exact, "flat", f"act {act}")
    # AvgPool
    for N, C, H, W in K.POOL_CASES:
        x = K.physical(torch.randn(N, H * W, C, generator=gen), dtype).reshape(N, H, W, -1)
        want, b32 = K.avgpool_fwd_reference(x)
        K.assert_within(emu_pool_fwd(x, dtype).reshape(N, -1, x.shape[3]), want, K.stored_bound(want, b32, dtype), f"pool fwd {H}x{W}", C)
        dy = K.physical(torch.randn(N, K.pool_out(H) * K.pool_out(W), C, generator=gen), dtype).reshape(N, K.pool_out(H), K.pool_out(W), -1)
        want, b32 = K.avgpool_bwd_reference(dy, H, W)
        K.assert_within(emu_pool_bwd(dy, H, W, dtype).reshape(N, -1, x.shape[3]), want, K.stored_bound(want, b32, dtype), f"pool bwd {H}x{W}", C)
    # losses
    for P, C in K.LOSS_CASES:
        for kind in (0, 1):
            a, b = K.loss_data(P, C, dt, kind)
            want, bound = K.loss_fwd_reference(kind, a, b, 1.0, C, 2.5, K.OUT0)
            got = emu_loss_fwd(kind, a, b, 1.0, C, 2.5, K.OUT0)
            assert abs(got - want) <= bound, (P, C, kind, got, want, bound)
            K.assert_bits_equal(emu_loss_bwd(kind, a, b, 1.0, C, 2.5, 1.75, dtype), K.loss_bwd_reference(kind, a, b, 1.0, C, 2.5, 1.75, dtype),
                                "flat", f"loss bwd {P}x{C} kind {kind}")


@pytest.mark.parametrize("t", [1, 1000])
def test_adam_emulation_passes_its_bounds(t):
    for n in K.ADAM_SIZES[:5] + [100003]:
        p, g, m, v = K.adam_state(n, n + t)
        check_adam(emu_adam(p, g, m, v, 2e-4, 0.5, 0.999, 1e-8, t, 0.25), p, g, m, v, t, f"adam n {n} t {t}")


# ----------------------------------------------------------------------------------------------------------------------
# the bounds bite
# ----------------------------------------------------------------------------------------------------------------------
MUT_CASE = K.IN_CASES[7]                                               # (2, 4, 32): HW - 1 against HW is 4 / 3


@pytest.mark.parametrize("dt", DTS)
def test_instnorm_mutants_fail(dt):
    N, HW, C = MUT_CASE[:3]
    d, dtype = K.in_data(MUT_CASE, dt), DT[dt]
    for mut, act, residual in (("unbiased", NONE, False), ("no_eps", NONE, False), ("res_before_act", RELU, True), ("slope025", LRELU, False)):
        out, _ = emu_in_fwd(d, HW, C, act, residual, dtype, mut)
        assert K.fails(check_in_fwd, out, d, HW, C, act, residual, dtype, mut), ("forward", mut)
        check_in_fwd(emu_in_fwd(d, HW, C, act, residual, dtype)[0], d, HW, C, act, residual, dtype, "unmutated")
    for mut, act in (("unbiased", RELU), ("no_eps", RELU), ("drop_yh_m2", RELU), ("m1_hw_minus_1", RELU), ("slope025", LRELU)):
        dy, bst, db = emu_in_bwd(d, HW, C, act, dtype, mut)
        assert K.fails(check_in_bwd, dy, bst, db, d, HW, C, act, dtype, mut), ("backward", mut)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", [K.IN_CASES[7], K.IN_CASES[11], K.IN_CASES[4]], ids=lambda c: "x".join(map(str, c[:3])))
def test_an_element_left_at_the_sentinel_fails(case, dt):
    """One sample, one pixel or one 16-byte channel piece that the kernel did not write keeps the sentinel of guarded_like."""
    N, HW, C = case[:3]
    d, dtype = K.in_data(case, dt), DT[dt]
    epp = 4 if dt == "f32" else 8
    Cp = K.cpitch(C)
    holes = {"sample": (slice(N - 1, N), slice(None), slice(None)), "pixel": (slice(None), slice(HW - 1, HW), slice(None)),
             "piece": (slice(0, 1), slice(HW // 2, HW // 2 + 1), slice(Cp - epp, Cp))}       # the last piece: pad channels where there are any
    for name, sl in holes.items():
        out, _ = emu_in_fwd(d, HW, C, LRELU, True, dtype)
        out[sl] = K.SENTINEL
        assert K.fails(check_in_fwd, out, d, HW, C, LRELU, True, dtype, name), ("forward", name)
        dy, bst, db = emu_in_bwd(d, HW, C, RELU, dtype)
        dy[sl] = K.SENTINEL
        assert K.fails(check_in_bwd, dy, bst, dy.float().sum((0, 1)), d, HW, C, RELU, dtype, name), ("backward", name)


@pytest.mark.parametrize("dt", DTS)
def test_activation_pool_and_loss_mutants_fail(dt):
    dtype = DT[dt]
    gen = torch.Generator().manual_seed(10)
    a, g = torch.randn(40, 40, generator=gen).to(dtype), torch.randn(40, 40, generator=gen).to(dtype)
    exact, _ = K.act_bwd_reference(g, a, LRELU, dtype)
    assert K.fails(K.assert_bits_equal, (g.float() * torch.where(a.float() > 0, f32(1.0), f32(0.25))).to(dtype), exact, "flat", "slope 0.25")
    N, C, H, W = K.POOL_CASES[5]
    x = K.physical(torch.randn(N, H * W, C, generator=gen), dtype).reshape(N, H, W, -1)
    want, b32 = K.avgpool_fwd_reference(x)
    flat = lambda t: t.reshape(N, -1, x.shape[3])
    assert K.fails(K.assert_within, flat(emu_pool_fwd(x, dtype, "include_pad")), want, K.stored_bound(want, b32, dtype), "include_pad", C)
    dy = K.physical(torch.randn(N, 12, C, generator=gen), dtype).reshape(N, 4, 3, -1)
    want, b32 = K.avgpool_bwd_reference(dy, H, W)
    K.assert_within(flat(emu_pool_bwd(dy, H, W, dtype)), want, K.stored_bound(want, b32, dtype), "unmutated", C)
    assert K.fails(K.assert_within, flat(emu_pool_bwd(dy, H, W, dtype, "input_count")), want, K.stored_bound(want, b32, dtype), "input_count", C)
    P, C = K.LOSS_CASES[1]                                               # (700, 67): masked, P Cp / (P C) = 72 / 67
    for kind in (0, 1):
        a, b = K.loss_data(P, C, dt, kind)
        want, bound = K.loss_fwd_reference(kind, a, b, 1.0, C, 2.5, K.OUT0)
        assert abs(emu_loss_fwd(kind, a, b, 1.0, C, 2.5, K.OUT0, "div_cp") - want) > bound
    a, b = K.loss_data(P, C, dt, 1)
    assert K.fails(K.assert_bits_equal, emu_loss_bwd(1, a, b, 0.0, C, 2.5, 1.75, dtype, "l1_plus_at_zero"),
                   K.loss_bwd_reference(1, a, b, 0.0, C, 2.5, 1.75, dtype), "flat", "+s at a == b")


@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("mut", ["no_bias_correction", "eps_in_sqrt"])
def test_adam_mutants_fail(mut, t):
    p, g, m, v = K.adam_state(1003, 5)
    assert K.fails(check_adam, emu_adam(p, g, m, v, 2e-4, 0.5, 0.999, 1e-8, t, 0.25, mut), p, g, m, v, t, mut)


# ----------------------------------------------------------------------------------------------------------------------
# which form of the InstanceNorm backward a case takes (host arithmetic of the library: no device needed)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_two_pass_query_matches_the_case_table(kind):
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib(kind)
    for N, HW, C, two_pass, _ in K.IN_CASES:
        for code in (_lib.F32, _lib.BF16):
            assert L.p2phd_instnorm_act_bwd_two_pass(code, N, HW, C) == two_pass, (kind, code, N, HW, C)
    assert L.p2phd_instnorm_act_bwd_two_pass(_lib.BF16, 0, 64, 64) == 0 and L.p2phd_instnorm_act_bwd_two_pass(_lib.BF16, 64, 0, 64) == 0
    # the rule's own edges: 127 / 128 (sample, column block) pairs
    assert L.p2phd_instnorm_act_bwd_two_pass(_lib.BF16, 127, 64, 3) == 1 and L.p2phd_instnorm_act_bwd_two_pass(_lib.BF16, 128, 64, 3) == 0
