"""CPU checks of tests/_timed_ref.py: the float64 references against tests/_time_d_ref.py, the conditions of the operands, the
float32 emulations of the three kernels of csrc/timed.hip inside their derived bounds, and planted defects outside them.  Only
the emulations and the reference's algorithm are measured here, never the kernels."""
import numpy as np
import pytest
import torch

import _companions as K
import _time_d_ref as T
import _timed_ref as D
import _transform_ref as R
from _exact import U32

PIN = 1e-12
B, F = 2, 5                                                           # F = 5: a partial last tile at every f_tile (16, 8, 4)
NAMES3 = ("b", "t", "i")
NAMES4 = ("b", "c", "k", "t")


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def _fwd_check(got, case, what):
    return R.assert_elements_close(got, case["want"], case["tol"], what, NAMES3)


def _bwd_check(got, case, what):
    return R.assert_elements_close(got, case["want"], case["tol"], what, NAMES4)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the references against the restatement of the reference's branch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", [16, 64, 512])
def test_references_agree_with_the_restatement(n_fft, monkeypatch):
    """_transform_ref holds the kernels' 0.05f (C005 = float32(0.05), 2^-26 relative above 0.05) in t; the restatement divides by
    20.  With that one constant set to 0.05 the two agree to 1e-12: layout, window, scale, transform, signs and the derivative."""
    monkeypatch.setattr(R, "C005", 0.05)
    sr, mm = D.dense_operands(B, n_fft, F, 5 + n_fft)
    w = R.window("ramp", n_fft, 1)
    s32 = float(np.float32(D.SCALE))
    args = (float(mm[0]), float(mm[1]), float(np.float32(D.ALPHA)), float(np.float32(D.MIN_VALUE)), 1.0 + s32 * s32,
            torch.from_numpy(w).double())
    want, tol = D.frames_fwd_ref(sr, mm, w, D.ALPHA, D.MIN_VALUE, D.SCALE, "dense")
    x64 = torch.from_numpy(sr).double().requires_grad_(True)
    ref = T.sr_frames(x64, *args)[:, 0]
    assert want.shape == tuple(ref.shape) and _rel(want, ref.detach().numpy()) <= PIN
    assert (tol > 0).all()
    g = D.cotangent(B, n_fft, F, 6 + n_fft)
    (gx,) = torch.autograd.grad(ref, x64, torch.from_numpy(g).double())
    gw, gtol = D.frames_bwd_ref(g, sr, mm, w, D.ALPHA, D.SCALE)
    assert gw.shape == tuple(gx.shape) and _rel(gw, gx.numpy()) <= PIN
    zero = sr == 0
    assert zero.any() and not gw[zero].any() and not gtol[zero].any()  # x == 0 (either sign): exactly zero is demanded
    assert (gtol[~zero] > 0).all()


@pytest.mark.parametrize("n_fft", D.N_FFTS)
def test_kernel_factorisation_is_the_dct3(n_fft):
    X = R.signal((3, n_fft), 40 + n_fft)
    assert _rel(D.kernel_dct3_64(X), R.dct3_rows(X)) <= PIN
    assert _rel(D.kernel_dct3_64(X, "rev_bins"), R.dct3_rows(X)) > 1e-2


# ----------------------------------------------------------------------------------------------------------------------
# 2. conditions of the operands
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", D.GEOMS, ids=D.GEOM_IDS)
def test_operand_conditions(geom):
    n_fft, Bc, Fc = geom
    x, mm = D.dense_operands(Bc, n_fft, Fc, D.case_seed(*geom))
    assert x.dtype == np.float32 and x.shape == (Bc, 2, n_fft, Fc) and np.abs(x).max() == 1.0
    pos0 = (x == 0) & ~np.signbit(x)
    neg0 = (x == 0) & np.signbit(x)
    assert pos0.any() and neg0.any() and (x == 1).any() and (x == -1).any()
    assert np.array_equal(x[:, 1, n_fft // 2], x[:, 0, n_fft // 2]) and np.array_equal(x[:, 1, n_fft // 4], -x[:, 0, n_fft // 4])
    S, _ = R.decode_ref(x, mm, D.ALPHA, D.MIN_VALUE)
    assert not S[:, :, n_fft // 2].any() and not S[:, :, n_fft // 4].any()    # |x0| == |x1|: exactly zero
    assert (S != 0).mean() > 0.8
    t, mm2 = D.two_level_operands(Bc, n_fft, Fc, 1 + D.case_seed(*geom))
    assert set(np.unique(np.abs(t))) == {0.5, 1.0} and (t < 0).any() and (t > 0).any()
    g = D.cotangent(Bc, n_fft, Fc, 3, impulse=True)
    assert np.array_equal((g != 0).sum(-1), np.ones((Bc, Fc))) and g.max() == 1.0


@pytest.mark.parametrize("n_fft", D.N_FFTS)
def test_two_level_premise(n_fft):
    """One magnitude per non-zero bin -- in the float64 reference and in the float32 emulation of the decode --, zero where
    |x0| == |x1|, and rho <= 64 u."""
    x, mm = D.two_level_operands(B, n_fft, F, 9 + n_fft)
    S, tolS = R.decode_ref(x, mm, D.ALPHA, D.MIN_VALUE)
    S32 = D.decode_model32(x, mm, D.ALPHA, D.MIN_VALUE)
    same = (np.abs(x[:, 0]) == np.abs(x[:, 1])).transpose(0, 2, 1)
    for name, s in (("float64", S), ("float32", S32)):
        assert not s[same].any(), name
        assert (s[~same] != 0).all() and len(np.unique(np.abs(s[~same]))) == 1, (name, np.unique(np.abs(s[~same])))
    assert 0.3 < same.mean() < 0.7
    rho = D.rho_of(S, tolS)
    print(f"n_fft {n_fft}: rho = {rho / U32:.2f} u, |S| = {np.abs(S[~same])[0]!r}, float32 {np.abs(S32[~same])[0]!r}")
    assert 0 < rho <= D.RHO_MAX
    assert abs(float(np.abs(S32[~same])[0]) / float(np.abs(S[~same])[0]) - 1.0) <= rho


def test_pack_operands_and_the_clamp_floor():
    a, b = D.pack_operands(1027, 3)
    for v in D.PLANTED:
        v32 = np.float32(v)
        for arr in (a, b):
            assert ((arr == v32) & (np.signbit(arr) == np.signbit(v32))).any(), v
    a1, b1 = D.pack_operands(1, 3)
    assert a1[0] == 0 and b1[0] == -1e3                                # the smallest size holds the two extremes of the range
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny            # the planted subnormal is one
    floor = 20.0 * np.log10(D.MIN_VALUE) - 20.0
    for dt in K.DT.values():
        want, tol = D.pack_db_ref(a, b, D.MIN_VALUE, dt)
        clamped = np.stack([np.abs(a) <= np.float32(D.MIN_VALUE), np.abs(b) <= np.float32(D.MIN_VALUE)], -1)
        assert clamped.sum() >= 16 and (np.abs(want[clamped] - floor) <= tol[clamped]).all(), dt
        assert (tol > 0).all() and (tol[clamped] < (2e-4 if dt == torch.float32 else 1.0)).all()


# ----------------------------------------------------------------------------------------------------------------------
# 3. the emulations stay inside the bounds; 4. the mutants do not
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft", D.N_FFTS)
def test_forward_emulation_inside_and_mutants_outside(n_fft):
    for kind in ("dense", "two_level"):
        c = D.fwd_case(kind, n_fft, B, F)
        got = D.frames_fwd_model32(c["sr"], c["mm"], c["w"], D.ALPHA, D.MIN_VALUE, c["scale"])
        worst = _fwd_check(got, c, f"forward {kind} n_fft {n_fft}")
        floor = float((c["tol"] / np.sqrt((c["want"] ** 2).sum(-1, keepdims=True))).min())
        print(f"forward {kind} n_fft {n_fft}: worst |err| / tol = {worst:.3f}; smallest tol / ||frame||_2 = {floor:.2e}")
        assert worst <= 0.5
    # every mutant fails the two-level check; the dense one, whose bound carries the worst-case decode term, is the structural
    # check: it rejects all but the single dropped bin (a quiet bin stays inside it)
    for kind in ("two_level", "dense"):
        c = D.fwd_case(kind, n_fft, B, F)
        for mutant in D.FWD_MUTANTS:
            if kind == "dense" and mutant == "drop_bin":
                continue
            got = D.frames_fwd_model32(c["sr"], c["mm"], c["w"], D.ALPHA, D.MIN_VALUE, c["scale"], mutant)
            assert K.fails(_fwd_check, got, c, mutant), (n_fft, kind, mutant)


@pytest.mark.parametrize("impulse", [False, True], ids=["normal", "impulse"])
@pytest.mark.parametrize("n_fft", D.N_FFTS)
def test_backward_emulation_inside_and_mutants_outside(n_fft, impulse):
    c = D.bwd_case(n_fft, B, F, impulse)
    got = D.frames_bwd_model32(c["g"], c["sr"], c["mm"], c["w"], D.ALPHA, c["scale"])
    worst = _bwd_check(got, c, f"backward n_fft {n_fft} impulse {impulse}")
    print(f"backward n_fft {n_fft} impulse {impulse}: worst |err| / tol = {worst:.3f}")
    assert worst <= 0.5
    zero = c["sr"] == 0
    assert zero.any() and not got[zero].any()
    for mutant in D.BWD_MUTANTS:
        got = D.frames_bwd_model32(c["g"], c["sr"], c["mm"], c["w"], D.ALPHA, c["scale"], mutant)
        assert K.fails(_bwd_check, got, c, mutant), (n_fft, impulse, mutant)


@pytest.mark.parametrize("dt", list(K.DT), ids=list(K.DT))
def test_pack_db_emulation_inside_and_mutants_outside(dt):
    """Held to the bound itself, not to half of it as the transforms' emulations are: the bound is a sum of single roundings, and
    one rounding can use its term up.  float32: d just below -16 has half an ulp of 16 u against the u |d| <= 20 u granted for the
    subtraction, and hardly anything else (|L| is small there): up to 0.8 of the bound with a correctly rounded log10f (measured:
    0.75).  16-bit storage: the rounding to the stored type is up to the half ulp the bound grants for it: up to 1.0."""
    dtype = K.DT[dt]
    a, b = D.pack_operands(1027, 11)
    want, tol = D.pack_db_ref(a, b, D.MIN_VALUE, dtype)
    names = ("pixel", "channel")
    worst = R.assert_elements_close(D.pack_db_model32(a, b, D.MIN_VALUE, dtype), want, tol, f"pack dB {dt}", names)
    print(f"pack dB {dt}: worst |err| / tol = {worst:.3f}")
    assert worst <= (0.8 if dtype == torch.float32 else 1.0)
    for mutant in D.PACK_MUTANTS:
        got = D.pack_db_model32(a, b, D.MIN_VALUE, dtype, mutant)
        assert K.fails(R.assert_elements_close, got, want, tol, mutant, names), (dt, mutant)


def test_a_dropped_bin_hides_in_the_relative_l2_norm():
    """Why these tests exist: one bin of one frame dropped fails the per-element bound by orders of magnitude and moves the
    tensor-wide relative L2 norm, the measure of tests/test_gpu_time_d.py, far less."""
    from conftest import rel_err
    c = D.fwd_case("two_level", 2048, B, F)
    got = D.frames_fwd_model32(c["sr"], c["mm"], c["w"], D.ALPHA, D.MIN_VALUE, c["scale"], "drop_bin")
    err = np.abs(got.astype(np.float64) - c["want"])
    ratio = float((err / c["tol"]).max())
    l2 = rel_err(got, c["want"])
    print(f"dropped bin at n_fft 2048: worst |err| / tol = {ratio:.0f}, tensor-wide relative L2 = {l2:.2e}")
    assert ratio > 1000 and l2 < 2e-2
