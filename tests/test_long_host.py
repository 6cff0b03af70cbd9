"""Past the grid cap, on the host: p2phd_stream_grid pinned to today's figures for every family, every case of tests/_long.py
shown to be past two trips with a partial last one, the numpy emulation of a strided launch and its mutants (what
tests/test_gpu_long.py would see if a loop were wrong), and the vectorised references against the restatements they vectorise."""
import numpy as np
import pytest

import torch

import _companions as C
import _generate_ref as G
import _long as K


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------
# the grids
# ------------------------------------------------------------------------------------------
# (family, dtype, rows) -> work above which used < wanted: the table of DESIGN.md, "Past the grid cap"
LOOPS_ABOVE = {
    ("segments_gather", 0, 1): 16777216, ("segments_gather_planar", 0, 2): 16777216, ("segments_stitch", 0, 1): 16777216,
    ("segments_stitch_planar", 0, 3): 16777216,
    ("pcm_decode", 0, 1): 4194304, ("pcm_encode", 0, 1): 4194304, ("pcm_encode_ex", 0, 1): 4194304,
    ("pcm_peak", 0, 8): 1048576 + 3, ("pcm_peak", 0, 1): 8388608 + 3, ("pcm_peak", 0, 2): 4194304 + 3,
    ("stereo_matrix", 0, 2): 4194304, ("stereo_matrix_scalar", 0, 2): 1048576,
    ("loudness_blocks", 0, 1): 524288, ("loudness_short_term", 0, 1): 524288,
    ("avgpool3s2_fwd", 0, 1): 2097152, ("avgpool3s2_bwd", 1, 1): 2097152, ("nchw_to_nhwc", 0, 1): 2097152,
    ("nhwc_to_nchw", 1, 1): 2097152, ("nchw_cat_to_nhwc", 0, 1): 2097152,
    ("act_bwd", 0, 1): 2097152 * 4, ("act_bwd", 1, 1): 2097152 * 8,
    ("loss_bwd", 0, 1): 524288 * 8 + 7, ("loss_bwd", 1, 1): 524288 * 8 + 7, ("loss_fwd", 0, 1): 262144 * 8 + 7, ("loss_fwd", 1, 1): 262144 * 8 + 7,
    ("adam_step", 0, 1): 4194304, ("adam_step_dev", 0, 1): 4194304, ("adam_step_scaled", 0, 1): 4194304, ("grads_nonfinite", 0, 1): 2097152,
    ("timed_pack_pair", 0, 1): 16777216, ("timed_pack_pair", 1, 1): 16777216,
    ("spectro_encode", 0, 1): 2097152, ("spectro_encode_ex", 0, 1): 2097152, ("spectro_stats", 0, 1): 262144,
    ("spectro_range", 0, 1): 262144 * 4, ("range_fold", 0, 1): 262144 * 4,
    ("spectro_range_scalar", 0, 1): 262144, ("range_fold_scalar", 0, 1): 262144,
}


def test_every_family_is_pinned():
    assert sorted({k[0] for k in LOOPS_ABOVE}) == K.ALL_FAMILIES


@pytest.mark.parametrize("key", sorted(LOOPS_ABOVE), ids=lambda k: f"{k[0]}_{k[1]}_r{k[2]}")
def test_stream_grid_is_todays(key):
    L = _lib().lib()
    family, dtype, rows = key
    edge = LOOPS_ABOVE[key]
    rc, unit, wanted, used = K.stream_grid(L, family, dtype, edge, rows)
    assert rc == 0 and wanted == used, (key, wanted, used)         # at the edge: the whole grid, one trip
    assert K.stream_grid(L, family, dtype, edge, rows) == (0,) + K.expected_grid(family, dtype, edge, rows)
    rc, unit, wanted, used = K.stream_grid(L, family, dtype, edge + (8 if family == "act_bwd" else 1), rows)   # (act_bwd: whole pieces)
    assert rc == 0 and wanted == used + 1, (key, wanted, used)     # one more unit of work: it loops
    for work in (1, 2, 5, 1023, 1025, edge - 1, edge + 1, 3 * edge + 77, 1 << 33):
        assert K.stream_grid(L, family, dtype, work, rows) == (0,) + K.expected_grid(family, dtype, work, rows), (key, work)
    assert K.stream_grid(L, family, dtype, 0, rows) == (0, 0, 0, 0)
    assert K.stream_grid(_lib().lib("f16"), family, dtype, 3 * edge + 77, rows) == (0,) + K.expected_grid(family, dtype, 3 * edge + 77, rows)


def test_caps_in_workgroups():
    """The caps of the table, as the workgroups of a launch far past them."""
    L = _lib().lib()
    caps = {"segments_stitch": 16384, "pcm_decode": 16384, "stereo_matrix": 4096, "stereo_matrix_scalar": 4096, "loudness_blocks": 2048,
            "avgpool3s2_fwd": 8192, "act_bwd": 8192, "nchw_to_nhwc": 8192, "loss_bwd": 2048, "loss_fwd": 1024, "adam_step_scaled": 4096,
            "grads_nonfinite": 2048, "timed_pack_pair": 16384, "spectro_encode": 8192, "spectro_stats": 1024, "spectro_range": 1024}
    for family, cap in caps.items():
        assert K.stream_grid(L, family, 0, 1 << 34)[3] == cap, family
    assert [K.stream_grid(L, "pcm_peak", 0, 1 << 34, c)[3] for c in (1, 2, 3, 8, 2048, 4096)] == [2048, 1024, 682, 256, 1, 1]


def test_stream_grid_refusals():
    L = _lib().lib()
    rc, unit, wanted, used = K.stream_grid(L, "segments_gather", 0, 100)
    assert (rc, wanted, used) == (0, 1, 1) and unit == 1024
    for family in ("", "nope", "limiter", "segments_gathers"):
        rc, unit, wanted, used = K.stream_grid(L, family, 0, 100)
        assert rc == -1 and (unit, wanted, used) == (0, 0, 0) and b"unknown family" in L.p2phd_last_error(), family      # (P2PHD_EINVAL)
    assert K.stream_grid(L, "pcm_decode", 7, 100)[0] != 0 and b"dtype" in L.p2phd_last_error()
    assert K.stream_grid(L, "pcm_decode", 0, -1)[0] != 0 and K.stream_grid(L, "pcm_peak", 0, 100, 0)[0] != 0


# ------------------------------------------------------------------------------------------
# the cases: past two trips, partial last trip; the emulation and its mutants at every case's size
# ------------------------------------------------------------------------------------------
# reducing families: (elements of a piece, pieces in flight per thread and trip with the index clamped to the last piece)
REDUCERS = {"pcm_peak": (4, 4), "grads_nonfinite": (4, 4), "loss_fwd": (None, 4), "range_fold": (4, 1), "range_fold_scalar": (1, 1),
            "spectro_range": (4, 1), "spectro_stats": (1, 1)}


@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_case_is_past_two_trips_and_mutants_show(case):
    """Every case is past two trips of its capped grid with a partial last one.  At the case's size the emulated launch visits every
    element exactly once (which is what 'reproduces the reference' means for a map: test_strided_reproduces_a_map shows the step
    from visits to values on a small grid) and each mutant does not; for the reducing kernels the emulated sum over integer data is
    the sum, and the mutants' is not."""
    cid, family, dtype, rows, _ = case
    work = K.case_work(cid)
    rc, unit, wanted, used = K.stream_grid(_lib().lib(), family, dtype, work, rows)
    assert rc == 0 and used < wanted and work > 2 * unit and work % unit != 0, (cid, work, unit, wanted, used)
    if family not in ("loss_fwd",):                                     # (loss_fwd shares loss_bwd's operands: five of its trips)
        assert work < 3 * unit, (cid, work, unit)
    epp = 8 if dtype == K.H16 else 4
    grid = used
    if family in REDUCERS:
        u, in_flight = REDUCERS[family]
        u = u or epp
        n = work
        assert u == 1 or (n % u != 0 or family == "loss_fwd"), (cid, n, u)      # a scalar tail behind the last whole piece (the losses take whole pieces)
        # integer data: every order of the additions gives the same sum, so only a wrong set of addends differs
        x = (K.index_hash(n, seed=5) >> np.uint32(20)).astype(np.int64) + 1
        want = int(x.sum())
        assert K.strided_sum(x, grid, 256, u, in_flight=in_flight) == want
        if in_flight > 1:                                               # (d): only where a clamped piece is loaded at all
            assert K.strided_sum(x, grid, 256, u, in_flight=in_flight, mutant="clamp") != want
        assert K.strided_sum(x, grid, 256, u, in_flight=in_flight, mutant="reset") != want     # (e)
        return
    per = epp if family == "loss_bwd" else unit // (used * 256)        # (loss_bwd: four pieces in flight are four trips of a piece each)
    if per > 1 and family not in ("act_bwd", "segments_gather_planar", "loss_bwd"):      # (whole pieces / whole quads by their contract)
        assert work % per != 0, (cid, work, per)                       # the last quad / piece is incomplete
    once = K.visits(work, grid, 256, per)
    assert once.min() == 1 and once.max() == 1
    for mutant in ("stride", "one", "tail"):                            # (a), (b), (c)
        if mutant == "stride" and per == 1:
            continue                                                    # (a thread's unit is one element: there is no factor to forget)
        v = K.visits(work, grid, 256, per, mutant)
        assert (v[unit:] != 1).any(), (cid, mutant)                     # it shows beyond the first trip
    # the partial last trip: some threads take one trip more than the others
    trips = np.zeros(grid * 256, dtype=np.int64)
    def tally(lo, hi, t):
        trips[(lo // per) % (grid * 256)] += 1                          # (one run per thread and trip)
    K.strided(tally, work, grid, 256, per)
    assert trips.min() >= 2 and trips.max() == trips.min() + 1


def test_strided_reproduces_a_map():
    """The emulation applied to a map kernel gives the reference at a small grid, and each mutant a different array."""
    work, grid, threads, unit = 2 * 3 * 8 * 4 + 3 * 8 * 2 + 3, 3, 8, 4
    src = K.hashed_floats(work, seed=3)

    def run(mutant):
        out = np.full(work, np.float32(0.7))
        def body(lo, hi, trip):
            for j in range(unit):
                e = lo + j
                e = e[e < hi]
                out[e] = src[e] * np.float32(2)
        K.strided(body, work, grid, threads, unit, mutant)
        return out
    assert np.array_equal(run(None), src * np.float32(2))
    for mutant in ("one", "tail"):
        assert not np.array_equal(run(mutant), src * np.float32(2)), mutant
    assert (K.visits(work, grid, threads, unit, "stride") > 1).any()


def test_hash_identifies_positions():
    h = K.index_hash(1 << 22)
    assert len(np.unique(h)) == 1 << 22                                # a bijection of the index
    x = K.hashed_floats(1 << 22)
    for period in (256, 1024, 4096 * 256, 16384 * 64):
        assert (x[period:] == x[:-period]).mean() < 1e-3               # no period that a grid could have
    assert np.array_equal(K.index_hash(100, start=1000), K.index_hash(1100)[1000:])
    s = K.hashed_small_ints(1 << 16)
    assert s.min() == -64 and s.max() == 63 and np.array_equal(s, np.rint(s))


# ------------------------------------------------------------------------------------------
# the vectorised references against the restatements
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,T,stride", [(1, 8, 8), (100, 16, 12), (1000, 64, 64), (4097, 256, 192), (5000, 100, 75), (777, 33, 17)])
def test_gather_and_stitch_vectorised_are_the_restatements(L, T, stride):
    V = T - stride
    S = max(1, -(-(L - V) // stride))
    audio = K.hashed_floats(L, seed=L)
    seg = K.gather_vec(audio, T, stride, S)
    assert np.array_equal(seg, G.gather(audio, T, stride, S))
    work = K.hashed_floats(S * T, seed=T).reshape(S, T)
    for gain in (1.0, 0.75):
        got = K.stitch_vec(work, stride, gain, L)
        want = G.stitch(work, stride, gain, L)
        # the restatement adds w * cur and (1 - w) * prev as two float64 terms onto 0 and scales: the same value within float64
        # rounding, so the float32 roundings agree except at a float64 tie's width -- compare in float64, then the bits
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24 * max(1.0, np.abs(want).max())
        if V == 0:
            assert np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("case", C.POOL_CASES, ids=lambda c: "n{}_c{}_h{}_w{}".format(*c))
def test_pool_vectorised_are_the_restatements(case):
    N, Cc, H, W = case
    x = torch.randn(N, H, W, (Cc + 7) // 8 * 8, generator=torch.Generator().manual_seed(H * W + Cc))
    want, bound = C.avgpool_fwd_reference(x)
    got, mag = K.avgpool_fwd_vec(x.numpy())
    assert np.array_equal(got, want.numpy()) and np.array_equal(C.POOL_ULPS * C.U32 * mag * C.SMALL, bound.numpy())
    dy = torch.randn(*want.shape, generator=torch.Generator().manual_seed(7))
    want, bound = C.avgpool_bwd_reference(dy, H, W)
    got, mag = K.avgpool_bwd_vec(dy.numpy(), H, W)
    # the same terms in another order of the (at most four) additions: equal within float64 rounding of the magnitude sum
    assert np.abs(got - want.numpy()).max() <= 4 * 2.0 ** -53 * max(1.0, float(mag.max()))
    assert np.abs(C.POOL_ULPS * C.U32 * mag * C.SMALL - bound.numpy()).max() <= 2.0 ** -50 * max(1.0, float(bound.max()))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("kind", [0, 1])
def test_loss_bound_holds_for_the_kernel_order_at_the_long_size(kind, dt):
    """The existing bound of the loss sum grows with the term count; a float32 emulation of loss_fwd_kernel in its own order
    (per-thread accumulators over the trips, shuffle tree, workgroup table, fold) at the size tests/test_gpu_long.py runs stays
    inside it -- the bound is used there unchanged."""
    code = K.F32 if dt == "f32" else K.H16
    P = K.LOSS_P[code]
    a, b = K.loss_operands(P, dt)
    want, bound = C.loss_fwd_reference(kind, a, b, 0.9, K.LOSS_C, 0.5, C.OUT0)
    grid = K.expected_grid("loss_fwd", code, P * K.LOSS_CP)[2]
    got = K.loss_fwd_model32(kind, a.float().numpy(), b.float().numpy(), 0.9, K.LOSS_C, 0.5, C.OUT0, grid, 4 if dt == "f32" else 8)
    print(f"loss_fwd kind {kind} {dt} P {P}: emulation {got!r}, float64 {want!r}, |difference| {abs(float(got) - want):.3e}, bound {bound:.3e}")
    assert abs(float(got) - want) <= bound
