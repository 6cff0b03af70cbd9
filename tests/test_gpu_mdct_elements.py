"""p2phd_mdct4_fwd / p2phd_imdct4_fwd element by element against the float64 cosine sum (tests/_transform_ref.py): the
register-resident kernels of csrc/mdct_fast.hip and the generic LDS kernels of csrc/mdct.hip, under windows that are
nowhere small (`sine`) and asymmetric (`ramp`), in the frame layouts of MDCT4.forward, IMDCT4.forward and both autograd
adjoints -- frames partly and wholly beyond the signal, samples no frame covers -- with every output in a guarded buffer."""
import contextlib

import numpy as np
import pytest
import torch

import _transform_ref as R
from _exact import check_guards, guarded_like

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WINDOWS = ("ramp", "sine")


@contextlib.contextmanager
def _options(**kw):
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    try:
        for k, v in kw.items():
            _lib.check(L.p2phd_set_option(k.encode(), int(v)), k)
        yield
    finally:
        for k in kw:
            _lib.check(L.p2phd_set_option(k.encode(), 0), k)


def _tables(n_fft):
    from pix2pixhdaudiosr_amd.models.mdct import _Tables
    return _Tables.get(n_fft, torch.device(DEV))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fwd(x, w, n_fft, hop, win, start_pad, F, scale, what):
    from pix2pixhdaudiosr_amd import _lib
    B, T = x.shape
    xd, wd, tb = _dev(x), _dev(w), _tables(n_fft)
    g, out = guarded_like((B, F, n_fft // 2), torch.float32, DEV)
    _lib.check(_lib.lib().p2phd_mdct4_fwd(_lib.ptr(xd), B, T, n_fft, hop, win, _lib.ptr(wd), _lib.ptr(tb), start_pad, F, scale,
                                          _lib.ptr(out), _lib.stream_ptr()), what)
    torch.cuda.synchronize()
    check_guards({"out": g}, what)
    return out.cpu().numpy()


def _inv(spec, w, n_fft, hop, win, crop, out_len, scale, what):
    from pix2pixhdaudiosr_amd import _lib
    B, F = spec.shape[:2]
    sd, wd, tb = _dev(spec), _dev(w), _tables(n_fft)
    g, out = guarded_like((B, out_len), torch.float32, DEV)
    _lib.check(_lib.lib().p2phd_imdct4_fwd(_lib.ptr(sd), B, F, n_fft, hop, win, _lib.ptr(wd), _lib.ptr(tb), crop, out_len, scale,
                                           _lib.ptr(out), _lib.stream_ptr()), what)
    torch.cuda.synchronize()
    check_guards({"out": g}, what)
    return out.cpu().numpy()


def _report(what, worst):
    print(f"{what}: worst |err| / tol = {worst:.3f}")


# ----------------------------------------------------------------------------------------------------------------------
# fast kernels: n_fft 1024 / 2048, hop = n_fft / 2, win = n_fft, rows of a multiple of 4 samples
# ----------------------------------------------------------------------------------------------------------------------
B_FAST = 3


def _fast_fwd_cases(hop):
    """(frames, T, start_pad).  1 frame: a wave's dead second frame; 8: a full workgroup tile; 9: one frame past it; 17: three
    tiles.  T = (F - 1) hop - 100 with start_pad = hop is MDCT4.forward on a [3, T] batch (the len(signal) quirk gives F frames:
    asserted), the last frame hangs over the end; start_pad = 0 rows are the adjoint of IMDCT4(center=False, out_length=T)."""
    return [(1, hop - 100, 0), (2, hop - 100, hop), (7, 6 * hop - 100, hop), (8, 7 * hop - 100, hop), (9, 8 * hop - 100, hop),
            (17, 16 * hop - 100, hop), (9, 8 * hop, hop), (17, 14 * hop - 100, 0)]        # the last: frames 14..16 wholly beyond


@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_fast_forward(n_fft, case):
    hop = n_fft // 2
    F, T, sp = _fast_fwd_cases(hop)[case]
    assert T % 4 == 0
    if sp == hop and T % hop:
        assert R.forward_layout(B_FAST, T, hop, n_fft) == (sp, F)
    x = R.signal((B_FAST, T), 100 * case + n_fft)
    for kind in WINDOWS + (("kbd",) if case == 4 else ()):
        w = R.window(kind, n_fft, case)
        ref = R.mdct4_ref(x, w, n_fft, hop, n_fft, sp, F, 1.0)
        if case == 7:
            assert not ref.norms[:, 14:].any()
        for generic in (0, 1):
            with _options(mdct_generic=generic):
                what = f"mdct4_fwd n_fft {n_fft} F {F} T {T} start_pad {sp} {kind} generic {generic}"
                got = _fwd(x, w, n_fft, hop, n_fft, sp, F, 1.0, what)
            _report(what, R.assert_frames_close(got, ref, R.k_mdct4(n_fft), what))


@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_fast_forward_tiles_per_workgroup(n_fft, iters):
    """17 frames = 3 tiles of 8: with 2 tiles per workgroup the second workgroup leaves its loop at the ragged `break`."""
    hop, F = n_fft // 2, 17
    T = 16 * hop - 100
    x = R.signal((B_FAST, T), 555 + n_fft)
    w = R.window("ramp", n_fft, 5)
    ref = R.mdct4_ref(x, w, n_fft, hop, n_fft, hop, F, 0.75)
    with _options(mdct_iters=iters):
        what = f"mdct4_fwd n_fft {n_fft} F 17 mdct_iters {iters}"
        got = _fwd(x, w, n_fft, hop, n_fft, hop, F, 0.75, what)
    _report(what, R.assert_frames_close(got, ref, R.k_mdct4(n_fft), what))


def _fast_inv_cases(hop):
    """(frames, crop, out_len).  crop = hop: IMDCT4.forward (center) -- F = hops + 1; crop = 0: center=False -- F = hops - 1
    (tf0 = -1: the dead first ring slot; 1 hop: no frame at all, every sample uncovered).  8 and 15 hops cross workgroups (7
    hops each): the frame two neighbours share is computed twice.  out_len = 8 hop - 100: out_length = T - 100, also the
    adjoint of MDCT4.forward on [3, 8 hop - 100].  The last case has fewer frames than the output needs: an uncovered tail."""
    cases = []
    for hops in (1, 7, 8, 15):
        cases += [(hops + 1, hop, hops * hop), (hops - 1, 0, hops * hop)]
    cases += [(9, hop, 8 * hop - 100), (7, 0, 8 * hop - 100), (5, 0, 8 * hop)]
    return cases


@pytest.mark.parametrize("case", range(11))
@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_fast_inverse(n_fft, case):
    hop = n_fft // 2
    F, crop, out_len = _fast_inv_cases(hop)[case]
    spec = R.signal((B_FAST, F, hop), 200 * case + n_fft)
    scale = 4.0 / n_fft
    for kind in WINDOWS + (("kbd",) if case == 8 else ()):
        w = R.window(kind, n_fft, case)
        ref = R.imdct4_ref(spec, w, n_fft, hop, n_fft, crop, out_len, scale)
        if case == 10:
            assert ref.covered[:6 * hop].all() and not ref.covered[6 * hop:].any()
        for generic in (0, 1):
            with _options(mdct_generic=generic):
                what = f"imdct4_fwd n_fft {n_fft} F {F} crop {crop} out_len {out_len} {kind} generic {generic}"
                got = _inv(spec, w, n_fft, hop, n_fft, crop, out_len, scale, what)
            _report(what, R.assert_samples_close(got, ref, R.k_mdct4(n_fft), what, hop))


# ----------------------------------------------------------------------------------------------------------------------
# generic kernels
# ----------------------------------------------------------------------------------------------------------------------
# (n_fft, hop, win, center, B, T).  Q = n_fft / 4 = 4, 8, 16, 32, 128, 1024: radix-4 only / + the final radix-2 / idle lanes /
# more than 64 points per wave / the 120 KiB LDS path with 2 frames per tile.  Frame counts off the tile of 8 and off 4 waves.
GENERIC = [
    (16, 8, 16, True, 3, 83), (32, 16, 32, True, 3, 165), (64, 32, 64, True, 3, 331), (128, 64, 128, True, 3, 650),
    (512, 256, 512, True, 3, 5 * 256 + 7), (4096, 2048, 4096, True, 2, 4 * 2048 - 100),
    (64, 16, 64, True, 2, 150),             # hop = win / 4: four frames per sample
    (64, 24, 64, True, 2, 205),             # hop no divisor of win
    (64, 64, 64, True, 2, 300),             # hop = win: no overlap
    (64, 24, 48, True, 2, 199),             # win < n_fft
    (64, 32, 64, False, 2, 32 * 4 + 64),    # center False: 5 frames
    (64, 32, 64, True, 2, 32 * 10 - 1),     # 11 frames
    (1024, 512, 1024, True, 2, 5 * 512 + 3),  # T % 4 != 0: not eligible for the fast kernels
]


@pytest.mark.parametrize("geom", GENERIC, ids=lambda g: "n{}_h{}_w{}_c{}_b{}_t{}".format(*[int(v) for v in g]))
def test_generic_forward_inverse_and_adjoint_layouts(geom):
    n_fft, hop, win, center, B, T = geom
    K = R.k_mdct4(n_fft)
    sp, F = R.forward_layout(B, T, hop, win, center)
    assert F <= 6 or n_fft < 4096
    x = R.signal((B, T), n_fft + hop + T)
    spec = R.signal((B, F, n_fft // 2), n_fft + hop + T + 1)
    crop, out_len = R.inverse_layout(F, hop, win, center)
    for kind in WINDOWS:
        w = R.window(kind, win, hop)
        tag = f"n_fft {n_fft} hop {hop} win {win} center {center} B {B} T {T} F {F} {kind}"
        got = _fwd(x, w, n_fft, hop, win, sp, F, 1.0, "mdct4_fwd " + tag)
        _report("mdct4_fwd " + tag, R.assert_frames_close(got, R.mdct4_ref(x, w, n_fft, hop, win, sp, F, 1.0), K, "mdct4_fwd " + tag))
        got = _inv(spec, w, n_fft, hop, win, crop, out_len, 4.0 / n_fft, "imdct4_fwd " + tag)
        _report("imdct4_fwd " + tag, R.assert_samples_close(got, R.imdct4_ref(spec, w, n_fft, hop, win, crop, out_len, 4.0 / n_fft), K,
                                                           "imdct4_fwd " + tag, hop))
        # _MDCT4Fn.backward: the inverse kernel on the forward's layout; _IMDCT4Fn.backward: the forward kernel on the inverse's
        got = _inv(spec, w, n_fft, hop, win, sp, T, 1.0, "mdct4 adjoint " + tag)
        _report("mdct4 adjoint " + tag, R.assert_samples_close(got, R.imdct4_ref(spec, w, n_fft, hop, win, sp, T, 1.0), K,
                                                              "mdct4 adjoint " + tag, hop))
        ga = R.signal((B, out_len), n_fft + hop + T + 2)
        got = _fwd(ga, w, n_fft, hop, win, crop, F, 4.0 / n_fft, "imdct4 adjoint " + tag)
        _report("imdct4 adjoint " + tag, R.assert_frames_close(got, R.mdct4_ref(ga, w, n_fft, hop, win, crop, F, 4.0 / n_fft), K,
                                                               "imdct4 adjoint " + tag))


# ----------------------------------------------------------------------------------------------------------------------
# impulses
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,generic", [(64, 0), (1024, 0), (1024, 1)])
def test_impulses(n_fft, generic):
    """Rows of one unit sample at 0, 1, hop-1, hop, hop+1, T-1: a frame that does not cover the impulse is zero exactly (the
    comparison demands it of every frame whose reference is zero), a covered one is the window value times one cosine row."""
    hop = n_fft // 2
    T = 5 * hop - 100 if n_fft == 1024 else 5 * hop - 4
    x, pos = R.impulses(T, hop)
    sp, F = R.forward_layout(len(pos), T, hop, n_fft)
    w = R.window("ramp", n_fft, 9)
    ref = R.mdct4_ref(x, w, n_fft, hop, n_fft, sp, F, 1.0)
    for r, p in enumerate(pos):                                          # the reference itself: exactly the covering frames are live
        live = [t for t in range(F) if 0 <= p - (t * hop - sp) < n_fft]
        assert sorted(np.nonzero(ref.norms[r])[0].tolist()) == live and len(live) == 2
    with _options(mdct_generic=generic):
        what = f"mdct4_fwd impulses n_fft {n_fft} generic {generic}"
        got = _fwd(x, w, n_fft, hop, n_fft, sp, F, 1.0, what)
    _report(what, R.assert_frames_close(got, ref, R.k_mdct4(n_fft), what))
