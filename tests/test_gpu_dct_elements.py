"""p2phd_mdct2_fwd / p2phd_mdct2_fwd_frames / p2phd_imdct2_fwd (csrc/dct.hip) and the DCT_2N_native / IDCT_2N_native operators
element by element against the float64 cosine sums of the kernel file's header (tests/_transform_ref.py), with the scale /
k0_scale pairs of the forward calls and of both autograd adjoints (models/mdct.py), every output in a guarded buffer; the
windowed-frame output bit for bit."""
import numpy as np
import pytest
import torch

import _transform_ref as R
from _exact import assert_bits_equal, check_guards, guarded, guarded_like

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WINDOWS = ("ramp", "sine")


def _tables(n_fft):
    from pix2pixhdaudiosr_amd.models.mdct import _DctTables
    return _DctTables.get(n_fft, torch.device(DEV))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fwd(x, w, n_fft, hop, win, start_pad, F, scale, k0, what, frames=None, frames_offset=0):
    """-> out [B, F, n_fft] (and the frames [B, F, win] with frames='yes'); `frames_offset`: bytes the frame buffer is moved
    off its 16-byte alignment."""
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    B, T = x.shape
    xd, wd, tb = _dev(x), _dev(w), _tables(n_fft)
    g, out = guarded_like((B, F, n_fft), torch.float32, DEV)
    bufs = {"out": g}
    if frames is None:
        _lib.check(L.p2phd_mdct2_fwd(_lib.ptr(xd), B, T, n_fft, hop, win, _lib.ptr(wd), _lib.ptr(tb), start_pad, F, scale, k0,
                                     _lib.ptr(out), _lib.stream_ptr()), what)
        fr = None
    else:
        nb = B * F * win * 4
        gf = guarded(nb + frames_offset, DEV, 0)                         # payload: `frames_offset` slack bytes, then the frames
        fr = gf.bytes[frames_offset:].view(torch.float32).view(B, F, win)
        fr.fill_(0.7)
        gf.bytes[:frames_offset].fill_(0xA5)
        bufs["frames"] = gf
        import ctypes as C
        _lib.check(L.p2phd_mdct2_fwd_frames(_lib.ptr(xd), B, T, n_fft, hop, win, _lib.ptr(wd), _lib.ptr(tb), start_pad, F, scale, k0,
                                            _lib.ptr(out), C.c_void_p(gf.ptr() + frames_offset), _lib.stream_ptr()), what)
    torch.cuda.synchronize()
    check_guards(bufs, what)
    if frames is not None:
        assert bool((gf.bytes[:frames_offset] == 0xA5).all()), f"{what}: bytes in front of the offset frame buffer were written"
        return out.cpu().numpy(), fr.cpu()
    return out.cpu().numpy()


def _inv(spec, w, n_fft, hop, win, crop, out_len, scale, k0, what):
    from pix2pixhdaudiosr_amd import _lib
    B, F = spec.shape[:2]
    sd, wd, tb = _dev(spec), _dev(w), _tables(n_fft)
    g, out = guarded_like((B, out_len), torch.float32, DEV)
    _lib.check(_lib.lib().p2phd_imdct2_fwd(_lib.ptr(sd), B, F, n_fft, hop, win, _lib.ptr(wd), _lib.ptr(tb), crop, out_len, scale, k0,
                                           _lib.ptr(out), _lib.stream_ptr()), what)
    torch.cuda.synchronize()
    check_guards({"out": g}, what)
    return out.cpu().numpy()


def _report(what, worst):
    print(f"{what}: worst |err| / tol = {worst:.3f}")


# (n_fft, hop, win, center, B, T): frames per tile 8 / 8 / 4 / 2 / 2; at 2048 two of the four waves run the FFTs.  Frame counts
# off the tile; a hop that is no divisor of the window; win < n_fft (also win % 4 != 0).
GEOMS = [
    (16, 8, 16, True, 3, 83), (64, 32, 64, True, 3, 331), (512, 256, 512, True, 2, 5 * 256 + 7),
    (1024, 512, 1024, True, 2, 4 * 512 - 100), (2048, 1024, 2048, True, 2, 4 * 1024 - 100),
    (64, 24, 64, True, 2, 205), (64, 25, 50, True, 2, 199), (64, 32, 64, False, 2, 32 * 4 + 64), (512, 300, 512, True, 2, 1500),
]


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "n{}_h{}_w{}_c{}_b{}_t{}".format(*[int(v) for v in g]))
def test_forward_inverse_and_adjoint_scales(geom):
    """MDCT2.forward: (scale, k0) = (1, 1); IMDCT2.forward: (0.5, 1); _MDCT2Fn.backward: the inverse kernel with (scale / N, 2 k0);
    _IMDCT2Fn.backward: the forward kernel with (scale N, k0 / 2) = (0.5 N, 0.5)."""
    n_fft, hop, win, center, B, T = geom
    K = R.k_dct(n_fft)
    sp, F = R.forward_layout(B, T, hop, win, center)
    crop, out_len = R.inverse_layout(F, hop, win, center)
    x = R.signal((B, T), 3 * n_fft + hop + T)
    spec = R.signal((B, F, n_fft), 3 * n_fft + hop + T + 1)
    ga = R.signal((B, out_len), 3 * n_fft + hop + T + 2)
    for kind in WINDOWS:
        w = R.window(kind, win, hop)
        tag = f"n_fft {n_fft} hop {hop} win {win} center {center} B {B} T {T} F {F} {kind}"
        for scale, k0, xs, s_pad in ((1.0, 1.0, x, sp), (0.5 * n_fft, 0.5, ga, crop)):
            what = f"mdct2_fwd scale {scale} k0 {k0} {tag}"
            got = _fwd(xs, w, n_fft, hop, win, s_pad, F, scale, k0, what)
            _report(what, R.assert_frames_close(got, R.mdct2_ref(xs, w, n_fft, hop, win, s_pad, F, scale, k0), K, what))
        for scale, k0, c, ol in ((0.5, 1.0, crop, out_len), (1.0 / n_fft, 2.0, sp, T)):
            what = f"imdct2_fwd scale {scale} k0 {k0} crop {c} out_len {ol} {tag}"
            got = _inv(spec, w, n_fft, hop, win, c, ol, scale, k0, what)
            _report(what, R.assert_samples_close(got, R.imdct2_ref(spec, w, n_fft, hop, win, c, ol, scale, k0), K, what, hop))


def test_kbd_window_at_the_shipped_size():
    n_fft, hop, B, T = 1024, 512, 2, 4 * 512 - 100
    w = R.window("kbd", n_fft)
    sp, F = R.forward_layout(B, T, hop, n_fft)
    x = R.signal((B, T), 77)
    got = _fwd(x, w, n_fft, hop, n_fft, sp, F, 1.0, 1.0, "mdct2_fwd kbd")
    _report("mdct2_fwd kbd", R.assert_frames_close(got, R.mdct2_ref(x, w, n_fft, hop, n_fft, sp, F), R.k_dct(n_fft), "mdct2_fwd kbd"))


@pytest.mark.parametrize("n_fft,hop,win,offset", [(64, 32, 64, 0), (2048, 1024, 2048, 0), (64, 25, 50, 0), (64, 32, 64, 4),
                                                  (1024, 512, 1024, 4)])
def test_windowed_frames_bit_for_bit(n_fft, hop, win, offset):
    """`frames` is one float32 product u[n] * w[n] per element: numpy float32 gives the same bits.  float4 route (win % 4 == 0,
    aligned rows), and both scalar routes: win % 4 != 0, and a frame buffer 4 bytes off its alignment.  The spectrum of the
    same launch is held to the bound as well."""
    B, T = 2, 5 * hop - 3
    sp, F = R.forward_layout(B, T, hop, win)
    x = R.signal((B, T), n_fft + win + offset)
    w = R.window("ramp", win, 3)
    what = f"mdct2_fwd_frames n_fft {n_fft} hop {hop} win {win} offset {offset}"
    out, frames = _fwd(x, w, n_fft, hop, win, sp, F, 1.0, 1.0, what, frames="yes", frames_offset=offset)
    want = R.frames_f32(x, w, hop, win, sp, F)
    assert (want != 0).mean() > 0.7
    assert_bits_equal(frames, torch.from_numpy(want), "flat", what)
    _report(what, R.assert_frames_close(out, R.mdct2_ref(x, w, n_fft, hop, win, sp, F), R.k_dct(n_fft), what))


@pytest.mark.parametrize("n_fft", R.N_FFTS_DCT)
def test_dct_operators(n_fft):
    """DCT_2N_native / IDCT_2N_native on [3, 5, N] (15 rows: off every tile), forward and through autograd."""
    from pix2pixhdaudiosr_amd.dct.dct_native import DCT_2N_native, IDCT_2N_native
    K = R.k_dct(n_fft)
    u = R.signal((3, 5, n_fft), 900 + n_fft)
    ud = _dev(u).requires_grad_(True)
    cot = R.signal((3, 5, n_fft), 901 + n_fft)
    y = DCT_2N_native()(ud)
    (gu,) = torch.autograd.grad((y * _dev(cot)).sum(), ud)
    what = f"DCT_2N_native N {n_fft}"
    _report(what, R.assert_frames_close(y.detach().cpu().numpy(), R.dct2_rows(u), K, what))
    # adjoint of X = (2/N) C u with c_0 = 1:  (1/N) (2 g_0 + 2 sum_k>=1 g_k cos) = dct3(g, k0 = 2) / N
    want = R.dct3_rows(cot, 2.0) / n_fft
    norm = np.sqrt((R.dct3_rows(cot, 2.0) ** 2).sum(-1, keepdims=True)) / n_fft
    err = np.abs(gu.cpu().numpy().astype(np.float64) - want) / (K * R.U32 * norm)
    assert err.max() <= 1.0, (what, "backward", float(err.max()))
    _report(what + " backward", float(err.max()))
    z = IDCT_2N_native()(ud)
    (gz,) = torch.autograd.grad((z * _dev(cot)).sum(), ud)
    what = f"IDCT_2N_native N {n_fft}"
    ref = R.dct3_rows(u)
    norm = np.sqrt((ref ** 2).sum(-1, keepdims=True))
    err = np.abs(z.detach().cpu().numpy().astype(np.float64) - ref) / (K * R.U32 * norm)
    assert err.max() <= 1.0, (what, float(err.max()))
    _report(what, float(err.max()))
    # adjoint of y = X_0 + 2 sum X_k cos:  g -> N * dct2(g, k0 = 0.5)
    what += " backward"
    _report(what, R.assert_frames_close(gz.cpu().numpy(), R.dct2_rows(cot, float(n_fft), 0.5), K, what))
