"""p2phd_timed_pack_pair / p2phd_timed_frames_fwd / p2phd_timed_frames_bwd (csrc/timed.hip) through the C ABI, element by element
against the float64 references and derived bounds of tests/_timed_ref.py, every output in a guarded buffer pre-filled with a
non-integer sentinel; and the wrappers _ops.PackFramePair / _ops.SpectroToFrames.  No element is left out of a comparison.

Worst |err| / tol per case, as this module printed it on the MI355X (gfx950):
  forward (n_fft, B, F)   dense   two-level | backward          forward (n_fft, B, F)   dense   two-level | backward
    16, 3, 17             0.115   0.165     | 0.171               1024, 2, 1            0.024   0.145     | 0.106
    64, 2, 1              0.088   0.128     | 0.149               1024, 2, 8            0.028   0.124     | 0.141
    64, 2, 15             0.082   0.159     | 0.159               1024, 2, 13           0.028   0.143     | 0.123
    64, 2, 16             0.082   0.152     | 0.174               2048, 2, 1            0.018   0.125     | 0.112
    64, 2, 33             0.084   0.178     | 0.197               2048, 2, 4            0.021   0.141     | 0.132
    64, 5, 17             0.084   0.169     | 0.172               2048, 2, 7            0.021   0.139     | 0.106
    512, 2, 16            0.046   0.165     | 0.150               512, 2, 21 kbd        0.032   0.118     | 0.247
    512, 2, 21            0.049   0.161     | 0.144               1024, 2, 13 impulses                    | 0.115
  SpectroToFrames (64, 2, 17): forward 0.083, backward 0.195.
  pack dB, sizes 1 / 3 / 4 / 5 / 1027 / 2x5x64:  f32 0.300 0.300 0.300 0.300 0.730 0.687;  bf16 0.000 0.000 0.000 0.000 0.999 0.998;
  f16 0.000 0.000 0.000 0.000 0.999 0.998.  (Sizes up to 5 hold planted values only: clamped ones and +-1, +-1e3.)
The transforms sit where their float32 emulations sit on the CPU (0.02 .. 0.11 dense, 0.12 .. 0.16 two-level, 0.13 .. 0.21
backward: tests/test_timed_ref_host.py).  The pack's dB mode is above 0.5 by construction, not by a defect: its bound is a sum of
single roundings and one rounding can use its own term up -- the rounding to a 16-bit storage type is up to the half ulp granted
for it (0.999), and in float32 the subtraction's half ulp at d just below -16 is 16 u of the 20 u granted there (0.73 on the
device, 0.75 for the emulation with a correctly rounded log10f).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _companions as K
import _timed_ref as D
import _transform_ref as R
from _exact import check_guards, guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = -1
SENTINEL = 0.7
NAMES3 = ("b", "t", "i")
NAMES4 = ("b", "c", "k", "t")


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L_
    return L_


def _tables(n_fft):
    from pix2pixhdaudiosr_amd.models.mdct import _DctTables
    return _DctTables.get(n_fft, torch.device(DEV))


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)            # a copy: the shared cases are read-only


def _shifted(t, off):
    """A copy of the float32 device tensor whose first byte lies `off` bytes behind a 16-byte boundary."""
    raw = torch.empty(t.numel() * 4 + 32, dtype=torch.uint8, device=DEV)
    s = (-raw.data_ptr()) % 16 + off
    v = raw[s:s + t.numel() * 4].view(torch.float32).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off
    return v


class Out:
    """A guarded float32 output of `shape`, `off` bytes behind the 16-byte aligned start of the payload, sentinel-filled."""

    def __init__(self, shape, off=0, dtype=torch.float32, snapshot=True):
        es = torch.empty((), dtype=dtype).element_size()
        self.off, self.g = off, guarded(int(np.prod(shape)) * es + off, DEV, 0)
        assert self.g.ptr() % 16 == 0
        self.g.bytes[:off].fill_(0xA5)
        self.t = self.g.bytes[off:].view(dtype).view(tuple(shape))
        self.t.fill_(SENTINEL)
        self.before = self.t.clone() if snapshot else None

    def ptr(self):
        return C.c_void_p(self.g.ptr() + self.off)

    def check(self, what):
        check_guards({"out": self.g}, what)
        assert bool((self.g.bytes[:self.off] == 0xA5).all()), f"{what}: bytes in front of the offset buffer were written"

    def intact(self):
        return torch.equal(self.t, self.before)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _report(what, worst):
    print(f"{what}: worst |err| / tol = {worst:.3f}")


def _error_text(L):
    return L.p2phd_last_error().decode("utf-8", "replace")


# ----------------------------------------------------------------------------------------------------------------------
# frames: launchers
# ----------------------------------------------------------------------------------------------------------------------
def _fwd_rc(sr, mm, w, tb, B, F, n_fft, out_ptr, alpha=D.ALPHA, scale=D.SCALE):
    L_ = _lib()
    return L_.lib().p2phd_timed_frames_fwd(L_.ptr(sr), L_.ptr(mm), B, F, n_fft, L_.ptr(w), L_.ptr(tb), alpha, D.MIN_VALUE, scale,
                                           out_ptr, L_.stream_ptr())


def _bwd_rc(g, sr, mm, w, tb, B, F, n_fft, out_ptr, alpha=D.ALPHA, scale=D.SCALE):
    L_ = _lib()
    return L_.lib().p2phd_timed_frames_bwd(L_.ptr(g), L_.ptr(sr), L_.ptr(mm), B, F, n_fft, L_.ptr(w), L_.ptr(tb), alpha, scale, out_ptr,
                                           L_.stream_ptr())


def _fwd(c, what, sr_off=0):
    """One guarded launch of the forward on the case's operands -> the output on the device."""
    B, _, N, F = c["sr"].shape
    sr = _dev(c["sr"]) if sr_off == 0 else _shifted(_dev(c["sr"]), sr_off)
    mm, w = _dev(c["mm"]), _dev(c["w"])
    o = Out((B, F, N))
    _lib().check(_fwd_rc(sr, mm, w, _tables(N), B, F, N, o.ptr(), scale=c["scale"]), what)
    torch.cuda.synchronize()
    o.check(what)
    return o.t


def _bwd(c, what, sr_off=0, g_off=0, out_off=0):
    B, _, N, F = c["sr"].shape
    sr = _dev(c["sr"]) if sr_off == 0 else _shifted(_dev(c["sr"]), sr_off)
    g = _dev(c["g"]) if g_off == 0 else _shifted(_dev(c["g"]), g_off)
    mm, w = _dev(c["mm"]), _dev(c["w"])
    o = Out((B, 2, N, F), out_off)
    _lib().check(_bwd_rc(g, sr, mm, w, _tables(N), B, F, N, o.ptr(), scale=c["scale"]), what)
    torch.cuda.synchronize()
    o.check(what)
    return o.t


def _check_fwd(c, what):
    got = _fwd(c, what)
    again = _fwd(c, what + " (second launch)")
    assert torch.equal(_bits(got), _bits(again)), f"{what}: two launches differ in their bits"
    worst = R.assert_elements_close(got.cpu().numpy(), c["want"], c["tol"], what, NAMES3)
    _report(what, worst)
    return got


def _check_bwd(c, what):
    got = _bwd(c, what)
    again = _bwd(c, what + " (second launch)")
    assert torch.equal(_bits(got), _bits(again)), f"{what}: two launches differ in their bits"
    host = got.cpu().numpy()
    worst = R.assert_elements_close(host, c["want"], c["tol"], what, NAMES4)
    zero = c["sr"] == 0
    assert zero.any() and not host[zero].any(), f"{what}: a gradient at x == 0"
    _report(what, worst)
    return got


# ----------------------------------------------------------------------------------------------------------------------
# frames: the table
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "two_level"])
@pytest.mark.parametrize("geom", D.GEOMS, ids=D.GEOM_IDS)
def test_frames_forward(geom, kind):
    n_fft, B, F = geom
    _check_fwd(D.fwd_case(kind, n_fft, B, F), f"timed_frames_fwd {kind} n_fft {n_fft} B {B} F {F}")


@pytest.mark.parametrize("geom", D.GEOMS, ids=D.GEOM_IDS)
def test_frames_backward(geom):
    n_fft, B, F = geom
    _check_bwd(D.bwd_case(n_fft, B, F), f"timed_frames_bwd n_fft {n_fft} B {B} F {F}")


def test_frames_backward_of_unit_impulses():
    n_fft, B, F = 1024, 2, 13
    _check_bwd(D.bwd_case(n_fft, B, F, True), f"timed_frames_bwd impulses n_fft {n_fft} B {B} F {F}")


def test_frames_with_the_shipped_window_scale_and_range():
    """The KBD window, the generator's scale sqrt(up_ratio - 1) and the low-rate clip's (min, max) of the reference's own step."""
    import os
    from conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, "time_d_step.npz"))
    mm = (float(z["lr_min"]), float(z["lr_max"]))
    n_fft, B, F = 512, 2, 21
    for kind in ("dense", "two_level"):
        _check_fwd(D.fwd_case(kind, n_fft, B, F, "kbd", D.kbd_scale(), mm), f"timed_frames_fwd {kind} kbd n_fft {n_fft} B {B} F {F} mm {mm}")
    _check_bwd(D.bwd_case(n_fft, B, F, False, "kbd", D.kbd_scale(), mm), f"timed_frames_bwd kbd n_fft {n_fft} B {B} F {F} mm {mm}")


@pytest.mark.parametrize("geom", [(64, 2, 33), (2048, 2, 7)], ids=["n64_b2_f33", "n2048_b2_f7"])
def test_frames_alignment_the_header_allows(geom):
    """Only `out` (16 bytes) and `g_frames` (8 bytes) carry an alignment rule: sr and g_sr 4 bytes off a 16-byte boundary and
    g_frames 8 bytes off give the bits of the aligned run."""
    n_fft, B, F = geom
    c = D.fwd_case("dense", n_fft, B, F)
    what = f"timed_frames_fwd n_fft {n_fft} B {B} F {F}"
    assert torch.equal(_bits(_fwd(c, what)), _bits(_fwd(c, what + " sr + 4", sr_off=4)))
    c = D.bwd_case(n_fft, B, F)
    what = f"timed_frames_bwd n_fft {n_fft} B {B} F {F}"
    ref = _bits(_bwd(c, what))
    assert torch.equal(ref, _bits(_bwd(c, what + " sr + 4, g_sr + 4", sr_off=4, out_off=4)))
    assert torch.equal(ref, _bits(_bwd(c, what + " g_frames + 8", g_off=8)))


def test_frames_refusals():
    """EINVAL, every sentinel in place, and an error text that names the entry point."""
    L = _lib().lib()
    n_fft, B, F = 64, 2, 5
    c = D.bwd_case(n_fft, B, F)
    sr, g, mm, w, tb = _dev(c["sr"]), _dev(c["g"]), _dev(c["mm"]), _dev(c["w"]), _tables(n_fft)
    null = C.c_void_p(0)

    def refused(rc, outs, what, name):
        torch.cuda.synchronize()
        text = _error_text(L)
        assert rc == EINVAL and text and name in text, (what, rc, text)
        for o in outs:
            assert o.intact(), f"{what}: the refused call wrote its output"
            o.check(what)

    o = Out((B, F, n_fft), 4)
    refused(_fwd_rc(sr, mm, w, tb, B, F, n_fft, o.ptr()), [o], "out + 4", "timed_frames_fwd")
    o, g4 = Out((B, 2, n_fft, F)), _shifted(g, 4)
    refused(_bwd_rc(g4, sr, mm, w, tb, B, F, n_fft, o.ptr()), [o], "g_frames + 4", "timed_frames_bwd")
    for bad in (8, 48, 4096):                                          # below the range, no power of two, above the range
        of, ob = Out((B, F, n_fft)), Out((B, 2, n_fft, F))
        refused(_fwd_rc(sr, mm, w, tb, 1, 1, bad, of.ptr()), [of], f"n_fft {bad}", "timed_frames_fwd")
        refused(_bwd_rc(g, sr, mm, w, tb, 1, 1, bad, ob.ptr()), [ob], f"n_fft {bad}", "timed_frames_bwd")
    of, ob = Out((B, F, n_fft)), Out((B, 2, n_fft, F))
    refused(_fwd_rc(sr, mm, w, tb, B, F, n_fft, of.ptr(), alpha=0.5), [of], "alpha 0.5", "timed_frames_fwd")
    refused(_bwd_rc(g, sr, mm, w, tb, B, F, n_fft, ob.ptr(), alpha=0.5), [ob], "alpha 0.5", "timed_frames_bwd")
    refused(_fwd_rc(None, mm, w, tb, B, F, n_fft, of.ptr()), [of], "sr null", "timed_frames_fwd")
    refused(_fwd_rc(sr, mm, None, tb, B, F, n_fft, of.ptr()), [of], "window null", "timed_frames_fwd")
    refused(_fwd_rc(sr, mm, w, tb, B, F, n_fft, null), [of], "out null", "timed_frames_fwd")
    refused(_bwd_rc(g, None, mm, w, tb, B, F, n_fft, ob.ptr()), [ob], "sr null", "timed_frames_bwd")
    refused(_bwd_rc(g, sr, mm, w, tb, B, F, n_fft, null), [ob], "g_sr null", "timed_frames_bwd")
    # the buffers the refusals left alone still serve a good call
    _lib().check(_fwd_rc(sr, mm, w, tb, B, F, n_fft, of.ptr()), "after the refusals")
    torch.cuda.synchronize()
    assert not of.intact()


def test_frames_empty_launches():
    L = _lib().lib()
    n_fft = 64
    c = D.bwd_case(n_fft, 2, 5)
    sr, g, mm, w, tb = _dev(c["sr"]), _dev(c["g"]), _dev(c["mm"]), _dev(c["w"]), _tables(n_fft)
    before = int(L.p2phd_launch_count(b"timed_frames", 0))
    for B, F in ((0, 5), (2, 0), (0, 0)):
        of, ob = Out((2, 5, n_fft)), Out((2, 2, n_fft, 5))
        assert _fwd_rc(sr, mm, w, tb, B, F, n_fft, of.ptr()) == 0 and _bwd_rc(g, sr, mm, w, tb, B, F, n_fft, ob.ptr()) == 0
        assert _fwd_rc(None, None, None, None, B, F, n_fft, C.c_void_p(0)) == 0   # nothing to touch: no pointer is looked at
        torch.cuda.synchronize()
        for o in (of, ob):
            assert o.intact()
            o.check(f"empty launch B {B} F {F}")
    assert int(L.p2phd_launch_count(b"timed_frames", 0)) == before


# ----------------------------------------------------------------------------------------------------------------------
# pack pair
# ----------------------------------------------------------------------------------------------------------------------
PACK_SIZES = [(1,), (3,), (4,), (5,), (1027,), (2, 5, 64)]


def _pack_rc(dt, a, b, n, mode_db, min_value, dst_ptr, code=None):
    L_ = _lib()
    dtype = K.DT[dt]
    code = (L_.F32 if dtype == torch.float32 else L_.BF16) if code is None else code
    return L_.lib_for(dtype).p2phd_timed_pack_pair(code, L_.ptr(a), L_.ptr(b), n, mode_db, min_value, dst_ptr, L_.stream_ptr())


def _pack(dt, a, b, mode_db, what, src_off=0, snapshot=True):
    """One guarded launch -> the whole [n, 8] payload on the device."""
    n = a.numel()
    if src_off:
        a, b = _shifted(a, src_off), _shifted(b, src_off)
    o = Out((n, 8), 0, K.DT[dt], snapshot)
    _lib().check(_pack_rc(dt, a, b, n, mode_db, D.MIN_VALUE if mode_db else 0.0, o.ptr()), what)
    torch.cuda.synchronize()
    o.check(what)
    return o.t


@pytest.mark.parametrize("shape", PACK_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_pack_pair(dt, shape):
    """Raw mode: the bits of torch's own cast in channels 0 and 1, +0 in channels 2..7 (the whole payload is compared).  dB mode:
    every element inside its bound.  16-byte aligned sources (four pixels per thread, the tail of the last quad element-wise) and
    sources 4 bytes off (element-wise throughout) give the same bits, as does a second launch."""
    dtype = K.DT[dt]
    n = int(np.prod(shape))
    a, b = D.pack_operands(n, 17 * n + len(dt))
    ad, bd = _dev(a.reshape(shape)), _dev(b.reshape(shape))
    assert ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    what = f"timed_pack_pair raw {dt} {shape}"
    raw = _pack(dt, ad, bd, 0, what)
    want = D.pack_raw_expected(ad, bd, dtype)
    diff = _bits(raw) != _bits(want)
    assert not bool(diff.any()), (what, diff.nonzero()[:8].tolist(), raw[diff][:8].tolist(), want[diff][:8].tolist())
    assert torch.equal(_bits(raw), _bits(_pack(dt, ad, bd, 0, what + " (second launch)")))
    assert torch.equal(_bits(raw), _bits(_pack(dt, ad, bd, 0, what + " sources + 4", src_off=4)))

    what = f"timed_pack_pair dB {dt} {shape}"
    db = _pack(dt, ad, bd, 1, what)
    assert not bool(_bits(db)[:, 2:].any()), f"{what}: a pad channel is not +0"
    ref, tol = D.pack_db_ref(a, b, D.MIN_VALUE, dtype)
    got = db[:, :2].float().cpu().numpy()
    _report(what, R.assert_elements_close(got, ref, tol, what, ("pixel", "channel")))
    clamped = np.stack([np.abs(a) <= np.float32(D.MIN_VALUE), np.abs(b) <= np.float32(D.MIN_VALUE)], axis=-1)
    floor = 20.0 * np.log10(D.MIN_VALUE) - 20.0                       # the planted zeros and sub-min_value inputs sit on the floor
    assert clamped.any() and bool((np.abs(got[clamped] - floor) <= tol[clamped]).all()), (what, got[clamped][:8])
    assert torch.equal(_bits(db), _bits(_pack(dt, ad, bd, 1, what + " (second launch)")))
    assert torch.equal(_bits(db), _bits(_pack(dt, ad, bd, 1, what + " sources + 4", src_off=4)))


def test_pack_pair_grid_stride_loop():
    """The grid is capped at 16384 workgroups of 256 threads, four pixels each: beyond 16384 x 256 quads a thread walks more than
    one.  Raw mode, bf16, compared on the device with torch's own cast."""
    n = 16384 * 256 * 4 + 1027
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = torch.randn(n, generator=gen, device=DEV) * 37.0
    b = torch.randn(n, generator=gen, device=DEV) * 0.011
    got = _bits(_pack("bf16", a, b, 0, "timed_pack_pair grid-stride", snapshot=False))
    assert torch.equal(got[:, 0], _bits(a.to(torch.bfloat16)))
    assert torch.equal(got[:, 1], _bits(b.to(torch.bfloat16)))
    assert not bool(got[:, 2:].any())


def test_pack_pair_refusals_and_empty():
    L_ = _lib()
    n = 8
    a, b = (_dev(v) for v in D.pack_operands(n, 1))
    count = int(L_.lib().p2phd_launch_count(b"timed_pack", 0))

    def refused(rc, o, what, dt="f32"):
        torch.cuda.synchronize()
        text = _error_text(L_.lib_for(K.DT[dt]))
        assert rc == EINVAL and text and "timed_pack_pair" in text, (what, rc, text)
        assert o.intact(), f"{what}: the refused call wrote its output"
        o.check(what)

    o = Out((n, 8), 8)
    refused(_pack_rc("f32", a, b, n, 0, 0.0, o.ptr()), o, "dst + 8")
    o = Out((n, 8))
    refused(_pack_rc("f32", a, b, n, 1, 0.0, o.ptr()), o, "dB with min_value 0")
    refused(_pack_rc("f32", a, b, n, 0, 0.0, o.ptr(), code=2), o, "dtype code 2")
    refused(_pack_rc("f32", a, b, n, 0, 0.0, o.ptr(), code=-1), o, "dtype code -1")
    refused(_pack_rc("f32", None, b, n, 0, 0.0, o.ptr()), o, "lr null")
    refused(_pack_rc("f32", a, None, n, 0, 0.0, o.ptr()), o, "other null")
    refused(_pack_rc("f32", a, b, n, 0, 0.0, C.c_void_p(0)), o, "dst null")
    o16 = Out((n, 8), 0, torch.float16)
    refused(_pack_rc("f16", a, b, n, 1, 0.0, o16.ptr()), o16, "dB with min_value 0, fp16 library", "f16")
    assert _pack_rc("f32", a, b, 0, 0, 0.0, o.ptr()) == 0 and _pack_rc("f32", None, None, 0, 1, D.MIN_VALUE, C.c_void_p(0)) == 0
    torch.cuda.synchronize()
    assert o.intact()
    o.check("n_pixels 0")
    assert int(L_.lib().p2phd_launch_count(b"timed_pack", 0)) == count


# ----------------------------------------------------------------------------------------------------------------------
# the wrappers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("four_d", [False, True], ids=["nfw", "n1fw"])
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_pack_frame_pair_gradient(dt, four_d):
    """The gradient reaches other_frames only and is channel 1 of the cotangent."""
    from pix2pixhdaudiosr_amd import _ops
    dtype = K.DT[dt]
    N, F, W = 2, 5, 64
    a, b = D.pack_operands(N * F * W, 23)
    shape = (N, 1, F, W) if four_d else (N, F, W)
    lr = _dev(a.reshape(shape)).requires_grad_(True)
    other = _dev(b.reshape(shape)).requires_grad_(True)
    out = _ops.PackFramePair.apply(dtype, lr, other)
    assert out.dtype == dtype and tuple(out.shape) == (N, F, W, 8)
    assert torch.equal(_bits(out.detach().reshape(-1, 8)), _bits(D.pack_raw_expected(lr.detach(), other.detach(), dtype)))
    cot = torch.randn((N, F, W, 8), generator=torch.Generator().manual_seed(29)).to(dtype).to(DEV)
    g_lr, g_other = torch.autograd.grad(out, (lr, other), cot, allow_unused=True)
    assert g_lr is None
    assert g_other.dtype == torch.float32 and tuple(g_other.shape) == shape
    assert torch.equal(_bits(g_other.reshape(N, F, W)), _bits(cot[..., 1].float()))


def test_spectro_to_frames_wrapper():
    """A transposed view of sr gives the values and the gradient of its contiguous copy, bit for bit (and inside the bounds); a
    window of the wrong length is refused."""
    from pix2pixhdaudiosr_amd import _lib as L_, _ops
    n_fft, B, F = 64, 2, 17
    c = D.bwd_case(n_fft, B, F)
    f = D.fwd_case("dense", n_fft, B, F)
    assert np.array_equal(c["sr"], f["sr"])
    mm, w, tb, cot = _dev(c["mm"]), _dev(c["w"]), _tables(n_fft), _dev(c["g"])
    base = _dev(c["sr"].transpose(0, 1, 3, 2))                          # [B, 2, F, N] in memory
    outs = []
    for x in (base.transpose(2, 3), base.transpose(2, 3).contiguous()):
        x = x.requires_grad_(True)
        out = _ops.SpectroToFrames.apply(x, mm, w, tb, D.ALPHA, D.MIN_VALUE, c["scale"])
        (gx,) = torch.autograd.grad(out, x, cot)
        assert tuple(gx.shape) == (B, 2, n_fft, F)
        outs.append((x.is_contiguous(), out.detach(), gx))
    assert [o[0] for o in outs] == [False, True]
    assert torch.equal(_bits(outs[0][1]), _bits(outs[1][1])) and torch.equal(_bits(outs[0][2]), _bits(outs[1][2]))
    _report("SpectroToFrames forward", R.assert_elements_close(outs[0][1].cpu().numpy(), f["want"], f["tol"], "SpectroToFrames", NAMES3))
    _report("SpectroToFrames backward", R.assert_elements_close(outs[0][2].cpu().numpy(), c["want"], c["tol"], "SpectroToFrames backward",
                                                                  NAMES4))
    with pytest.raises(L_.P2PHDError):
        _ops.SpectroToFrames.apply(base.transpose(2, 3), mm, w[:-1], tb, D.ALPHA, D.MIN_VALUE, c["scale"])
    with pytest.raises(L_.P2PHDError):
        _ops.SpectroToFrames.apply(base.transpose(2, 3), mm, torch.cat((w, w)), tb, D.ALPHA, D.MIN_VALUE, c["scale"])
