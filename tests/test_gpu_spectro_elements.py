"""p2phd_spectro_encode_ex / p2phd_spectro_decode / p2phd_spectro_decode_signed (csrc/spectro.hip) element by element against
the float64 value of the kernels' own expressions on the same float32 inputs (tests/_transform_ref.py, where the bounds are
derived), at shapes that are no multiple of the 32 x 32 tile, with planted zeros, sub-`min_value` values (the clamp) and
+-1e3; every output in a guarded buffer."""

import numpy as np
import pytest
import torch

import _transform_ref as R
from _exact import assert_bits_equal, check_guards, guarded_like

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(2, 33, 40), (1, 1, 1), (3, 31, 64), (2, 64, 32)]           # (B, F, M)
ALPHA = 0.6
SENTINEL = 0.7


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _report(what, worst):
    print(f"{what}: worst |err| / tol = {worst:.3f}")


def _mask_rows(M):
    return sorted({0, 1, min(M, 2 * (M // 3) + 1), M})                 # none, one, an odd count, all


def _encode(spec, C_, mask_rows, mask_mode, noise, sign, what):
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    B, F, M = spec.shape
    bufs = {}
    bufs["log_spectro"], out = guarded_like((B, C_, M, F), torch.float32, DEV, SENTINEL)
    bufs["pha"], pha = guarded_like((B, 1, M, F), torch.float32, DEV, SENTINEL)
    bufs["norm"], norm = guarded_like((8,), torch.float32, DEV, SENTINEL)
    bufs["partials"], part = guarded_like((int(L.p2phd_spectro_partials_floats(B, F, M)),), torch.float32, DEV, SENTINEL)
    sd, nd, gd = _dev(spec), _dev(noise), _dev(sign)
    _lib.check(L.p2phd_spectro_encode_ex(_lib.ptr(sd), B, F, M, C_, ALPHA, R.MIN_VALUE, mask_rows, mask_mode, _lib.ptr(nd), _lib.ptr(gd),
                                         _lib.ptr(out), _lib.ptr(pha), _lib.ptr(norm), _lib.ptr(part), _lib.stream_ptr()), what)
    torch.cuda.synchronize()
    check_guards(bufs, what)
    return out.cpu().numpy(), pha.cpu(), norm.cpu().numpy()


_ENC_WORST = {}


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("mask_mode", [0, 1, 2])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_encode(shape, channels, mask_mode, with_noise):
    B, F, M = shape
    spec = R.spectro_spec(B, F, M, 7 * F + M)
    for mask_rows in _mask_rows(M):
        rng = np.random.default_rng(1000 * mask_rows + mask_mode)
        noise = sign = None
        if with_noise and mask_rows > 0:
            noise = rng.standard_normal((B, channels, mask_rows, F)).astype(np.float32)
            sign = (2.0 * rng.integers(0, 2, noise.shape) - 1.0).astype(np.float32) if mask_mode == 1 else None
        what = f"spectro_encode {shape} C {channels} mask_rows {mask_rows} mode {mask_mode} noise {with_noise}"
        got, pha, norm = _encode(spec, channels, mask_rows, mask_mode, noise, sign, what)
        ref = R.encode_ref(spec, channels, ALPHA, R.MIN_VALUE, mask_rows, mask_mode, noise, sign)
        keep = ref["keep"]
        assert_bits_equal(pha, torch.from_numpy(ref["pha"]), "flat", what + " pha")
        # norm4: extremes against the float64 dB extremes, mean / std within the derived sum bounds
        for i, name in enumerate(("min", "max", "mean", "std")):
            err, tol = abs(float(norm[i]) - ref["norm"][i]), ref["norm_tol"][i]
            print(f"{what}: {name} got {norm[i]!r} want {ref['norm'][i]!r} |err| / tol = {err / tol if tol else 0.0:.3f}"
                  + (f" (cancellation factor of s2 - count mean^2: {ref['kappa']:.2f})" if name == "std" else ""))
            assert err <= tol, (what, name, float(norm[i]), ref["norm"][i], tol)
        if noise is not None:                                          # the noise statistics: float32 extremes are exact
            assert norm[4] == noise.min() and norm[5] == noise.max(), (what, norm[4:6])
        degenerate = ref["norm"][0] == ref["norm"][1]                  # a single dB value: (d - mn) / 0 is NaN by definition
        if keep > 0:
            worst = R.assert_elements_close(got[:, :, :keep], ref["out"][:, :, :keep], ref["out_tol"][:, :, :keep], what + " kept rows",
                                            ("b", "c", "m", "f"))
            _ENC_WORST["kept"] = max(_ENC_WORST.get("kept", 0.0), worst)
            _report(what + " kept rows", worst)
            if degenerate:
                assert np.isnan(got[:, :, :keep]).all(), what
            else:                                                      # +-1e3 and the clamped values sit in bin 0 / everywhere
                kept = got[:, :, :keep]
                assert kept.min() == 0.0, (what, float(kept.min()))
                assert abs(float(kept.max()) - 1.0) <= 2 * 2.0 ** -23, (what, float(kept.max()))   # 2 ulp(1)
        if mask_rows > 0:
            worst = R.assert_elements_close(got[:, :, keep:], ref["out"][:, :, keep:], ref["out_tol"][:, :, keep:], what + " masked rows",
                                            ("b", "c", "m", "f"))
            _ENC_WORST["masked"] = max(_ENC_WORST.get("masked", 0.0), worst)
            _report(what + " masked rows", worst)
    print("spectro_encode worst so far:", _ENC_WORST)


def _decode_out(B, F, M):
    return guarded_like((B, F, M), torch.float32, DEV, SENTINEL)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode(shape):
    from pix2pixhdaudiosr_amd import _lib
    B, F, M = shape
    x, _, mm = R.decode_operands(B, F, M, 2, 100 * F + M)
    g, out = _decode_out(B, F, M)
    xd, md = _dev(x), _dev(mm)
    what = f"spectro_decode {shape}"
    _lib.check(_lib.lib().p2phd_spectro_decode(_lib.ptr(xd), _lib.ptr(md), B, F, M, ALPHA, R.MIN_VALUE, _lib.ptr(out), _lib.stream_ptr()), what)
    torch.cuda.synchronize()
    check_guards({"spec": g}, what)
    want, tol = R.decode_ref(x, mm, ALPHA, R.MIN_VALUE)
    _report(what, R.assert_elements_close(out.cpu().numpy(), want, tol, what, ("b", "f", "m")))


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode_signed(shape, channels, scale):
    from pix2pixhdaudiosr_amd import _lib
    B, F, M = shape
    x, pha, mm = R.decode_operands(B, F, M, channels, 100 * F + M)
    xd, pd, md = _dev(x), _dev(pha), _dev(mm)
    for keep in sorted({0, M // 3, M}):
        g, out = _decode_out(B, F, M)
        what = f"spectro_decode_signed {shape} C {channels} keep {keep} scale {scale}"
        _lib.check(_lib.lib().p2phd_spectro_decode_signed(_lib.ptr(xd), _lib.ptr(pd), _lib.ptr(md), B, F, M, channels, keep, R.MIN_VALUE,
                                                          scale, _lib.ptr(out), _lib.stream_ptr()), what)
        torch.cuda.synchronize()
        check_guards({"spec": g}, what)
        want, tol, amb = R.decode_signed_ref(x, pha, mm, channels, keep, R.MIN_VALUE, scale)
        assert not amb.any()
        _report(what, R.assert_elements_close(out.cpu().numpy(), want, tol, what, ("b", "f", "m")))


def test_decode_refuses_a_grid_it_cannot_launch():
    """B = 65536 exceeds gridDim.z: p2phd_spectro_decode names itself in the error, like its siblings, and writes nothing."""
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    B = 65536
    x = torch.zeros((B, 2, 1, 1), dtype=torch.float32, device=DEV)
    mm = _dev(np.array([-70.0, 20.0], dtype=np.float32))
    g, out = _decode_out(B, 1, 1)
    rc = L.p2phd_spectro_decode(_lib.ptr(x), _lib.ptr(mm), B, 1, 1, ALPHA, R.MIN_VALUE, _lib.ptr(out), _lib.stream_ptr())
    text = L.p2phd_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "spectro_decode:" in text and "grid too large" in text, (rc, text)
    assert bool((out == SENTINEL).all())
    check_guards({"spec": g}, "spectro_decode grid guard")
    pha = torch.ones((B, 1, 1), dtype=torch.float32, device=DEV)
    rc = L.p2phd_spectro_decode_signed(_lib.ptr(x), _lib.ptr(pha), _lib.ptr(mm), B, 1, 1, 2, 0, R.MIN_VALUE, 1.0, _lib.ptr(out),
                                       _lib.stream_ptr())
    assert rc != 0 and "spectro_decode_signed" in L.p2phd_last_error().decode()
    assert bool((out == SENTINEL).all())
    # the largest batch the guard admits still runs
    g2, out2 = _decode_out(65535, 1, 1)
    _lib.check(L.p2phd_spectro_decode(_lib.ptr(x), _lib.ptr(mm), 65535, 1, 1, ALPHA, R.MIN_VALUE, _lib.ptr(out2), _lib.stream_ptr()), "B 65535")
    torch.cuda.synchronize()
    check_guards({"spec": g2}, "B 65535")
    assert bool((out2 == 0).all())                                     # equal channels: (a0 - a1) inv = 0
