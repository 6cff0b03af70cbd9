"""The time-domain crossover on the GPU (csrc/xover.hip: p2phd_xover_fwd; generate.crossover): integer operands against the
float64 restatement bit for bit, float operands inside the worst-case bound of an fp32 dot product, the identities the header
promises, refusals, and what the filter does to two tones.  Every call writes `out` between canaries with a row pitch above L."""
import numpy as np
import pytest
import torch

import _xover_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 1024                                                       # floats on either side of the output
GUARD_BITS = 0x7FC0BEEF                                            # a NaN pattern no kernel writes
TAPS = (1, 3, 63, 255, 1023, 4095)
OFFSETS = ((0, 0, 0), (1, 3, 0), (3, 0, 1), (0, 1, 3), (3, 1, 1))  # floats past a 16-byte boundary: sr, lr, out


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _tile():
    return int(_lib().lib().p2phd_xover_tile_len())


def _placed(a, pitch, off):
    """Rows of `a` [C, L] at `pitch` floats apart, the first one `off` floats past a 16-byte boundary -> (buffer, view of row 0)."""
    C, L = a.shape
    host = np.full(4 + off + C * pitch, np.float32(77.0))
    for c in range(C):
        host[4 + off + c * pitch:4 + off + c * pitch + L] = a[c]
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[4 + off:]


def _call(sr, lr, level, h, offs=(0, 0, 0), pitches=(5, 2, 3), taps=None, h_dev=None):
    """p2phd_xover_fwd on rows placed as asked -> (return code, out [C, L] as numpy or None, canaries and row gaps intact)."""
    L_ = _lib()
    sr, lr = np.ascontiguousarray(sr, dtype=np.float32), np.ascontiguousarray(lr, dtype=np.float32)
    C, L = sr.shape
    ld_sr, ld_lr, ld_out = L + pitches[0], L + pitches[1], L + pitches[2]
    keep_s, s = _placed(sr, ld_sr, offs[0])
    keep_l, l = _placed(lr, ld_lr, offs[1])
    if h_dev is None:
        h_dev = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(DEV)
    n = C * ld_out
    buf = torch.full((GUARD + 4 + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    o0 = GUARD + offs[2]
    out = buf[o0:]
    rc = L_.lib().p2phd_xover_fwd(L_.ptr(s), ld_sr, L_.ptr(l), ld_lr, float(level), L_.ptr(h_dev), h_dev.numel() if taps is None else taps,
                                  C, L, L_.ptr(out), ld_out, L_.stream_ptr())
    torch.cuda.synchronize()
    bits = buf.view(torch.int32).cpu().numpy()
    rows = bits[o0:o0 + n].reshape(C, ld_out) if C else bits[:0].reshape(0, 1)
    intact = bool((bits[:o0] == GUARD_BITS).all() and (bits[o0 + n:] == GUARD_BITS).all() and (rows[:, L:] == GUARD_BITS).all())
    return rc, np.ascontiguousarray(rows[:, :L]).view(np.float32), intact


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------
# 1. exact: every product and partial sum is representable, so there is one right bit pattern per element
# ------------------------------------------------------------------------------------------
def _lengths(taps, T):
    return sorted({L for L in (1, 2, 63, 64, 65, taps - 1, taps, taps + 1, T - 1, T, T + 1, 2 * T + 5, 10007) if L >= 1})


@pytest.mark.parametrize("taps", TAPS)
def test_integer_operands_are_exact(taps):
    """lr, sr integers in [-8, 8], level in {1, 2, 0.5}, taps integers in [-4, 4] / 16, not symmetric: |d| <= 24 in halves,
    products in 1/32, sums below 4095 * 24 / 4 < 2^15 -- 20 bits at most, exact in fp32 whatever the order or contraction."""
    L_ = _lib()
    T = _tile()
    rng = np.random.default_rng(taps)
    h = rng.integers(-4, 5, taps).astype(np.float32) / 16.0
    h[0], h[-1] = 0.25, -0.1875                                    # not symmetric, both ends count
    h_dev = torch.from_numpy(h).to(DEV)
    srm = rng.integers(-8, 9, (3, 10007)).astype(np.float32)
    lrm = rng.integers(-8, 9, (3, 10007)).astype(np.float32)
    case = 0
    for L in _lengths(taps, T):
        for level in (1.0, 2.0, 0.5):
            want = R.xover_ref(srm[:, :L], lrm[:, :L], level, h)
            w32 = want.astype(np.float32)
            assert np.array_equal(w32.astype(np.float64), want)    # the expected values are fp32 numbers
            for C in (1, 2, 3):
                L_.lib().p2phd_launch_count(b"xover", 1)
                rc, got, intact = _call(srm[:C, :L], lrm[:C, :L], level, h, OFFSETS[case % len(OFFSETS)], h_dev=h_dev)
                case += 1
                assert rc == 0 and intact, (L, level, C, rc, intact)
                assert L_.lib().p2phd_launch_count(b"xover", 0) == 1
                bad = np.argwhere(_bits(got) != _bits(w32[:C]))
                assert bad.size == 0, (taps, L, level, C, bad[:4].tolist(), len(bad))


def test_empty_clip_launches_nothing():
    L_ = _lib()
    h = np.array([0.25, 0.5, 0.25], dtype=np.float32)
    L_.lib().p2phd_launch_count(b"xover", 1)
    for C, L in ((2, 0), (0, 5)):
        rc, got, intact = _call(np.zeros((C, L), np.float32), np.zeros((C, L), np.float32), 1.0, h)
        assert rc == 0 and intact and got.size == 0
    # L = 0 with null data pointers is fine too: nothing is looked at
    assert L_.lib().p2phd_xover_fwd(None, 0, None, 0, 1.0, None, 3, 2, 0, None, 0, L_.stream_ptr()) == 0
    assert L_.lib().p2phd_launch_count(b"xover", 0) == 0


# ------------------------------------------------------------------------------------------
# 2. float operands
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", (459, 255, 4095))
def test_float_operands_within_the_dot_product_bound(taps):
    """|out - ref| <= (taps + 8) 2^-24 ((|h| (*) (|level| |lr| + |sr|))[i] + |sr[i]|) for every element: the worst case of an fp32
    dot product of `taps` terms plus the roundings of d and of the last addition (derived; a sequential fp32 evaluation on the
    CPU stays below 0.012 of it)."""
    from pix2pixhdaudiosr_amd.generate import crossover, crossover_coefficients, crossover_plan
    plan = crossover_plan(48000, 12000)
    assert plan[0] == 459
    h = crossover_coefficients(taps, plan[1], plan[2]).numpy()
    rng = np.random.default_rng(100 + taps)
    C, L = 2, 5000
    level = np.float32(np.sqrt(3.0))
    lr = rng.standard_normal((C, L)).astype(np.float32)
    sr = (level * lr + np.float32(0.3) * rng.standard_normal((C, L)).astype(np.float32)).astype(np.float32)
    want = R.xover_ref(sr, lr, level, h)
    bound = (taps + 8) * 2.0 ** -24 * (R.abs_conv_ref(sr, lr, level, h) + np.abs(sr.astype(np.float64)))
    rc, got, intact = _call(sr, lr, level, h, (1, 3, 3))
    assert rc == 0 and intact
    err = np.abs(got.astype(np.float64) - want)
    print(f"taps {taps}: worst error {float((err / bound).max()):.4f} of the bound, largest |error| {err.max():.3e}")
    assert (bound > 0).all() and (err <= bound).all()
    # the Python binding: the same kernel on contiguous tensors
    via = crossover(torch.from_numpy(sr).to(DEV), torch.from_numpy(lr).to(DEV), float(level), torch.from_numpy(h).to(DEV))
    assert tuple(via.shape) == (C, L) and via.is_contiguous() and np.array_equal(_bits(via.cpu().numpy()), _bits(got))


# ------------------------------------------------------------------------------------------
# 3. identities, bit for bit
# ------------------------------------------------------------------------------------------
def _float_rows(seed, C, L):
    rng = np.random.default_rng(seed)
    lr = rng.standard_normal((C, L)).astype(np.float32)
    sr = (np.float32(1.7) * lr + np.float32(0.3) * rng.standard_normal((C, L)).astype(np.float32)).astype(np.float32)
    return sr, lr


def test_no_difference_gives_sr_back():
    from pix2pixhdaudiosr_amd.generate import crossover_coefficients
    T = _tile()
    _, lr = _float_rows(1, 2, T + 77)
    sr = np.float32(2.0) * lr                                      # exact: d = 2 lr - sr = +0 everywhere
    for taps in (1, 255, 459):
        h = crossover_coefficients(taps, 0.11875, 8.96).numpy()
        rc, got, intact = _call(sr, lr, 2.0, h, (3, 1, 1))
        assert rc == 0 and intact and np.array_equal(_bits(got), _bits(sr)), taps


def test_one_tap_is_the_stated_expression():
    """taps = 1: out = sr + fma(h0, d, +0) with d = level * lr - sr as one rounded product and one rounded subtraction; fma(h0, d, 0)
    is the rounded product h0 * d, and d itself for h0 = 1 -- all of it fp32 numpy arithmetic."""
    T = _tile()
    sr, lr = _float_rows(2, 2, 2 * T + 5)
    level = np.float32(np.sqrt(3.0))
    d = (level * lr).astype(np.float32) - sr
    assert d.dtype == np.float32
    for h0 in (1.0, 0.75, -0.3):
        want = sr + (np.float32(h0) * d).astype(np.float32)
        rc, got, intact = _call(sr, lr, level, np.array([h0], dtype=np.float32), (1, 3, 3))
        assert rc == 0 and intact and np.array_equal(_bits(got), _bits(want)), h0


def test_rows_runs_and_pitches_do_not_change_a_bit():
    from pix2pixhdaudiosr_amd.generate import crossover, crossover_coefficients
    T = _tile()
    L = 2 * T + 301
    sr, lr = _float_rows(3, 3, L)
    h = crossover_coefficients(459, 0.11875, 8.96).numpy()
    h[3] += np.float32(1e-3)                                       # the caller's table need not be symmetric
    rc, all3, intact = _call(sr, lr, 1.7, h)
    assert rc == 0 and intact
    for c in range(3):                                             # row c of the 3-row call is the 1-row call on that row
        rc, one, intact = _call(sr[c:c + 1], lr[c:c + 1], 1.7, h, OFFSETS[c + 1])
        assert rc == 0 and intact and np.array_equal(_bits(one[0]), _bits(all3[c])), c
    rc, again, intact = _call(sr, lr, 1.7, h)                      # a run repeats
    assert np.array_equal(_bits(again), _bits(all3))
    rc, moved, intact = _call(sr, lr, 1.7, h, (3, 1, 3), pitches=(1, 64, 9))
    assert rc == 0 and intact and np.array_equal(_bits(moved), _bits(all3))
    # the binding: views with different pitches against contiguous copies
    hd = torch.from_numpy(h).to(DEV)
    s_buf = torch.zeros((3, L + 7), device=DEV)
    l_buf = torch.zeros((3, L + 130), device=DEV)
    s_view, l_view = s_buf[:, 3:3 + L], l_buf[:, 1:1 + L]
    s_view.copy_(torch.from_numpy(sr))
    l_view.copy_(torch.from_numpy(lr))
    assert not s_view.is_contiguous() and s_view.stride(0) != l_view.stride(0)
    a = crossover(s_view, l_view, 1.7, hd)
    b = crossover(s_view.contiguous(), l_view.contiguous(), 1.7, hd)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and np.array_equal(_bits(a.cpu().numpy()), _bits(all3))


# ------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------
def test_refusals():
    L_ = _lib()
    lib = L_.lib()
    C, L, ld = 2, 300, 310
    h = torch.full((9,), 0.1, device=DEV)
    span = (C - 1) * ld + L
    buf = torch.full((4 * GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    sr, lr, out = buf[GUARD:], buf[2 * GUARD:], buf[3 * GUARD:]
    st = L_.stream_ptr()
    einval = lib.p2phd_segments_stitch(None, 0, 0, 0, 1.0, None, 0, st)          # P2PHD_EINVAL of a neighbour
    assert einval != 0
    lib.p2phd_launch_count(b"xover", 1)

    def refused(word, *args):
        rc = lib.p2phd_xover_fwd(*args)
        text = lib.p2phd_last_error().decode()
        assert rc == einval and "xover_fwd" in text and word in text, (word, rc, text)

    p = L_.ptr
    # out aliasing an input: the same pointer, and one element of overlap at either end of the span
    refused("overlaps", p(sr), ld, p(lr), ld, 1.0, p(h), 9, C, L, p(sr), ld, st)
    refused("overlaps", p(sr), ld, p(lr), ld, 1.0, p(h), 9, C, L, p(lr), ld, st)
    refused("overlaps", p(sr), ld, p(lr), ld, 1.0, p(h), 9, C, L, p(sr[span - 1:]), ld, st)
    refused("overlaps", p(sr), ld, p(lr), ld, 1.0, p(h), 9, C, L, p(lr[span - 1:]), ld, st)
    refused("overlaps", p(sr), ld, p(lr), ld, 1.0, p(h), 9, C, L, p(buf[GUARD - span + 1:]), ld, st)
    # touching spans are fine
    assert lib.p2phd_xover_fwd(p(sr), ld, p(sr[span:]), ld, 1.0, p(h), 9, C, L, p(sr[2 * span:]), ld, st) == 0
    torch.cuda.synchronize()
    assert lib.p2phd_launch_count(b"xover", 1) == 1
    buf.view(torch.int32).fill_(GUARD_BITS)
    for taps in (0, 2, 8, 4096, 4097, -1):
        refused("taps", p(sr), ld, p(lr), ld, 1.0, p(h), taps, C, L, p(out), ld, st)
    for args in ((None, ld, p(lr), ld, 1.0, p(h), 9, C, L, p(out), ld, st), (p(sr), ld, None, ld, 1.0, p(h), 9, C, L, p(out), ld, st),
                 (p(sr), ld, p(lr), ld, 1.0, None, 9, C, L, p(out), ld, st), (p(sr), ld, p(lr), ld, 1.0, p(h), 9, C, L, None, ld, st)):
        refused("null pointer", *args)
    refused("pitch", p(sr), L - 1, p(lr), ld, 1.0, p(h), 9, C, L, p(out), ld, st)
    refused("pitch", p(sr), ld, p(lr), ld, 1.0, p(h), 9, C, L, p(out), L - 1, st)
    refused("C", p(sr), ld, p(lr), ld, 1.0, p(h), 9, 65536, L, p(out), ld, st)
    torch.cuda.synchronize()
    assert lib.p2phd_launch_count(b"xover", 0) == 0               # nothing launched
    assert bool((buf.view(torch.int32) == GUARD_BITS).all())      # nothing written
    # the binding's own checks
    from pix2pixhdaudiosr_amd.generate import crossover
    a = torch.zeros((2, 100), device=DEV)
    with pytest.raises(ValueError, match=r"one shape"):
        crossover(a, a[:, :99], 1.0, h)
    with pytest.raises(ValueError, match=r"odd number"):
        crossover(a, a.clone(), 1.0, h[:8])
    with pytest.raises(L_.P2PHDError, match=r"float32 tensor on the GPU"):
        crossover(a.cpu(), a, 1.0, h)
    with pytest.raises(L_.P2PHDError, match=r"rows that are contiguous"):
        crossover(a[:, ::2], a[:, ::2], 1.0, h)


# ------------------------------------------------------------------------------------------
# 5. what the default filter does to a tone on either side
# ------------------------------------------------------------------------------------------
def test_bands():
    """lr = sin(2 pi 1000 t); sr carries the 1 kHz tone at half the level and another phase, plus a 9 kHz tone.  Away from the
    ends the result is level * lr's tone + the 9 kHz tone within 2e-4 (level + 1): the pass-band (1e-4 on a difference of at most
    1.5 level) and stop-band (-85 dB on amplitude 1) bounds of the host test plus the float bound."""
    from pix2pixhdaudiosr_amd.generate import crossover, crossover_coefficients, crossover_plan
    plan = crossover_plan(48000, 12000)
    h = crossover_coefficients(*plan)
    L, c0 = 48000, (plan[0] - 1) // 2
    t = np.arange(L, dtype=np.float64) / 48000.0
    level = 1.5
    lo, hi = np.sin(2 * np.pi * 1000 * t), np.sin(2 * np.pi * 9000 * t)
    lr = lo.astype(np.float32)[None]
    sr = (0.5 * level * np.sin(2 * np.pi * 1000 * t + 0.7) + hi).astype(np.float32)[None]
    rc, got, intact = _call(sr, lr, level, h.numpy(), (0, 1, 3))
    assert rc == 0 and intact
    want = level * lo + hi
    err = np.abs(got[0].astype(np.float64) - want)
    print(f"bands: worst error away from the ends {err[c0:L - c0].max():.3e} (allowed {2e-4 * (level + 1):.3e}), at the ends {err.max():.3e}")
    assert err[c0:L - c0].max() <= 2e-4 * (level + 1)
    via = crossover(torch.from_numpy(sr).to(DEV), torch.from_numpy(lr).to(DEV), level, h.to(DEV))
    assert np.array_equal(_bits(via.cpu().numpy()), _bits(got))
