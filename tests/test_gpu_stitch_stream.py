"""The streamed stitch on the GPU (csrc/stitch.hip: p2phd_segments_stitch_stream), through the C ABI and through the wrapper of
generate/ops.py: a clip's segments are stitched window by window -- K segments of every channel per call, the carry of one call
handed to the next -- and the windows' outputs, laid one behind the other, are compared as int32, bit for bit, with
p2phd_segments_stitch_planar on the whole clip.  Outputs and carries sit between canaries, prefilled with a sentinel.  A refused
call launches nothing: the family's counter, the payloads and the canaries stay."""
import ctypes

import pytest
import torch

import _exact as E
import _long as K_

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GAIN = 0.75


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _count():
    return _lib().lib().p2phd_launch_count(b"stitch", 0)


def _vp(p):
    return None if p is None else ctypes.c_void_p(int(p))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _floats(n, seed):
    return torch.from_numpy(K_.hashed_floats(max(n, 1), seed=seed)[:n]).to(DEV)


def _call(seg_ptr, C, K, T, stride, gain, cin, cout, first, out_ptr, ld, n_out):
    L = _lib()
    return L.lib().p2phd_segments_stitch_stream(_vp(seg_ptr), C, K, T, stride, gain, _vp(cin), _vp(cout), first, _vp(out_ptr), ld, n_out,
                                                L.stream_ptr())


def _windows(seg, C, S, T, stride, K, L, shift, what):
    """seg [C * S, T], the whole clip's segments -> the clip [C, L] stitched in windows of K segments through the raw entry.
    `shift` 0: every buffer 16-byte aligned, the pitch a multiple of 4, the last window keeps a carry too.  `shift` 4: the window's
    segments and its output start 4 bytes off the 16-byte grid, the pitch is odd, the last window passes no carry_out."""
    V = T - stride
    got = torch.empty((C, L), dtype=torch.float32, device=DEV)
    carries = [E.Guarded(C * V * 4, DEV, 0xFF), E.Guarded(C * V * 4, DEV, 0xFF)]      # the first call's carry_in is poison (NaN)
    for w, s0 in enumerate(range(0, S, K)):
        Kw = min(K, S - s0)
        last = s0 + Kw == S
        n_out = L - s0 * stride if last else Kw * stride
        ld = (n_out + 3) // 4 * 4 if shift == 0 else (n_out | 1) + 2
        win = E.Guarded(C * Kw * T * 4 + shift, DEV, 0)
        wseg = win.bytes[shift:].view(torch.float32).view(C * Kw, T)
        for c in range(C):
            wseg[c * Kw:(c + 1) * Kw].copy_(seg[c * S + s0:c * S + s0 + Kw])
        out = E.Guarded(((C - 1) * ld + n_out) * 4 + shift, DEV, E.GUARD_BYTE)
        cin, cout = carries[w % 2], carries[(w + 1) % 2]
        keep = not (last and shift)
        before = _count()
        rc = _call(win.ptr() + shift, C, Kw, T, stride, GAIN, cin.ptr(), cout.ptr() if keep else None, 1 if s0 == 0 else 0,
                   out.ptr() + shift, ld, n_out)
        assert rc == 0, (what, w, _lib().lib().p2phd_last_error())
        assert _count() == before + 1
        torch.cuda.synchronize()
        assert not out.touched() and not cin.touched() and not cout.touched() and not win.touched(), (what, w)
        assert bool((out.bytes[:shift] == E.GUARD_BYTE).all())
        rows = out.bytes[shift:].view(torch.float32)
        for c in range(C):
            got[c, s0 * stride:s0 * stride + n_out] = rows[c * ld:c * ld + n_out]
            gap = rows[c * ld + n_out:(c + 1) * ld] if c + 1 < C else rows[:0]
            assert bool((_bits(gap) == -0x5A5A5A5B).all()), (what, w, "the rest of a row is untouched")
        if keep and V:
            want = torch.stack([seg[c * S + s0 + Kw - 1, stride:] for c in range(C)])
            assert torch.equal(_bits(cout.view(torch.float32, (C, V))), _bits(want)), (what, w, "carry_out")
    return got


# ------------------------------------------------------------------------------------------
# windows laid one behind the other are the planar stitch of the whole clip
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["T", "3T/4", "T/2"])
@pytest.mark.parametrize("T", [8, 10, 64])
def test_windows_are_the_planar_stitch_of_the_whole_clip(T, kind):
    """T 8 and 64 with strides that are multiples of 4 take the 16-byte paths where the bases allow, T 10 and the shifted buffers
    the scalar ones.  S x K x C x both ends of the last segment's span, each aligned and 4 bytes off with an odd pitch."""
    from pix2pixhdaudiosr_amd.generate import segments_stitch_planar
    stride = {"T": T, "3T/4": 3 * T // 4, "T/2": T // 2}[kind]
    for S in (1, 2, 3, 7):
        for C in (1, 2):
            seg = _floats(C * S * T, seed=1000 * T + 10 * S + C).reshape(C * S, T)
            for L in ((S - 1) * stride + 1, (S - 1) * stride + T):
                want = segments_stitch_planar(seg, C, stride, GAIN, L)
                for K in sorted({1, 2, 3, S}):
                    for shift in (0, 4):
                        what = (T, stride, S, K, C, L, shift)
                        got = _windows(seg, C, S, T, stride, K, L, shift, what)
                        assert torch.equal(_bits(got), _bits(want)), what


def test_a_window_past_the_cap_behind_a_carry():
    """One window long enough for the grid-stride loop to take a third trip (asked of p2phd_stream_grid, not assumed), as the second
    window of a clip: its first segment fades with the carry, the rest is walked by the loop."""
    from pix2pixhdaudiosr_amd.generate import segments_stitch_planar, segments_stitch_stream
    L = _lib().lib()
    T, stride = 4096, 3072
    unit = K_.stream_grid(L, "segments_stitch_stream", 0, 1 << 30)[1]
    K = -(-(2 * unit + unit // 2 + 1237) // stride)
    n_out = (K - 1) * stride + T - 3
    rc, u, wanted, used = K_.stream_grid(L, "segments_stitch_stream", 0, n_out, 2)
    assert rc == 0 and used < wanted and n_out > 2 * u and u == unit
    S = K + 1
    seg = _floats(2 * S * T, seed=5).reshape(2 * S, T)
    want = segments_stitch_planar(seg, 2, stride, GAIN, stride + n_out)
    carry = torch.stack([seg[c * S, stride:] for c in range(2)]).contiguous()
    win = torch.cat([seg[c * S + 1:(c + 1) * S] for c in range(2)])
    got = segments_stitch_stream(win, 2, stride, GAIN, carry_in=carry, out_length=n_out)
    assert torch.equal(_bits(got), _bits(want[:, stride:]))


def test_stream_grid_of_the_family():
    L = _lib().lib()
    family = "segments_stitch_stream"
    assert K_.stream_grid(L, family, 0, 100) == (0, 1024, 1, 1)
    assert K_.stream_grid(L, family, 0, 1024 * 1024, 2) == (0, 1024 * 1024, 1024, 1024)         # at the edge: one trip
    assert K_.stream_grid(L, family, 0, 1024 * 1024 + 1, 2) == (0, 1024 * 1024, 1025, 1024)     # one more quad: it loops


# ------------------------------------------------------------------------------------------
# the wrapper
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,stride", [(8, 6), (64, 48), (64, 64)])
def test_wrapper_hands_the_carry_from_window_to_window(T, stride):
    from pix2pixhdaudiosr_amd.generate import segments_stitch_planar, segments_stitch_stream
    C, S, K, V = 2, 7, 3, T - stride
    L = (S - 1) * stride + T - 5
    seg = _floats(C * S * T, seed=T + stride).reshape(C * S, T)
    want = segments_stitch_planar(seg, C, stride, GAIN, L)
    carries = [torch.full((C, V), float('nan'), device=DEV), torch.full((C, V), float('nan'), device=DEV)]
    parts = []
    before = _count()
    for w, s0 in enumerate(range(0, S, K)):
        Kw = min(K, S - s0)
        last = s0 + Kw == S
        win = torch.cat([seg[c * S + s0:c * S + s0 + Kw] for c in range(C)])
        parts.append(segments_stitch_stream(win, C, stride, GAIN, carry_in=carries[w % 2], carry_out=None if last else carries[(w + 1) % 2],
                                            first=s0 == 0, out_length=L - s0 * stride if last else None))
    assert _count() == before + 3
    assert torch.equal(_bits(torch.cat(parts, dim=1)), _bits(want))
    with pytest.raises(ValueError, match=r"segments_stitch_stream: expected \[C \* K, T\]"):
        segments_stitch_stream(seg[:-1], C, stride)
    with pytest.raises(ValueError, match=r"segments_stitch_stream: carry_out must be"):
        segments_stitch_stream(seg, C, stride, first=True, carry_out=torch.zeros((C, V + 1), device=DEV))


def test_two_runs_and_a_side_stream_give_the_same_bits():
    from pix2pixhdaudiosr_amd.generate import segments_stitch_stream
    T, stride, C, K = 64, 48, 2, 40
    seg = _floats(C * K * T, seed=11).reshape(C * K, T)
    carry = _floats(C * (T - stride), seed=12).reshape(C, T - stride)

    def run():
        cout = torch.zeros_like(carry)
        return segments_stitch_stream(seg, C, stride, GAIN, carry_in=carry, carry_out=cout), cout

    first, again = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for other in (again, aside):
        assert torch.equal(_bits(other[0]), _bits(first[0])) and torch.equal(_bits(other[1]), _bits(first[1]))


# ------------------------------------------------------------------------------------------
# refusals: on the host, before anything is launched
# ------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing():
    L = _lib().lib()
    C, K, T, stride = 2, 3, 8, 6
    V = T - stride
    n_out = K * stride
    seg = E.Guarded(C * K * T * 4, DEV, E.GUARD_BYTE)
    out = E.Guarded(C * n_out * 4, DEV, E.GUARD_BYTE)
    cin, cout = E.Guarded(C * V * 4, DEV, E.GUARD_BYTE), E.Guarded(C * V * 4, DEV, E.GUARD_BYTE)
    s, o, a, b = seg.ptr(), out.ptr(), cin.ptr(), cout.ptr()
    cases = [("K < 1", (s, C, 0, T, stride, GAIN, a, b, 0, o, n_out, n_out)),
             ("T < 1", (s, C, K, 0, 0, GAIN, a, b, 0, o, n_out, n_out)),
             ("an overlap above T / 2", (s, C, K, T, T // 2 - 1, GAIN, a, b, 0, o, n_out, n_out)),
             ("stride > T", (s, C, K, T, T + 1, GAIN, a, b, 0, o, n_out, n_out)),
             ("C < 1", (s, 0, K, T, stride, GAIN, a, b, 0, o, n_out, n_out)),
             ("C > 65535", (s, 65536, K, T, stride, GAIN, a, b, 0, o, n_out, n_out)),
             ("n_out beyond the span", (s, C, K, T, stride, GAIN, a, b, 0, o, (K - 1) * stride + T + 1, (K - 1) * stride + T + 1)),
             ("n_out < 0", (s, C, K, T, stride, GAIN, a, b, 0, o, n_out, -1)),
             ("ld < n_out", (s, C, K, T, stride, GAIN, a, b, 0, o, n_out - 1, n_out)),
             ("no carry_in behind the first window", (s, C, K, T, stride, GAIN, None, b, 0, o, n_out, n_out)),
             ("carry_out is carry_in", (s, C, K, T, stride, GAIN, a, a, 0, o, n_out, n_out)),
             ("carry_out ends inside carry_in", (s, C, K, T, stride, GAIN, a, a - 4, 0, o, n_out, n_out)),
             ("carry_out inside seg", (s, C, K, T, stride, GAIN, a, s + 4 * (C * K * T - 1), 0, o, n_out, n_out)),
             ("carry_out inside out", (s, C, K, T, stride, GAIN, a, o + 4 * (C * n_out - 1), 1, o, n_out, n_out)),
             ("a null seg", (None, C, K, T, stride, GAIN, a, b, 0, o, n_out, n_out)),
             ("a null out", (s, C, K, T, stride, GAIN, a, b, 0, None, n_out, n_out))]
    before = _count()
    for what, args in cases:
        assert _call(*args) == -1 and L.p2phd_last_error(), what          # (P2PHD_EINVAL)
    assert _call(s, C, K, T, stride, GAIN, a, b, 0, o, 0, 0) == 0         # nothing to write: nothing launched, the carry stays
    torch.cuda.synchronize()
    assert _count() == before
    for g in (seg, out, cin, cout):
        assert not g.touched() and bool((g.bytes == E.GUARD_BYTE).all())
    # and the call as it was meant runs; without an overlap there is no carry, and none is asked for
    assert _call(s, C, K, T, stride, GAIN, a, b, 0, o, n_out, n_out) == 0
    assert _call(s, C, K, T, T, GAIN, None, None, 0, o, n_out, n_out) == 0
    torch.cuda.synchronize()
    assert _count() == before + 2 and not out.touched() and not cout.touched()
