"""csrc/stereo.hip on the GPU: the long-term cross-spectrum of channel pairs against the float64 restatement (tests/_stereo_ref.py)
within a derived bound, its bits (a pair of a call is the call on that pair, a run repeats, a second stream gives the same) and its
degenerate cases; the band sums bit for bit against their numpy restatement on hand-made spectra; the mid/side matrix bit for bit
against numpy float32; every refusal, the launch counter "stereo", and stereo_image on the inputs of tests/test_stereo_host.py."""
import math

import numpy as np
import pytest
import torch

import _stereo_ref as SR
from _bandwidth_ref import frames_ref
from test_gpu_bandwidth import GEOMETRIES, U, _offset_rows, _signal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"stereo", 1 if reset else 0)


def _chunk():
    return _lib().lib().p2phd_ltas_chunk_frames()


# ------------------------------------------------------------------------------------------
# the cross-spectrum
# ------------------------------------------------------------------------------------------
# The bound.  tests/test_gpu_bandwidth.py derives, for the amplitude of one bin of one frame (|X| 4 / n_fft), |a_gpu - a_ref| <= t with
# t = 16 u log2(n) (4 / n) sqrt(n) ||z||_2 (u = 2^-24; Higham's FFT bound, doubled for the window product and for the two real signals
# that share one complex transform) -- here ||z||_2 is the norm of the complex frame the kernel transforms, z = w x_L + i w x_R, so
# ||z||_2 = sqrt(||w x_L||^2 + ||w x_R||^2), the largest over the pair's frames.  The separation hands each of A and B an error of at
# most t (as a complex number, in the scaled units).  With a = |A|, b = |B| in those units:
#   the auto-spectra are that file's case: |P_gpu - P_ref| <= 2 a t + t^2 + 4 u P per frame (_ltas_bound);
#   a cross term is a product of two such numbers: A_gpu conj(B_gpu) - A conj(B) = dA conj(B) + A conj(dB) + dA conj(dB), at most
#   b t + a t + t^2 in modulus, hence in its real and in its imaginary part; the kernel then forms ax bx + ay by (or ay bx - ax by) in
#   fp32 -- two products, one sum, an exact scaling: at most 4 u (|ax bx| + |ay by|) <= 4 u a b by Cauchy-Schwarz (3 roundings and the
#   contraction either way).  So per frame |X_gpu - X_ref| <= a t + b t + t^2 + 4 u a b.
# The float64 sums over F frames add F 2^-53 relative, which disappears in the 4 u.
def _xspec_bound(pair64, n_fft, hop):
    V = SR.frame_values_ref(pair64, n_fft, hop)                                       # [4, F, K]
    t = 16.0 * U * math.log2(n_fft) * (4.0 / n_fft) * math.sqrt(n_fft) * SR.frame_norms_ref(pair64, n_fft, hop).max()
    a, b = np.sqrt(V[0]), np.sqrt(V[1])
    auto = [2.0 * s * t + t * t + 4.0 * U * s * s for s in (a, b)]
    cross = a * t + b * t + t * t + 4.0 * U * a * b
    return V.sum(axis=1), np.stack([auto[0].sum(axis=0), auto[1].sum(axis=0), cross.sum(axis=0), cross.sum(axis=0)])


def _check_xspec(rows_dev, rows_host, n_fft, hop):
    from pix2pixhdaudiosr_amd.generate import cross_spectrum
    before = _count()
    got = cross_spectrum(rows_dev, n_fft, hop)
    assert _count() == before + 1                                                     # exactly one launch a call, whatever G is
    G, L = rows_host.shape[0] // 2, rows_host.shape[1]
    assert tuple(got.shape) == (G, 4, n_fft // 2 + 1) and got.dtype == torch.float64
    again = cross_spectrum(rows_dev, n_fft, hop)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                # the same bits on every run
    g = got.cpu().numpy()
    assert np.isfinite(g).all() and (g[:, :2] >= 0.0).all()
    x64 = rows_host.double().numpy()
    refs, tols = zip(*[_xspec_bound(x64[2 * p:2 * p + 2], n_fft, hop) for p in range(G)])
    ref, tol = np.stack(refs), np.stack(tols)
    ratio = np.abs(g - ref) / tol
    worst = [float(ratio[:, q].max()) for q in range(4)]
    print(f"xspec n_fft {n_fft} hop {hop} G {G} L {L} F {frames_ref(L, n_fft, hop)}: max |S_gpu - S_ref| / bound = "
          f"{worst[0]:.4f} {worst[1]:.4f} {worst[2]:.4f} {worst[3]:.4f} (ll rr re im)")
    assert max(worst) <= 1.0, (n_fft, hop, G, L, worst, np.unravel_index(ratio.argmax(), ratio.shape))
    return got, ref, tol


def _pairs(G, L):
    """G pairs of speech: a shared part and a part of each channel's own, so that no cross term vanishes."""
    rows = []
    for p in range(G):
        common, own = _signal(L, 900 * p), _signal(L, 5000 + 1300 * p)
        rows += [(0.8, -0.5, 0.3)[p] * common + 0.2 * own, 0.4 * common - (0.3, 0.6, 0.1)[p] * own]
    return torch.stack(rows)


@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_xspec_is_within_the_bound_of_float64(n_fft, hop):
    from pix2pixhdaudiosr_amd.generate import cross_spectrum
    lib, chunk = _lib().lib(), _chunk()
    assert chunk == 8
    # (19 chunks and a frame: the folding workgroup takes its partials in batches, two full ones and a rest)
    for F in (1, 2, 7, 8, 9, 17, 19 * chunk + 1):
        L = n_fft + (F - 1) * hop + (hop - 1) // 2                 # not a whole number of hops where the hop allows it
        assert lib.p2phd_ltas_frames(L, n_fft, hop) == F == frames_ref(L, n_fft, hop)
        x = _pairs(3, L)
        got, _, _ = _check_xspec(_offset_rows(x, L + 9), x, n_fft, hop)
        # pair g of the 3-pair call is the 1-pair call (G = 1), bit for bit -- from a buffer of its own, so neither pitch nor alignment matter
        for p in (0, 2):
            one = cross_spectrum(x[2 * p:2 * p + 2].to(DEV), n_fft, hop)
            assert tuple(one.shape) == (1, 4, n_fft // 2 + 1)
            assert torch.equal(one.view(torch.int64)[0], got.view(torch.int64)[p]), (F, p)


def test_xspec_tone_in_both_channels_and_a_second_stream():
    """At the bin of a tone present in both channels (another level, another phase) the bound is a small fraction of each of the
    four sums: it is not vacuous.  The same bits from a second stream."""
    from pix2pixhdaudiosr_amd.generate import cross_spectrum
    n_fft, hop = 512, 256
    F = _chunk() + 3
    L = n_fft + (F - 1) * hop
    t = torch.arange(L, dtype=torch.float64)
    k1 = 50
    noise = 1e-3 * torch.randn((2, L), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    x = (torch.stack([0.5 * torch.sin(2 * torch.pi * k1 * t / n_fft), 0.3 * torch.sin(2 * torch.pi * k1 * t / n_fft + 0.7)]) + noise).float()
    rows = _offset_rows(x, L + 7)
    got, ref, tol = _check_xspec(rows, x, n_fft, hop)
    # amplitudes 0.5 and 0.3, the right channel 0.7 rad ahead: A conj B = 0.15 e^(-0.7 i) per frame
    want = [F * 0.25, F * 0.09, F * 0.15 * math.cos(0.7), -F * 0.15 * math.sin(0.7)]
    for q in range(4):
        assert ref[0, q, k1] == pytest.approx(want[q], rel=2e-2), (q, ref[0, q, k1], want[q])
        assert tol[0, q, k1] < 0.05 * abs(ref[0, q, k1]), (q, tol[0, q, k1], ref[0, q, k1])
        assert abs(float(got[0, q, k1]) / ref[0, q, k1] - 1.0) < 0.05
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = cross_spectrum(rows, n_fft, hop)
    side.synchronize()
    assert torch.equal(other.view(torch.int64), got.view(torch.int64))


def test_xspec_short_clip_is_zeros_and_no_pairs_is_no_launch():
    from pix2pixhdaudiosr_amd.generate import cross_spectrum
    L = _lib()
    _count(reset=True)
    for n_fft, n in ((64, 63), (2048, 2047), (256, 0)):
        xs = cross_spectrum(torch.randn((4, n), device=DEV), n_fft, n_fft // 2)
        assert tuple(xs.shape) == (2, 4, n_fft // 2 + 1) and (xs.view(torch.int64) == 0).all()
    # written, not left: a buffer of NaN comes back as zeros
    out = torch.full((2, 4, 33), float('nan'), dtype=torch.float64, device=DEV)
    x = torch.randn((4, 50), device=DEV)
    assert L.lib().p2phd_xspec(L.ptr(x), 50, 2, 50, 64, 16, None, L.ptr(out), None, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (out.view(torch.int64) == 0).all() and _count() == 0
    # G = 0: nothing launched, nothing touched, whatever the other pointers are
    out.fill_(float('nan'))
    assert L.lib().p2phd_xspec(None, 4096, 0, 4096, 64, 16, None, None, None, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _count() == 0 and torch.isnan(out).all()
    assert L.lib().p2phd_xspec_workspace_bytes(3, 50, 64, 16) == 0 and L.lib().p2phd_xspec_workspace_bytes(0, 4096, 64, 16) == 0
    assert L.lib().p2phd_xspec_workspace_bytes(3, 64 + 16 * 40, 64, 16) == 3 * -(-41 // _chunk()) * 4 * 33 * 8       # 41 frames
    assert L.lib().p2phd_xspec_workspace_bytes(3, 64 + 16 * 40, 64, 16) == 4 * L.lib().p2phd_ltas_workspace_bytes(3, 64 + 16 * 40, 64, 16)


def test_xspec_refusals():
    from pix2pixhdaudiosr_amd.generate import cross_spectrum, stereo_image
    L = _lib()
    lib = L.lib()
    x = torch.zeros((4, 4096), device=DEV)
    out = torch.zeros((2, 4, 2049), dtype=torch.float64, device=DEV)
    tables = torch.zeros((3 * 2048,), device=DEV)
    work = torch.zeros((1 << 21,), dtype=torch.uint8, device=DEV)
    _count(reset=True)

    def call(xp=None, ld=4096, G=2, n=4096, n_fft=64, hop=16, tp=None, op=None, wp=None):
        return lib.p2phd_xspec(L.ptr(x) if xp is None else xp, ld, G, n, n_fft, hop, L.ptr(tables) if tp is None else tp,
                               L.ptr(out) if op is None else op, L.ptr(work) if wp is None else wp, L.stream_ptr())
    for kw, word in ((dict(n_fft=1000), b"n_fft"), (dict(n_fft=32), b"n_fft"), (dict(n_fft=4096), b"n_fft"), (dict(n_fft=0), b"n_fft"),
                     (dict(hop=0), b"hop"), (dict(hop=65), b"hop"), (dict(hop=-1), b"hop"), (dict(G=32768), b"G"), (dict(G=-1), b"G"),
                     (dict(n=-1), b"L"), (dict(ld=4095), b"row pitch"), (dict(xp=L.ptr(x).value + 2), b"aligned"),
                     (dict(op=L.ptr(out).value + 4), b"8 bytes"), (dict(wp=L.ptr(work).value + 4), b"aligned"),
                     (dict(tp=L.ptr(tables).value + 4), b"aligned"), (dict(op=0), b"xs"), (dict(wp=0), b"null"), (dict(tp=0), b"null"),
                     (dict(xp=0), b"null")):
        assert call(**kw) == -1 and word in lib.p2phd_last_error(), (kw, lib.p2phd_last_error())
    assert lib.p2phd_xspec_workspace_bytes(2, 4096, 64, 65) == 0 and b"hop" in lib.p2phd_last_error()
    with pytest.raises(L.P2PHDError, match="n_fft"):
        cross_spectrum(x, 1000, 16)
    with pytest.raises(L.P2PHDError, match="float32"):
        cross_spectrum(x.double(), 64, 16)
    with pytest.raises(ValueError, match=r"\[2 \* G, L\]"):       # an odd row count
        cross_spectrum(x[:3], 64, 16)
    for bad in (x[:3], x, x[:1], x[0]):
        with pytest.raises(ValueError, match=r"waveform \[2, L\]"):
            stereo_image(bad, 48000, 8000)
    with pytest.raises(ValueError, match="must lie in"):
        stereo_image(x[:2], 48000, 96000)
    torch.cuda.synchronize()
    assert _count() == 0 and float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------
# the band sums
# ------------------------------------------------------------------------------------------
def _same_bits(got, want):
    g, w = got.cpu().numpy(), np.asarray(want)
    assert g.shape == w.shape and (g.view(np.int64) == w.view(np.int64)).all(), (g.tolist(), w.tolist())


def _spectra(G, K, seed):
    """Hand-made 'spectra' whose values differ by 2^60 in magnitude, of either sign: a sum taken in another order rounds otherwise."""
    rng = np.random.default_rng(seed)
    return rng.uniform(1.0, 2.0, (G, 4, K)) * 2.0 ** rng.integers(-30, 31, (G, 4, K)) * rng.choice([-1.0, 1.0], (G, 4, K))


@pytest.mark.parametrize("K", [33, 129, 1025])
def test_band_sums_are_the_restatement_bit_for_bit(K):
    from pix2pixhdaudiosr_amd.generate import stereo_bands
    _count(reset=True)
    for i, k_split in enumerate((1, K // 2, K - 1)):
        xs = _spectra(3, K, 10 * K + i)
        want = SR.bands_ref(xs, k_split)
        assert np.isfinite(want).all()
        if K > 256:                                                 # (where a lane has more than one bin, the order shows)
            assert not np.array_equal(want[:, 4:] if k_split == 1 else want[:, :4], (xs[:, :, k_split:] if k_split == 1 else xs[:, :, :k_split]).sum(axis=2))
        _same_bits(stereo_bands(torch.from_numpy(xs).to(DEV), k_split), want)
        # one NaN and one infinity, in either band, each in a row of its own: they go through as IEEE arithmetic leaves them
        for nan_k, inf_k in ((0, K - 1), (K - 1, 0)):
            bad = xs.copy()
            bad[0, 1, nan_k], bad[1, 2, inf_k], bad[2, 0, inf_k], bad[2, 3, nan_k] = np.nan, np.inf, -np.inf, np.nan
            want = SR.bands_ref(bad, k_split)
            assert np.isnan(want).sum() == 2 and np.isinf(want).sum() == 2
            _same_bits(stereo_bands(torch.from_numpy(bad).to(DEV), k_split), want)
    out = torch.full((24,), float('nan'), dtype=torch.float64, device=DEV)
    assert stereo_bands(torch.from_numpy(xs).to(DEV), K - 1, out=out).data_ptr() == out.data_ptr()
    _same_bits(out.view(3, 8), SR.bands_ref(xs, K - 1))
    assert _count() == 3 * 3 + 1                                   # one launch a call, whatever G is


def test_band_sums_refusals():
    from pix2pixhdaudiosr_amd.generate import stereo_bands
    L = _lib()
    lib = L.lib()
    xs = torch.ones((3, 4, 4097), dtype=torch.float64, device=DEV)
    res = torch.zeros((3, 8), dtype=torch.float64, device=DEV)
    _count(reset=True)

    def call(xp=None, G=3, K=33, k_split=16, rp=None):
        return lib.p2phd_stereo_bands(L.ptr(xs) if xp is None else xp, G, K, k_split, L.ptr(res) if rp is None else rp, L.stream_ptr())
    for kw, word in ((dict(K=1), b"K"), (dict(K=4098), b"K"), (dict(k_split=0), b"k_split"), (dict(k_split=33), b"k_split"), (dict(k_split=-1), b"k_split"),
                     (dict(G=-1), b"G"), (dict(xp=0), b"null"), (dict(rp=0), b"null"), (dict(xp=L.ptr(xs).value + 4), b"aligned"),
                     (dict(rp=L.ptr(res).value + 4), b"aligned")):
        assert call(**kw) == -1 and word in lib.p2phd_last_error(), (kw, lib.p2phd_last_error())
    assert call(G=0) == 0 and call(G=0, xp=0, rp=0) == 0
    torch.cuda.synchronize()
    assert _count() == 0 and float(res.abs().max()) == 0.0
    assert call(K=4097, k_split=4096, G=1) == 0 and call(K=2, k_split=1) == 0
    assert _count() == 2
    with pytest.raises(ValueError, match=r"\[G, 4, K\]"):
        stereo_bands(xs[:, :3].contiguous(), 16)
    with pytest.raises(L.P2PHDError, match="float64"):
        stereo_bands(xs.float(), 16)
    with pytest.raises(ValueError, match="out must hold"):
        stereo_bands(xs, 16, out=torch.zeros(8, dtype=torch.float64, device=DEV))
    with pytest.raises(L.P2PHDError, match="k_split"):
        stereo_bands(xs, 4097)


# ------------------------------------------------------------------------------------------
# the matrix
# ------------------------------------------------------------------------------------------
def _same_f32(got, want):
    """Bit for bit, except that the sign and payload of a NaN are nobody's promise (IEEE 754 leaves them open: x - NaN comes back with
    the sign bit set from the device, clear from numpy)."""
    g = got.cpu().numpy()
    return g.shape == want.shape and bool(((g.view(np.int32) == want.view(np.int32)) | (np.isnan(g) & np.isnan(want))).all())


def _matrix_input(L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((2, L), generator=g) * 2.0 ** torch.randint(-20, 4, (2, L), generator=g).float()
    return x


@pytest.mark.parametrize("L", [1, 3, 4, 255, 256, 257, 4099])
def test_matrix_is_numpy_float32_bit_for_bit(L):
    """Out of place and in place (out == x at the same pitch is allowed), at an aligned pitch (float4 path) and at an odd one."""
    from pix2pixhdaudiosr_amd.generate import stereo_matrix
    _count(reset=True)
    calls = 0
    for a in (0.5, 1.0):
        for guard in (False, True):
            x = _matrix_input(L, 31 * L + int(2 * a) + guard)
            if L >= 3:
                x[1, 0], x[1, L // 2], x[1, L - 1] = float('nan'), float('inf'), float('-inf')       # the side row only ...
            if L >= 4:
                x[0, 1] = float('nan')                              # ... and a NaN of the mid row, which survives
            want = SR.matrix_ref(x.numpy(), a, guard)
            if L >= 3:
                assert np.isfinite(want[:, [0, L // 2, L - 1]]).all() == guard and (L < 4 or np.isnan(want[:, 1]).all())
            ld = (L + 3) // 4 * 4 + 4
            aligned = torch.full((2, ld), float('nan'), device=DEV)
            assert aligned.data_ptr() % 16 == 0
            aligned[:, :L] = x.to(DEV)
            for rows in (aligned[:, :L], _offset_rows(x, L + 9)):
                got = stereo_matrix(rows, a, guard_side=guard)
                assert got.data_ptr() != rows.data_ptr() and _same_f32(got, want), (L, a, guard)
                assert stereo_matrix(rows, a, guard_side=guard, out=rows).data_ptr() == rows.data_ptr()
                assert _same_f32(rows, want), (L, a, guard, "in place")
                calls += 2
            assert torch.isnan(aligned[:, L:]).all()                # nothing beyond the row's end is written
    assert _count() == calls


def test_matrix_round_trip_and_refusals():
    from pix2pixhdaudiosr_amd.generate import stereo_matrix
    L = _lib()
    lib = L.lib()
    # operands on the 2^-15 grid: encode then decode returns left and right, as the restatement does
    x = (torch.randint(-32768, 32768, (2, 4099), generator=torch.Generator().manual_seed(6)).float() / 32768.0).to(DEV)
    assert torch.equal(stereo_matrix(stereo_matrix(x, 0.5), 1.0, guard_side=True), x)
    out = torch.zeros((2, 4100), device=DEV)
    _count(reset=True)

    def call(xp=None, ld=4099, n=4099, a=0.5, op=None, ld_out=4100):
        return lib.p2phd_stereo_matrix(L.ptr(x) if xp is None else xp, ld, n, a, 0, L.ptr(out) if op is None else op, ld_out, L.stream_ptr())
    for kw, word in ((dict(n=-1), b"L"), (dict(ld=4098), b"row pitch"), (dict(ld_out=4098), b"row pitch"), (dict(a=float('nan')), b"finite"),
                     (dict(a=float('inf')), b"finite"), (dict(xp=0), b"null"), (dict(op=0), b"null"), (dict(xp=L.ptr(x).value + 2, n=100), b"aligned"),
                     (dict(op=L.ptr(out).value + 2), b"aligned"), (dict(op=L.ptr(x).value + 4, ld_out=4099, n=100), b"overlaps"),
                     (dict(op=L.ptr(x).value, ld_out=4098, n=100, ld=4099), b"overlaps")):
        assert call(**kw) == -1 and word in lib.p2phd_last_error(), (kw, lib.p2phd_last_error())
    assert call(n=0) == 0 and call(n=0, xp=0, op=0) == 0
    torch.cuda.synchronize()
    assert _count() == 0 and float(out.abs().max()) == 0.0
    with pytest.raises(ValueError, match=r"\[2, L\]"):
        stereo_matrix(torch.zeros((3, 8), device=DEV), 0.5)
    with pytest.raises(ValueError, match="shape of x"):
        stereo_matrix(x, 0.5, out=torch.zeros((2, 8), device=DEV))
    with pytest.raises(L.P2PHDError, match="float32"):
        stereo_matrix(x.double(), 0.5)


# ------------------------------------------------------------------------------------------
# both launches in a row
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def premise_inputs():
    return SR.premise_inputs()


@pytest.mark.parametrize("name", ['same', 'inverted', 'half', 'independent', 'partial', 'split'])
def test_stereo_image_on_the_premise_inputs(premise_inputs, name):
    """The restatement meets the input's cap first (a failure there is the input's, not the kernel's); the eight sums are the
    restatement's within the cross-spectrum's bound summed over the band, and every figure lies in the interval that bound leaves it
    (_stereo_ref.figure_intervals).  The caps hold for the device's figures too -- except that a correlation of +-1 within 1e-12
    and a side level of -+inf are float64's: of an fp32 transform they hold within the bound's consequence, which is the interval."""
    from pix2pixhdaudiosr_amd.generate import stereo_figures, stereo_image
    x = premise_inputs[name]
    plan = {'n_fft': SR.N_FFT, 'hop': SR.HOP}
    want_fig, want = SR.image_ref(x, SR.HR, SR.LR, **plan)
    SR.check_premise(name, want_fig)
    k = SR.split_bin_ref(SR.HR, SR.LR, SR.N_FFT)
    _, tol = _xspec_bound(x.astype(np.float64), SR.N_FFT, SR.HOP)
    tol8 = np.concatenate([tol[:, :k].sum(axis=1), tol[:, k:].sum(axis=1)]) * (1.0 + 1e-9)
    _count(reset=True)
    res = stereo_image(torch.from_numpy(x).to(DEV), SR.HR, SR.LR, plan)
    assert _count() == 2 and tuple(res.shape) == (8,) and res.dtype == torch.float64
    got = res.cpu().numpy()
    assert (np.abs(got - want) <= tol8).all(), (got.tolist(), want.tolist(), tol8.tolist())
    fig = stereo_figures(got.tolist())
    box = SR.figure_intervals(want, tol8)
    for band in ('low', 'high'):
        for key, (lo, hi) in box[band].items():
            print(f"{name} {band} {key}: device {fig[band][key]}, restatement {want_fig[band][key]}, interval [{lo}, {hi}]")
            assert fig[band][key] is not None and lo <= fig[band][key] <= hi, (name, band, key, fig[band][key], lo, hi)
    if name in ('same', 'inverted'):
        sign = 1.0 if name == 'same' else -1.0
        for band in ('low', 'high'):
            lo, hi = box[band]['corr']
            assert lo <= sign <= hi and hi - lo < 1e-2              # (the interval is no licence: it holds the cap's value and little else)
    else:
        SR.check_premise(name, fig)
    out = torch.full((8,), float('nan'), dtype=torch.float64, device=DEV)
    assert stereo_image(torch.from_numpy(x).to(DEV), SR.HR, SR.LR, plan, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out.view(torch.int64), res.view(torch.int64))
