"""Per-element checks of the MDCT4 / MDCT2 / DCT and spectrogram-codec kernels: operands, float64 references by direct
definition, measured error constants and comparison functions.

Why not `conftest.rel_err` with a KBD window.  A relative L2 norm over a whole tensor at 1e-4 leaves about 800 x of slack
over what fp32 arithmetic needs: an error in one bin, one frame or one tile seam hides in it.  And the shipped KBD window is
below 1e-4 on 9.5 % of its positions (both frame edges) and symmetric: a wrong index at a frame edge, or `w[N-1-n]` read
for `w[n]`, is numerically invisible under it.  So the operands here are
  * `sine`  0.35 + 0.65 sin(pi (n + 1/2) / N): symmetric like the shipped windows, but nowhere small;
  * `ramp`  0.5 + (n + rho[n]) / N, rho seeded in [0.1, 0.9]: strictly increasing, so w[n] != w[N-1-n] for every n, in [0.5, 1.5];
  * `kbd`   the shipped window (one case per family ties the tests back to the shipped configuration);
  * signals dense in [-1, 1] (uniform), and unit impulses,
and every element is compared against a bound that scales with its own frame:
  frames   |got[b,t,k] - ref[b,t,k]| <= K U32 ||ref[b,t,:]||_2
  samples  |got[b,m]   - ref[b,m]|   <= K U32 |scale| sum_{t covers m} |w[q]| ||y_t||_2      (y_t: float64 inverse frame)
A frame whose reference is identically zero, and a sample no frame covers, must be zero exactly (the sign of a zero is not
compared, as in _exact.py: -0.f - 0.f is -0.f).

K is MEASURED ON THE CPU AGAINST THE REFERENCE'S ALGORITHM, never against the kernels (`measure_k_*`): a complex64 / float32
run of the reference's own transform (window, rotate, torch.fft.fft, rotate -- oracle/mdct4.py in complex128; zero-pad, rfft,
twiddle -- oracle/mdct2.py) against the direct float64 cosine sum gives max |err| / (U32 ||frame||_2); K is 8 x the worst of
those ratios, rounded up to the next integer.  The factor 8 is for the kernels' other factorisation (an N/4-point radix-4
FFT between two rotations from fp32 tables for the MDCT, an N-point one behind Makhoul's reordering for the DCT): both obey
the same O(log2 N) u ||.||_2 bound.  K must stay below the derived ceiling 5 log2(n_fft) + 10 (Higham's FFT bound plus the
window, the two rotations, the scale and the overlap-add roundings).  tests/test_transform_ref_host.py re-measures the ratios
and holds the tables below to both conditions.

This module is a plain helper (no fixtures, no test functions).
"""
import functools
import math

import numpy as np
import torch

from oracle import mdct4 as O4
from _exact import U32, _hist

N_FFTS_MDCT4 = (16, 32, 64, 128, 512, 1024, 2048, 4096)
N_FFTS_DCT = (16, 64, 512, 1024, 2048)

# n_fft: (measured forward ratio, measured inverse ratio, K) -- sine window, uniform input, seeds 0..2 (measure_k_mdct4)
K_MDCT4_TABLE = {
    16: (1.712, 1.524, 14.0),
    32: (1.810, 1.279, 15.0),
    64: (1.155, 0.831, 10.0),
    128: (1.235, 0.672, 10.0),
    512: (0.643, 0.462, 6.0),
    1024: (0.474, 0.395, 4.0),
    2048: (0.488, 0.305, 4.0),
    4096: (0.261, 0.190, 3.0),
}
# n_fft: (measured DCT-II ratio, measured DCT-III ratio, K) (measure_k_dct)
K_DCT_TABLE = {
    16: (1.938, 1.062, 16.0),
    64: (1.066, 0.873, 9.0),
    512: (0.421, 0.417, 4.0),
    1024: (0.457, 0.316, 4.0),
    2048: (0.270, 0.244, 3.0),
}


def k_ceiling(n_fft):
    return 5.0 * math.log2(n_fft) + 10.0


def k_mdct4(n_fft):
    return K_MDCT4_TABLE[n_fft][2]


def k_dct(n_fft):
    return K_DCT_TABLE[n_fft][2]


# ----------------------------------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------------------------------
def window(kind, n, seed=0):
    """float32 window of length n (module docstring)."""
    i = np.arange(n, dtype=np.float64)
    if kind == "sine":
        w = 0.35 + 0.65 * np.sin(np.pi * (i + 0.5) / n)
    elif kind == "ramp":
        rho = np.random.default_rng(1000 + seed).uniform(0.1, 0.9, n)
        w = 0.5 + (i + rho) / n
    elif kind == "kbd":
        assert n % 2 == 0
        return O4.kbdwin(n)
    elif kind == "ones":
        w = np.ones(n)
    else:
        raise ValueError(kind)
    return w.astype(np.float32)


def signal(shape, seed):
    """float32, uniform in [-1, 1]."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def impulses(T, hop):
    """One row per unit impulse at 0, 1, hop-1, hop, hop+1, T-1 -> (x [6, T] float32, positions)."""
    pos = [0, 1, hop - 1, hop, hop + 1, T - 1]
    x = np.zeros((len(pos), T), dtype=np.float32)
    for r, p in enumerate(pos):
        x[r, p] = 1.0
    return x, pos


# ----------------------------------------------------------------------------------------------------------------------
# float64 references by direct definition
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def cos4(n_fft):
    """[n, k] = cos(2 pi / N (n + 1/2 + N/4)(k + 1/2)): the MDCT4 kernel of oracle.mdct4 (direct form)."""
    return O4._cos_kernel(n_fft)


@functools.lru_cache(maxsize=2)
def cos2(n_fft):
    """[i, k] = cos(pi (2 i + 1) k / 2N): the DCT-II / DCT-III kernel of the header of csrc/dct.hip."""
    i = np.arange(n_fft, dtype=np.float64)[:, None]
    k = np.arange(n_fft, dtype=np.float64)[None, :]
    return np.cos(np.pi * (2 * i + 1) * k / (2 * n_fft))


def gather_frames(x, hop, win, start_pad, n_frames, dtype=np.float64):
    """[B, F, win]: frame t holds x[t hop - start_pad + n], zero outside [0, T) -- the entry points' explicit layout."""
    x = np.asarray(x, dtype=dtype)
    B, T = x.shape
    idx = np.arange(n_frames)[:, None] * hop - start_pad + np.arange(win)[None, :]
    ok = (idx >= 0) & (idx < T)
    if T == 0 or n_frames == 0:
        return np.zeros((B, n_frames, win), dtype=dtype)
    return np.where(ok[None], x[:, np.clip(idx, 0, T - 1)], dtype(0))


def forward_layout(B, T, hop, win, center=True):
    """(start_pad, n_frames) of MDCT4.forward / MDCT2.forward on a [B, T] batch: oracle.mdct4.frame_layout, with its
    `len(signal)` quirk (the padding is derived from the batch size)."""
    start_pad, _, n_frames = O4.frame_layout((B, T), hop, win, center)
    return start_pad, n_frames


def inverse_layout(F, hop, win, center=True, out_length=None):
    """(crop, out_len) of IMDCT4.forward / IMDCT2.forward on F frames (oracle.mdct4.imdct4_forward :94-102)."""
    full = (F - 1) * hop + win
    crop, out_len = (win // 2, max(full - 2 * (win // 2), 0)) if center else (0, full)
    if out_length is not None:
        out_len = min(out_len, int(out_length))
    return crop, out_len


class FramesRef:
    """out [B, F, L] float64, frames: the windowed frames [B, F, n_fft] (zero beyond win), norms [B, F] = ||out[b, t, :]||_2."""

    def __init__(self, out, frames):
        self.out, self.frames = out, frames
        self.norms = np.sqrt((out * out).sum(-1))


class SamplesRef:
    """out [B, out_len] float64; y [B, F, n_fft]: un-windowed, un-scaled inverse frames; ynorm [B, F]; tol1 [B, out_len] =
    |scale| sum_{t covers m} |w[q]| ||y_t||_2 (the tolerance for K U32 = 1); covered [out_len]: some frame covers the sample."""

    def __init__(self, out, y, ynorm, tol1, covered):
        self.out, self.y, self.ynorm, self.tol1, self.covered = out, y, ynorm, tol1, covered


def _windowed(x, w, n_fft, hop, win, start_pad, n_frames):
    fr = gather_frames(x, hop, win, start_pad, n_frames) * np.asarray(w, dtype=np.float64)
    if n_fft > win:
        fr = np.pad(fr, [(0, 0), (0, 0), (0, n_fft - win)])
    return fr


def _ola(y, w, hop, win, crop, out_len, scale):
    """Overlap-add of the inverse frames y [B, F, >= win]: out[m] = scale sum_t w[q] y_t[q], q = m + crop - t hop in [0, win)."""
    B, F = y.shape[:2]
    w = np.asarray(w, dtype=np.float64)
    ynorm = np.sqrt((y * y).sum(-1))
    full_len = max((F - 1) * hop + win if F else 0, crop + out_len)
    full = np.zeros((B, full_len))
    tol = np.zeros((B, full_len))
    cover = np.zeros(full_len, dtype=np.int64)
    for t in range(F):
        full[:, t * hop: t * hop + win] += w * y[:, t, :win]
        tol[:, t * hop: t * hop + win] += np.abs(w)[None, :] * ynorm[:, t, None]
        cover[t * hop: t * hop + win] += 1
    s = float(np.float32(scale))
    sl = slice(crop, crop + out_len)
    return SamplesRef(s * full[:, sl], y, ynorm, abs(s) * tol[:, sl], cover[sl] > 0)


def mdct4_ref(x, w, n_fft, hop, win, start_pad, n_frames, scale=1.0):
    """p2phd_mdct4_fwd: S[b, t, k] = scale sum_n u_t[n] cos(2 pi / N (n + 1/2 + N/4)(k + 1/2)), u_t = window * frame."""
    fr = _windowed(x, w, n_fft, hop, win, start_pad, n_frames)
    return FramesRef(float(np.float32(scale)) * (fr @ cos4(n_fft)), fr)


def imdct4_ref(spec, w, n_fft, hop, win, crop, out_len, scale):
    """p2phd_imdct4_fwd: y_t = C S_t (the adjoint core), out[m] = scale sum_t w[q] y_t[q]."""
    spec = np.asarray(spec, dtype=np.float64)
    y = spec @ cos4(n_fft).T if spec.shape[1] else np.zeros((spec.shape[0], 0, n_fft))
    return _ola(y, w, hop, win, crop, out_len, scale)


def dct2_rows(u, scale=1.0, k0_scale=1.0):
    """X[k] = scale c_k (2/N) sum_i u[i] cos(pi (2i+1) k / 2N), c_0 = k0_scale (csrc/dct.hip header)."""
    u = np.asarray(u, dtype=np.float64)
    N = u.shape[-1]
    X = float(np.float32(scale)) * (2.0 / N) * (u @ cos2(N))
    X[..., 0] *= float(np.float32(k0_scale))
    return X


def dct3_rows(X, k0_scale=1.0):
    """y[i] = k0_scale X[0] + 2 sum_{k>=1} X[k] cos(pi (2i+1) k / 2N) (csrc/dct.hip header, without `scale`)."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[-1]
    Xp = 2.0 * X
    Xp[..., 0] = float(np.float32(k0_scale)) * X[..., 0]
    return Xp @ cos2(N).T


def mdct2_ref(x, w, n_fft, hop, win, start_pad, n_frames, scale=1.0, k0_scale=1.0):
    fr = _windowed(x, w, n_fft, hop, win, start_pad, n_frames)
    return FramesRef(dct2_rows(fr, scale, k0_scale), fr)


def imdct2_ref(spec, w, n_fft, hop, win, crop, out_len, scale, k0_scale=1.0):
    spec = np.asarray(spec, dtype=np.float64)
    y = dct3_rows(spec, k0_scale) if spec.shape[1] else np.zeros((spec.shape[0], 0, n_fft))
    return _ola(y, w, hop, win, crop, out_len, scale)


def frames_f32(x, w, hop, win, start_pad, n_frames):
    """The `frames` output of p2phd_mdct2_fwd_frames: ONE float32 product u[n] * w[n] per element -- bit-exact in numpy float32."""
    return gather_frames(x, hop, win, start_pad, n_frames, dtype=np.float32) * np.asarray(w, dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# K: float32 models of the reference's algorithm against the direct form
# ----------------------------------------------------------------------------------------------------------------------
def _c64(a):
    return torch.from_numpy(np.asarray(a).astype(np.complex64))


def mdct4_model32(frames32, n_fft):
    """oracle.mdct4.mdct4_forward :67-76 in complex64 on float32 windowed frames [.., n_fft]."""
    n = np.arange(n_fft, dtype=np.float64)
    exp1 = _c64(np.exp(-1j * np.pi / n_fft * n))
    k2 = np.arange(1, n_fft, 2, dtype=np.float64)
    exp2 = _c64(np.exp(-1j * (np.pi / (2 * n_fft) + np.pi / 4) * k2))
    s1 = torch.from_numpy(np.asarray(frames32, dtype=np.float32)).to(torch.complex64) * exp1
    s3 = exp2 * torch.fft.fft(s1, dim=-1)[..., : n_fft // 2]
    return s3.real.numpy()


def imdct4_model32(spec32, n_fft):
    """oracle.mdct4.imdct4_forward :83-89 in complex64: the un-windowed inverse frames [.., n_fft]."""
    k2 = np.arange(1, n_fft, 2, dtype=np.float64)
    exp1 = _c64(np.exp(-1j * (np.pi / (2 * n_fft) + np.pi / 4) * k2))
    n2 = np.arange(0, 2 * n_fft, 2, dtype=np.float64)
    exp2 = _c64(np.exp(-1j * np.pi / (2 * n_fft) * n2))
    s = exp1 * torch.from_numpy(np.asarray(spec32, dtype=np.float32)).to(torch.complex64)
    s = torch.fft.fft(s, n=n_fft, dim=-1)
    return (s * exp2).real.numpy()


def dct2_model32(u32):
    """oracle.mdct2.dct_2n in float32 / complex64."""
    u = torch.from_numpy(np.asarray(u32, dtype=np.float32))
    N = u.shape[-1]
    y = torch.fft.rfft(torch.cat([u, torch.zeros_like(u)], dim=-1), dim=-1)[..., :N] / N
    k = np.arange(N)
    c = torch.from_numpy((2 * np.cos(np.pi * k / (2 * N))).astype(np.float32))
    s = torch.from_numpy((2 * np.sin(np.pi * k / (2 * N))).astype(np.float32))
    return (y.real * c + y.imag * s).numpy()


def dct3_model32(X32):
    """oracle.mdct2.idct_2n in float32 / complex64."""
    X = torch.from_numpy(np.asarray(X32, dtype=np.float32))
    N = X.shape[-1]
    k = np.arange(N)
    c = torch.from_numpy((2 * np.cos(np.pi * k / (2 * N))).astype(np.float32))
    s = torch.from_numpy((2 * np.sin(np.pi * k / (2 * N))).astype(np.float32))
    z = torch.complex(X * c, X * s)
    z = torch.cat([z, torch.zeros_like(z[..., :1])], dim=-1)
    return (torch.fft.irfft(z, n=2 * N, dim=-1)[..., :N] * N).numpy()


K_SEEDS = (0, 1, 2)
K_FRAMES = 6


def _ratio(model, ref):
    norm = np.sqrt((ref * ref).sum(-1, keepdims=True))
    return float((np.abs(model.astype(np.float64) - ref) / (U32 * norm)).max())


def measure_k_mdct4(n_fft):
    """(forward ratio, inverse ratio): worst max |err| / (U32 ||frame||_2) of the complex64 models over K_SEEDS."""
    hop = n_fft // 2
    w = window("sine", n_fft)
    fwd = inv = 0.0
    for seed in K_SEEDS:
        x = signal((2, (K_FRAMES - 1) * hop), 7000 + 10 * seed + n_fft)
        fr32 = gather_frames(x, hop, n_fft, hop, K_FRAMES, dtype=np.float32) * w
        ref = mdct4_ref(x, w, n_fft, hop, n_fft, hop, K_FRAMES)
        fwd = max(fwd, _ratio(mdct4_model32(fr32, n_fft), ref.out))
        spec = signal((2, K_FRAMES, n_fft // 2), 7500 + 10 * seed + n_fft)
        inv = max(inv, _ratio(imdct4_model32(spec, n_fft), spec.astype(np.float64) @ cos4(n_fft).T))
    return fwd, inv


def measure_k_dct(n_fft):
    """(DCT-II ratio, DCT-III ratio) of the float32 models of DCT_2N_native / IDCT_2N_native over K_SEEDS."""
    hop = n_fft // 2
    w = window("sine", n_fft)
    fwd = inv = 0.0
    for seed in K_SEEDS:
        x = signal((2, (K_FRAMES - 1) * hop), 8000 + 10 * seed + n_fft)
        fr32 = gather_frames(x, hop, n_fft, hop, K_FRAMES, dtype=np.float32) * w
        fwd = max(fwd, _ratio(dct2_model32(fr32), dct2_rows(fr32)))
        spec = signal((2, K_FRAMES, n_fft), 8500 + 10 * seed + n_fft)
        inv = max(inv, _ratio(dct3_model32(spec), dct3_rows(spec)))
    return fwd, inv


def k_from(ratios):
    return float(math.ceil(8.0 * max(ratios)))


# ----------------------------------------------------------------------------------------------------------------------
# comparison: every element, with a message that says where
# ----------------------------------------------------------------------------------------------------------------------
def _nonzero(a):
    return np.asarray(a) != 0                                         # -0.0 == 0: the sign of a zero is not compared


def _fail(what, bad, got, ref, tol, names, hists):
    """hists: (name, column of the index, modulus or None, divisor or None)."""
    idx = np.argwhere(bad)
    n = len(idx)
    first = [tuple(int(v) for v in i) + (float(got[tuple(i)]), float(ref[tuple(i)]), float(tol[tuple(i)])) for i in idx[:8]]
    hist = {name: _hist(idx[:, col] // (div or 1), mod) for name, col, mod, div in hists}
    raise AssertionError(f"{what}: {n} of {bad.size} elements outside their bound; first {names + ('got', 'want', 'tol')}: {first}; "
                         f"histograms of failing elements: {hist}")


def assert_frames_close(got, ref, K, what):
    """got [B, F, L] float32 (host), ref: FramesRef or a float64 array.  Every element within K U32 ||ref[b, t, :]||_2; a frame
    whose reference is identically zero must be zero exactly.  Returns the worst |err| / tol (for reports)."""
    want = ref.out if isinstance(ref, FramesRef) else np.asarray(ref, dtype=np.float64)
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == np.float32, (what, got.dtype)
    norms = np.sqrt((want * want).sum(-1))
    tol = np.broadcast_to((K * U32 * norms)[..., None], want.shape)
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= tol)                                               # a NaN fails; tol = 0: exact zero demanded
    if bad.any():
        _fail(what, bad, got, want, tol, ("b", "t", "k"),
              [("t", 1, None, None), ("t%8", 1, 8, None), ("k", 2, None, None), ("k%64", 2, 64, None), ("b", 0, None, None)])
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


def assert_samples_close(got, ref, K, what, hop):
    """got [B, out_len] float32 (host), ref: SamplesRef.  Every sample within K U32 ref.tol1; a sample no frame covers must be
    zero exactly.  Returns the worst |err| / tol."""
    got = np.asarray(got)
    want = ref.out
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == np.float32, (what, got.dtype)
    tol = K * U32 * ref.tol1
    assert not tol[:, ~ref.covered].any()
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= tol)
    if bad.any():
        _fail(what, bad, got, want, tol, ("b", "m"),
              [("m//hop", 1, None, hop), ("m%hop", 1, hop, None), ("m%64", 1, 64, None), ("b", 0, None, None)])
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# spectrogram codec (csrc/spectro.hip): the kernels' expressions in float64 on the same float32 inputs, and their bounds
# ----------------------------------------------------------------------------------------------------------------------
# Ulp errors of the two library functions.  The HIP math API's accuracy table is not shipped with the toolchain this was
# written against, so both figures are the 2 ulp that table is remembered to give at most -- UNMEASURED.  ulp(v) <= 2 U32 |v|.
LOG10F_ULPS = 2
EXP10F_ULPS = 2
MIN_VALUE = 1e-7
LN10 = math.log(10.0)
C005 = float(np.float32(0.05))                                       # the kernels' 0.05f
PLANTED = (1e3, -1e3, 0.0, 0.0, 5e-8, -5e-8, 1e-3, -1e-3)            # the extremes of the dB range first; +-5e-8: the clamp branch


def spectro_spec(B, F, M, seed):
    """spec [B, F, M] float32: normal values over four decades (all |.| < 1e3) with PLANTED values; +-1e3 and one exact zero sit
    in bin 0, so both extremes of the dB range are in a kept row for every mask_rows < M (the single-channel minimum is reached
    at exact zeros only).  Shapes too small for all take the first that fit."""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((B, F, M)) * 10.0 ** rng.uniform(-4, 0, (B, F, M))).astype(np.float32)
    s = np.clip(s, -100.0, 100.0)
    flat = s.reshape(-1)
    rows = B * F
    taken = []
    for i, v in enumerate(PLANTED):
        if len(taken) >= flat.size:
            break
        if i < 3:
            p = (0, rows - 1, rows // 2)[i] * M                       # bin 0 of the first / the last / the middle (b, f) row
            if p in taken:
                continue
        else:
            free = [q for q in rng.permutation(flat.size)[: len(PLANTED) + 2] if q not in taken]
            if not free:
                continue
            p = int(free[0])
        flat[p] = v
        taken.append(p)
    return s


def _f32(v):
    return float(np.float32(v))


def encode_db(spec, channels, alpha, min_value):
    """Pass 1: db [B, C, M, F] float64, its per-element bound tol [same], pha [B, 1, M, F] float32.
    d = 20 log10f(arg) - 20.  arg = alpha pos + (1 - alpha) neg with one of pos / neg zero (or |s| + min_value): the rounding
    of 1 - alpha, one product, one sum: relative error <= 3 u, which log10 turns into 3 u / ln 10 absolute; log10f itself:
    LOG10F_ULPS ulp(L) <= 2 LOG10F_ULPS u |L|; the product with 20 rounds once (u |20 L|), the subtraction once (u |d|); a
    fused multiply-add only drops one of those:   tol_d = u (20 (3 / ln 10 + 2 LOG10F_ULPS |L|) + 20 |L| + |d|)."""
    s = np.asarray(spec, dtype=np.float32).astype(np.float64)
    a, mv = _f32(alpha), _f32(min_value)
    neg = 0.5 * (np.abs(s) - s)
    pos = s + neg
    if channels == 2:
        args = [np.maximum(a * pos + (1.0 - a) * neg, mv), np.maximum((1.0 - a) * pos + a * neg, mv)]
    else:
        args = [np.maximum(np.abs(s) + mv, mv)]
    L = np.stack([np.log10(g) for g in args], axis=1)                 # [B, C, F, M]
    d = 20.0 * L - 20.0
    tol = U32 * (20.0 * (3.0 / LN10 + 2.0 * LOG10F_ULPS * np.abs(L)) + 20.0 * np.abs(L) + np.abs(d))
    pha = np.sign(np.asarray(spec, dtype=np.float32)).astype(np.float32)
    return d.transpose(0, 1, 3, 2).copy(), tol.transpose(0, 1, 3, 2).copy(), pha.transpose(0, 2, 1)[:, None].copy()


def encode_ref(spec, channels, alpha, min_value, mask_rows, mask_mode, noise=None, noise_sign=None):
    """p2phd_spectro_encode_ex in float64: dict(pha, db, out, out_tol, norm = (min, max, mean, std), norm_tol, kappa).
    Kept rows:  v = (d - mn) / (mx - mn); with d, mn, mx off by e, en, ex (tol_d of the element / of the extremes) and one
      rounding each for the difference, the range, its reciprocal and the product:
      |dv| <= (e + en) / R + v (ex + en) / R + 4 u v,  R = mx - mn.
    Masked rows (encode_pass2_kernel): v = (noise - nmn) nscale [* sign], nmn = 0 in mask_mode 0, nscale = 1 / (nmax - nmin) with
      EXACT float32 extremes: four roundings, |dv| <= ((1 + u)^4 - 1) |v|; no noise: 0 exactly.
    mean: the float32 sums run over the <= P = C min(32, F) min(32, M) terms of a block (any order: sum_bound), the partials
      are merged in double:  |dmean| <= sum_bound(sum |d| / count, P) + mean(tol_d).
    std:  var = (s2 - count mean^2) / (count - 1) in double from the float32-accumulated s1, s2:
      |ds2| <= sum_bound(sum d^2, P, 2) + sum (2 |d| tol_d + tol_d^2), |ds1| <= count |dmean|,
      |dvar| <= (|ds2| + 2 |mean| |ds1|) / (count - 1).  The subtraction cancels: relative to var the error of s2 is
      amplified by kappa = sum d^2 / ((count - 1) var) (returned; about 4 for the operands here), and the bound carries that
      factor through |ds2| / (count - 1) being compared with var.  std = sqrt(var) lies in [sqrt(var - dvar), sqrt(var + dvar)],
      plus 2 u std for the square root and the conversion to float."""
    from _exact import sum_bound
    d, tol_d, pha = encode_db(spec, channels, alpha, min_value)
    B, C, M, F = d.shape
    count = d.size
    mn, mx = float(d.min()), float(d.max())
    en = float(tol_d[d <= mn + 1e-3].max())
    ex = float(tol_d[d >= mx - 1e-3].max())
    R = mx - mn
    P = C * min(32, F) * min(32, M)
    mean = float(d.mean())
    dmean = sum_bound(float(np.abs(d).sum()) / count, P) + float(tol_d.mean())
    if count > 1:
        var = float(((d - mean) ** 2).sum() / (count - 1))
        ds2 = sum_bound(float((d * d).sum()), P, 2) + float((2 * np.abs(d) * tol_d + tol_d ** 2).sum())
        dvar = (ds2 + 2 * abs(mean) * count * dmean) / (count - 1)
        std = math.sqrt(var)
        dstd = max(math.sqrt(var + dvar) - std, std - math.sqrt(max(var - dvar, 0.0))) + 2 * U32 * std
        kappa = float((d * d).sum()) / ((count - 1) * var) if var > 0 else float("inf")
    else:
        std, dstd, kappa = 0.0, 0.0, 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (d - mn) / R                                            # R = 0 (one value): 0 / 0 = NaN, as the kernel and the reference
        out_tol = (tol_d + en) / R + out * (ex + en) / R + 4 * U32 * out
    keep = M - mask_rows
    if mask_rows > 0:
        if noise is not None:
            nz = np.asarray(noise, dtype=np.float32).astype(np.float64)
            nmn = 0.0 if mask_mode == 0 else float(nz.min())
            with np.errstate(invalid="ignore", divide="ignore"):     # one noise value: x / 0, as the kernel and the reference
                v = (nz - nmn) / (float(nz.max()) - float(nz.min()))
            if mask_mode == 1:
                v = v * np.asarray(noise_sign, dtype=np.float64)
            out[:, :, keep:, :] = v
            out_tol[:, :, keep:, :] = ((1 + U32) ** 4 - 1) * np.abs(v)
        else:
            out[:, :, keep:, :] = 0.0
            out_tol[:, :, keep:, :] = 0.0
    return dict(pha=pha, db=d, out=out, out_tol=out_tol, norm=(mn, mx, mean, std), norm_tol=(en, ex, dmean, dstd), kappa=kappa,
                keep=keep)


def decode_operands(B, F, M, C, seed):
    """x [B, C, M, F] float32 in [-1, 1] with exact 0 and +-1 entries and (C = 2) a band of equal channels; pha [B, M, F] in
    {-1, 0, 1}; (min, max) float32, not exactly representable differences."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (B, C, M, F)).astype(np.float32)
    r = rng.random(x.shape)
    x[r < 0.05] = 0.0
    x[r > 0.95] = 1.0
    if C == 2 and M > 2:
        x[:, 1, M // 2] = x[:, 0, M // 2]                             # a0 == a1: sign(a0 - a1) = 0
    pha = rng.integers(-1, 2, (B, M, F)).astype(np.float32)
    return x, pha, np.array([-71.3, 19.7], dtype=np.float32)


def _amplitude(x, mm, min_value):
    """a = 10 exp10f(t) - min_value, t = (|x| range + mn) 0.05f, and its bound E.
    t: the roundings of range = max - min, of |x| range, of the sum and of the product with 0.05f:
      dt <= u (0.05 (2 |x range| + |x range + mn|) + |t|);  exp10 turns dt into the relative error ln(10) dt (for the worst
      |t| = 3.6 here that is 8 u per u of RELATIVE error of t: the amplification ln(10) |t|); exp10f: EXP10F_ULPS ulp <= 2
      EXP10F_ULPS u relative; the product with 10 and the subtraction of min_value round once each:
      E = 10 e (ln(10) dt + (2 EXP10F_ULPS + 1) u) + u |a|."""
    ax = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64))
    mn, mx = float(mm[0]), float(mm[1])
    rng_ = mx - mn
    t = (ax * rng_ + mn) * C005
    dt = U32 * (C005 * (2 * np.abs(ax * rng_) + np.abs(ax * rng_ + mn)) + np.abs(t))
    e = 10.0 ** t
    a = 10.0 * e - _f32(min_value)
    E = 10.0 * e * (LN10 * dt + (2 * EXP10F_ULPS + 1) * U32) + U32 * np.abs(a)
    return a, E


def decode_ref(x, mm, alpha, min_value):
    """p2phd_spectro_decode: spec [B, F, M] = (a0 - a1) inv, inv = 1 / (2 alpha - 1); (value, tol).  The difference, 2 alpha - 1,
    its reciprocal and the product round once each: tol = |inv| (E0 + E1 + 4 u (|a0| + |a1|)) -- it scales with the
    amplitudes, not with their cancelled difference."""
    a, E = _amplitude(x, mm, min_value)
    inv = 1.0 / (2.0 * _f32(alpha) - 1.0)
    v = (a[:, 0] - a[:, 1]) * inv
    tol = abs(inv) * (E[:, 0] + E[:, 1] + 4 * U32 * (np.abs(a[:, 0]) + np.abs(a[:, 1])))
    return v.transpose(0, 2, 1).copy(), tol.transpose(0, 2, 1).copy()


def decode_signed_ref(x, pha, mm, channels, keep, min_value, scale):
    """p2phd_spectro_decode_signed: amp * sgn * scale; (value, tol, ambiguous).  amp = a0 (+ a1: one rounding), times scale: one;
    tol = |scale| (E0 (+ E1) + 2 u |amp|).  Rows >= keep of the two-channel form take sgn = sign(a0 - a1) from the ROUNDED
    amplitudes: `ambiguous` marks elements with 0 < |a0 - a1| <= E0 + E1, whose sign rounding could flip (the operands have none:
    asserted on the CPU)."""
    a, E = _amplitude(x, mm, min_value)
    sgn = np.asarray(pha, dtype=np.float64).copy()                    # [B, M, F]
    amp, Et = a[:, 0], E[:, 0]
    amb = np.zeros(sgn.shape, dtype=bool)
    if channels == 2:
        amp, Et = a[:, 0] + a[:, 1], E[:, 0] + E[:, 1]
        diff = a[:, 0] - a[:, 1]
        eq = np.asarray(x, dtype=np.float32)
        same = np.abs(eq[:, 0]) == np.abs(eq[:, 1])
        diff = np.where(same, 0.0, diff)
        sgn[:, keep:] = np.sign(diff)[:, keep:]
        amb[:, keep:] = ((~same) & (np.abs(diff) <= Et))[:, keep:]
    s = _f32(scale)
    v = amp * sgn * s
    tol = abs(s) * (Et + 2 * U32 * np.abs(amp)) * (sgn != 0)
    return v.transpose(0, 2, 1).copy(), tol.transpose(0, 2, 1).copy(), amb.transpose(0, 2, 1).copy()


def assert_elements_close(got, want, tol, what, names):
    """Every element of `got` within `tol` of `want` (NaN matches NaN only, an infinity the same infinity); returns the worst
    |err| / tol."""
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want)
        both_nan = (np.isnan(got) & np.isnan(want)) | (np.isinf(want) & (got == want))
        bad = ~((err <= tol) | both_nan)
    if bad.any():
        tolb = np.broadcast_to(tol, want.shape)
        _fail(what, bad, got, want, tolb, names, [(nm, i, None, None) for i, nm in enumerate(names)] +
              [(f"{names[-1]}%32", len(names) - 1, 32, None), (f"{names[-2]}%32", len(names) - 2, 32, None)])
    live = np.broadcast_to(tol, want.shape) > 0
    live = live & ~both_nan
    return float((err[live] / np.broadcast_to(tol, want.shape)[live]).max()) if live.any() else 0.0
