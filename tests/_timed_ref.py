"""Per-element checks of the time-domain discriminator kernels (csrc/timed.hip: p2phd_timed_pack_pair, p2phd_timed_frames_fwd,
p2phd_timed_frames_bwd): operands, float64 references, derived bounds and float32 emulations of the three kernels.

Why not a relative L2 norm over the tensor.  The decode 10 * 10^((|x| range + min) / 20) spans more than four decades, so the
loud frames carry the norm of the tensor and an error in a quiet frame, a dropped bin or a swapped pair of frames hides in
it (the argument of tests/_transform_ref.py, whose references, constants K and comparison functions are used here and not
restated).  Every element is compared against a bound that scales with its own frame.

Notation: u = U32 = 2^-24; N = n_fft; sr [B, 2, N, F]; (S, tolS) = decode_ref(sr, mm, alpha, min_value), S [B, F, N];
sw[i] = float64(f32(window[i])) float64(f32(scale)) -- the kernels form s_win[i] = fl(window[i] * scale) once per workgroup;
c_0 = 1, c_k = 2 otherwise; K = k_dct(N), relative to the norm of the transform's OUTPUT row, measured against the reference's
algorithm (tests/test_transform_ref_host.py pins it).

Forward: want[b, t, i] = sw[i] y[b, t, i], y = dct3_rows(S) (`frames_fwd_ref`).
  The kernel rounds s_win once and the product with it once; 3 u |want| covers both with one to spare.
  * dense operands (`dense_operands`: |x| <= 1 with exact 0, -0, +-1 and bins with |x0| == |x1|): the decode error tolS of every
    bin reaches every output of its frame with weight at most c_k |cos| <= c_k:
      tol = |sw_i| (K u ||y_t||_2 + sum_k c_k tolS[t, k]) + 3 u |want|.
    The sum is a worst case and dominates (the transform term is 0.1 .. 0.5 of it): the structural check, not the tight one.
  * two-level operands (`two_level_operands`: |x| in {1, 0.5} per bin and channel, random signs): a bin with |x0| == |x1| is
    (a - mv) - (a - mv) = 0 exactly, in float32 as in float64; every other bin is +-((A(1) - mv) - (A(0.5) - mv)) inv -- the
    same float32 expression on the same inputs, and negation is exact -- so all non-zero bins of the kernel's S hold ONE
    float32 magnitude m' = m (1 + delta), |delta| <= rho = max tolS / |S| over the non-zero bins.  The transform is linear:
    the kernel transforms (1 + delta) S, whose exact result is (1 + delta) y.  So the decode error is one common relative
    factor of the output and never meets the cancellation inside the cosine sum:
      tol = |sw_i| K u ||y_t||_2 + (rho + 3 u) |want|.
    rho is about 36 u for mm = (-71.3, 19.7); the host test asserts rho <= 64 u and the one-magnitude premise.

Backward: u_t[i] = g[t, i] sw[i]; gX = dct2_rows(u, scale = N, k0_scale = 0.5), i.e. gX_0 = sum_i u_i, gX_k = 2 sum_i u_i cos(.)
  (the kernel's comment: "scale N and k0 1/2"); d_c = +- inv dk A(x_c) sign(x_c), + for channel 0, - for channel 1, A(x) = 10 *
  10^t(x) (`_amplitude` without its min_value subtraction), dk = C005 ln(10) (max - min) -- the derivative of the function the
  forward reference computes, which holds the kernels' 0.05f = C005 in t; it differs from 0.05 ln(10) (max - min) by 2^-26
  relative, a quarter of u --, sign(0) = 0; want[b, c, k, t] = gX[b, t, k] d_c[b, k, t] (`frames_bwd_ref`).
  * the windowed input carries two roundings (s_win, the product with g): |du_i| <= 2 u |u_i|, which reaches gX_k with weight at
    most c_k: 2 u c_k ||u_t||_1; the transform itself: K u ||gX_t||_2.  Both are absolute errors of gX and scale with |d|.
  * d is a product and its error relative: inv = 1 / (2 alpha - 1): the subtraction and the reciprocal, 2 u; dk: the float32
    forms of 0.05 and of ln(10), the range and two products, 5 u; A: ln(10) dt + (2 EXP10F_ULPS + 1) u (`_amplitude`); the
    three products gX inv, . A, . dk: 3 u (the products with sign(x) = +-1 or 0 and the negation are exact):
      rho_d = ln(10) dt + (2 EXP10F_ULPS + 11) u       (per element: dt depends on |x|)
      tol = (|d| (K u ||gX_t||_2 + 2 u c_k ||u_t||_1) + rho_d |want|) SMALL
    SMALL = 1 + 2^-20 covers the products of two first-order terms.  An element with x == 0 (either sign) has d = 0 and
    tol = 0: exactly zero is demanded.

Pack: raw mode is one rounding to the storage type -- torch's own cast gives the bits.  dB mode: d = 20 log10f(arg) - 20, arg =
  max(|x|, min_value) exact (fabsf and fmaxf do not round).  As `encode_db` counts it, without its argument term: log10f:
  LOG10F_ULPS ulp(L) <= 2 LOG10F_ULPS u |L|, times 20; the product with 20 rounds once, u |20 L|; the subtraction once, u |d|
  (a fused multiply-add only drops one):   tol = u (20 (2 LOG10F_ULPS + 1) |L| + |d|), plus half an ulp of the stored type for
  16-bit storage (`_companions.stored_bound`).

The float32 emulations (`*_model32`) restate the kernels' expressions in numpy float32 with exp10f / log10f taken as the
correctly rounded value (deterministic on every host) and the transforms of `dct3_model32` / `dct2_model32`; their `mutant`
arguments plant the defects the host test demands the bounds to reject.  `kernel_dct3_64` is the forward kernel's own
factorisation in float64 (the only place the `X[N - k]` index exists).

Plain helper: no fixtures, no test functions.  tests/test_timed_ref_host.py checks it on the CPU, tests/test_gpu_timed_elements.py
runs the kernels against it.
"""
import functools
import math

import numpy as np
import torch

import _companions as K_
import _transform_ref as R
from _exact import U32

ALPHA = 0.6
MIN_VALUE = R.MIN_VALUE
SCALE = 0.37                                                          # table cases; the kbd case takes sqrt(up_ratio - 1)
UP_RATIO = 6.0
MM = (-71.3, 19.7)
SMALL = K_.SMALL
RHO_MAX = 64 * U32

# (n_fft, B, F): frames per tile 16 / 16 / 16 / 8 / 4, FFT waves 4 / 4 / 4 / 4 / 2.  F = 1, f_tile - 1, f_tile, f_tile + 1, more
# tiles than FFT waves, a batch above 3.
N_FFTS = (16, 64, 512, 1024, 2048)
GEOMS = [(16, 3, 17),
         (64, 2, 1), (64, 2, 15), (64, 2, 16), (64, 2, 33), (64, 5, 17),
         (512, 2, 16), (512, 2, 21),
         (1024, 2, 1), (1024, 2, 8), (1024, 2, 13),
         (2048, 2, 1), (2048, 2, 4), (2048, 2, 7)]
GEOM_IDS = ["n{}_b{}_f{}".format(*g) for g in GEOMS]

FWD_MUTANTS = ("rev_bins", "bin0_x2", "window_reversed", "drop_bin", "swap_frames", "last_partial_zero", "range_is_max")
BWD_MUTANTS = ("ch1_plus", "sign0_is_1", "gx0_x2", "window_reversed")
PACK_MUTANTS = ("swapped", "no_minus_20", "clamp_half")


def f_tile(n_fft):
    """frames_tile of csrc/timed.hip."""
    return 16 if n_fft <= 512 else (8 if n_fft <= 1024 else 4)


def _f32(v):
    return float(np.float32(v))


def mm_array(mm=MM):
    return np.array(mm, dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------------------------------
def dense_operands(B, n_fft, F, seed):
    """sr [B, 2, N, F] float32 in [-1, 1] from `decode_operands` (exact 0 and 1, bins N/2 with x0 == x1), plus exact -1 and -0.0
    entries and bins N/4 with x1 == -x0; (min, max) float32."""
    x, _, mm = R.decode_operands(B, F, n_fft, 2, seed)
    rng = np.random.default_rng(seed + 77)
    r = rng.random(x.shape)
    x[r < 0.04] = -1.0
    x[(r > 0.04) & (r < 0.07)] = -0.0
    x[:, 1, n_fft // 4] = -x[:, 0, n_fft // 4]
    x[:, 1, n_fft // 2] = x[:, 0, n_fft // 2]
    # both zeros and both units in every case, whatever the draw (F = 1 at N = 16 leaves 64 elements)
    flat = x[0, 0].reshape(-1)
    flat[:4] = (0.0, -0.0, 1.0, -1.0)
    return x, mm


def two_level_operands(B, n_fft, F, seed):
    """sr [B, 2, N, F] float32 with |x| in {1, 0.5}, random signs; (min, max) = MM."""
    rng = np.random.default_rng(seed)
    mag = np.where(rng.random((B, 2, n_fft, F)) < 0.5, 1.0, 0.5)
    sgn = np.where(rng.random(mag.shape) < 0.5, -1.0, 1.0)
    return (mag * sgn).astype(np.float32), mm_array()


def cotangent(B, n_fft, F, seed, impulse=False):
    """g [B, F, N] float32: standard normal, or one unit impulse per frame (at a position that walks over the frame)."""
    if not impulse:
        return np.random.default_rng(seed).standard_normal((B, F, n_fft)).astype(np.float32)
    g = np.zeros((B, F, n_fft), dtype=np.float32)
    for b in range(B):
        for t in range(F):
            g[b, t, (7 * t + 3 * b + (n_fft - 1) * (t % 2)) % n_fft] = 1.0
    return g


PLANTED = (0.0, -0.0, 1e-7, -1e-7, 5e-8, -5e-8, float(np.finfo(np.float32).tiny), 1e-40, 1.0, -1.0, 1e3, -1e3)


def pack_operands(n, seed):
    """(a, b) float32 [n]: normal values over six decades, with PLANTED (0, -0, +-min_value, +-min_value / 2 -- the clamp branch
    --, the smallest normal, a subnormal, +-1, +-1e3) at the head of `a` and, reversed, at the tail of `b`, as far as n reaches."""
    rng = np.random.default_rng(seed)
    a, b = ((rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 1, n)).astype(np.float32) for _ in range(2))
    m = min(n, len(PLANTED))
    a[:m] = np.array(PLANTED[:m], dtype=np.float32)
    b[n - m:] = np.array(PLANTED[::-1][:m], dtype=np.float32)[::-1]
    return a, b


# ----------------------------------------------------------------------------------------------------------------------
# frames forward
# ----------------------------------------------------------------------------------------------------------------------
def _sw(w, scale):
    return np.asarray(w, dtype=np.float32).astype(np.float64) * _f32(scale)


def rho_of(S, tolS):
    """max tolS / |S| over the non-zero bins (two-level operands: the one relative error of the decoded magnitude)."""
    nz = S != 0
    return float((tolS[nz] / np.abs(S[nz])).max()) if nz.any() else 0.0


def frames_fwd_ref(sr, mm, w, alpha, min_value, scale, kind):
    """(want [B, F, N] float64, tol [same]) of p2phd_timed_frames_fwd; kind: 'dense' or 'two_level' (module docstring)."""
    S, tolS = R.decode_ref(sr, mm, alpha, min_value)
    N = S.shape[-1]
    y = R.dct3_rows(S)
    sw = _sw(w, scale)
    want = sw * y
    ynorm = np.sqrt((y * y).sum(-1, keepdims=True))
    Ku = R.k_dct(N) * U32
    if kind == "dense":
        c = np.full(N, 2.0)
        c[0] = 1.0
        tol = np.abs(sw) * (Ku * ynorm + (tolS * c).sum(-1, keepdims=True)) + 3 * U32 * np.abs(want)
    elif kind == "two_level":
        tol = np.abs(sw) * Ku * ynorm + (rho_of(S, tolS) + 3 * U32) * np.abs(want)
    else:
        raise ValueError(kind)
    return want, tol


def _exp10_32(t32):
    """exp10f taken as the correctly rounded value of 10^t for the float32 t."""
    return (10.0 ** t32.astype(np.float64)).astype(np.float32)


def _amp32(x, mm, mutant=None):
    """amp_of of csrc/timed.hip in numpy float32: 10.f * exp10f((fabsf(x) * range + mn) * 0.05f)."""
    mm = np.asarray(mm, dtype=np.float32)
    mn = mm[0]
    rng_ = mm[1] if mutant == "range_is_max" else np.float32(mm[1] - mm[0])
    t = (np.abs(np.asarray(x, dtype=np.float32)) * rng_ + mn) * np.float32(0.05)
    return np.float32(10.0) * _exp10_32(t), rng_


def _inv32(alpha):
    return np.float32(1.0) / (np.float32(2.0) * np.float32(alpha) - np.float32(1.0))


def decode_model32(sr, mm, alpha, min_value, mutant=None):
    """S [B, F, N] float32: ((A0 - mv) - (A1 - mv)) * inv, as frames_fwd_kernel stages it."""
    a, _ = _amp32(sr, mm, mutant)
    mv = np.float32(min_value)
    S = ((a[:, 0] - mv) - (a[:, 1] - mv)) * _inv32(alpha)
    return np.ascontiguousarray(S.transpose(0, 2, 1))


def kernel_dct3_64(X, mutant=None):
    """The forward kernel's factorisation in float64: conj(V_k) = (X_k + i X_{N-k}) exp(-i pi k / 2N), X_N = 0; v = Re FFT(conj V);
    y[2n] = v[n], y[2n + 1] = v[N - 1 - n].  mutant 'rev_bins': X[N - 1 - k] read for X[N - k]."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[-1]
    k = np.arange(N)
    Xr = np.zeros_like(X)
    if mutant == "rev_bins":
        Xr[..., 1:] = X[..., N - 1 - k[1:]]
    else:
        Xr[..., 1:] = X[..., N - k[1:]]
    v = np.fft.fft((X + 1j * Xr) * np.exp(-1j * np.pi * k / (2 * N)), axis=-1).real
    y = np.empty_like(X)
    y[..., 0::2] = v[..., : N // 2]
    y[..., 1::2] = v[..., ::-1][..., : N // 2]
    return y


def _first_nonzero_bin(S, b, t):
    nz = np.flatnonzero(S[b, t])
    return int(nz[min(5, len(nz) - 1)])


def frames_fwd_model32(sr, mm, w, alpha, min_value, scale, mutant=None):
    """float32 emulation of p2phd_timed_frames_fwd -> [B, F, N] float32; `mutant`: one of FWD_MUTANTS."""
    assert mutant is None or mutant in FWD_MUTANTS, mutant
    S = decode_model32(sr, mm, alpha, min_value, mutant)
    B, F, N = S.shape
    if mutant == "bin0_x2":
        S[..., 0] *= np.float32(2.0)
    if mutant == "drop_bin":
        b, t = B - 1, min(2, F - 1)
        S[b, t, _first_nonzero_bin(S, b, t)] = 0.0
    y = kernel_dct3_64(S, mutant).astype(np.float32) if mutant == "rev_bins" else R.dct3_model32(S)
    w32 = np.asarray(w, dtype=np.float32)
    s_win = (w32[::-1] if mutant == "window_reversed" else w32) * np.float32(scale)
    out = y * s_win
    if mutant == "swap_frames":
        out[:, [0, 1]] = out[:, [1, 0]]
    if mutant == "last_partial_zero":
        assert F % f_tile(N), "the last tile must be partial"
        out[:, F - 1] = 0.0
    return out


# ----------------------------------------------------------------------------------------------------------------------
# frames backward
# ----------------------------------------------------------------------------------------------------------------------
def frames_bwd_ref(g, sr, mm, w, alpha, scale):
    """(want [B, 2, N, F] float64, tol [same]) of p2phd_timed_frames_bwd (module docstring)."""
    x = np.asarray(sr, dtype=np.float32).astype(np.float64)
    N = x.shape[2]
    sw = _sw(w, scale)
    u = np.asarray(g, dtype=np.float32).astype(np.float64) * sw                 # [B, F, N]
    gX = R.dct2_rows(u, scale=float(N), k0_scale=0.5)
    Ku = R.k_dct(N) * U32
    c = np.full(N, 2.0)
    c[0] = 1.0
    gnorm = np.sqrt((gX * gX).sum(-1, keepdims=True))
    u1 = np.abs(u).sum(-1, keepdims=True)
    abs_gx = (Ku * gnorm + 2 * U32 * c * u1).transpose(0, 2, 1)[:, None]       # [B, 1, N, F]
    # d: A = 10 * 10^t and its relative bound, from _amplitude's own terms (a = A - mv, E = A rel_A + u |a|)
    mv = _f32(MIN_VALUE)
    a, E = R._amplitude(x, mm, MIN_VALUE)
    A = a + mv
    rel_A = (E - U32 * np.abs(a)) / A
    inv = 1.0 / (2.0 * _f32(alpha) - 1.0)
    dk = R.C005 * R.LN10 * (float(mm[1]) - float(mm[0]))
    d = inv * dk * A * np.sign(x)
    d[:, 1] = -d[:, 1]
    rho_d = rel_A + (2 + 5 + 3) * U32
    want = gX.transpose(0, 2, 1)[:, None] * d
    tol = (np.abs(d) * abs_gx + rho_d * np.abs(want)) * SMALL
    return want, tol


def frames_bwd_model32(g, sr, mm, w, alpha, scale, mutant=None):
    """float32 emulation of p2phd_timed_frames_bwd -> [B, 2, N, F] float32; `mutant`: one of BWD_MUTANTS."""
    assert mutant is None or mutant in BWD_MUTANTS, mutant
    x = np.asarray(sr, dtype=np.float32)
    N = x.shape[2]
    w32 = np.asarray(w, dtype=np.float32)
    s_win = (w32[::-1] if mutant == "window_reversed" else w32) * np.float32(scale)
    u = np.asarray(g, dtype=np.float32) * s_win
    X = R.dct2_model32(u) * np.float32(N)                                        # scale N: exact, a power of two
    X[..., 0] *= np.float32(1.0 if mutant == "gx0_x2" else 0.5)
    gs = (X * _inv32(alpha)).transpose(0, 2, 1)                                  # [B, N, F]
    a, rng_ = _amp32(x, mm)
    dk = np.float32(0.05) * np.float32(2.302585092994046) * rng_
    sg = np.sign(x)
    if mutant == "sign0_is_1":
        sg = np.where(x == 0, np.float32(1.0), sg)
    out = np.empty(x.shape, dtype=np.float32)
    out[:, 0] = gs * a[:, 0] * dk * sg[:, 0]
    out[:, 1] = (gs if mutant == "ch1_plus" else -gs) * a[:, 1] * dk * sg[:, 1]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# pack pair
# ----------------------------------------------------------------------------------------------------------------------
def pack_db_ref(a, b, min_value, dtype):
    """(want [n, 2] float64, tol [same]) of the dB mode's channels 0 and 1 as STORED in `dtype` (module docstring)."""
    mv = _f32(min_value)
    v = np.stack([np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)], axis=-1).astype(np.float64)
    L = np.log10(np.maximum(np.abs(v), mv))
    d = 20.0 * L - 20.0
    tol32 = U32 * (20.0 * (2 * R.LOG10F_ULPS + 1) * np.abs(L) + np.abs(d))
    tol = K_.stored_bound(torch.from_numpy(d), torch.from_numpy(tol32), dtype).numpy()
    return d, tol


def pack_db_model32(a, b, min_value, dtype, mutant=None):
    """float32 emulation of the dB mode -> [n, 2] as stored (a float32 array holding the values of `dtype`)."""
    assert mutant is None or mutant in PACK_MUTANTS, mutant
    mv = np.float32(min_value) * np.float32(0.5 if mutant == "clamp_half" else 1.0)
    v = np.stack([np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)], axis=-1)
    if mutant == "swapped":
        v = v[:, ::-1]
    L = np.log10(np.maximum(np.abs(v), mv).astype(np.float64)).astype(np.float32)
    d = np.float32(20.0) * L
    if mutant != "no_minus_20":
        d = d - np.float32(20.0)
    return torch.from_numpy(np.ascontiguousarray(d)).to(dtype).float().numpy()


def pack_raw_expected(a, b, dtype):
    """[n, 8] in `dtype` (torch, on the device of a / b): channels 0, 1 = torch's own cast, 2..7 = +0."""
    out = torch.zeros((a.numel(), 8), dtype=dtype, device=a.device)
    out[:, 0] = a.reshape(-1).to(dtype)
    out[:, 1] = b.reshape(-1).to(dtype)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# cases shared by the host and the GPU tests (references are computed once per case and left unchanged)
# ----------------------------------------------------------------------------------------------------------------------
def case_seed(n_fft, B, F):
    return 1000 * n_fft + 37 * F + B


@functools.lru_cache(maxsize=4)
def fwd_case(kind, n_fft, B, F, window="ramp", scale=SCALE, mm=None):
    """dict(sr, mm, w, scale, want, tol) of a forward case; `mm`: a (min, max) pair replacing the operands' own."""
    seed = case_seed(n_fft, B, F)
    sr, mm_ = dense_operands(B, n_fft, F, seed) if kind == "dense" else two_level_operands(B, n_fft, F, seed + 1)
    if mm is not None:
        mm_ = mm_array(mm)
    w = R.window(window, n_fft, seed % 7)
    want, tol = frames_fwd_ref(sr, mm_, w, ALPHA, MIN_VALUE, scale, kind)
    for a in (sr, mm_, w, want, tol):
        a.setflags(write=False)
    return dict(sr=sr, mm=mm_, w=w, scale=scale, want=want, tol=tol)


@functools.lru_cache(maxsize=4)
def bwd_case(n_fft, B, F, impulse=False, window="ramp", scale=SCALE, mm=None):
    seed = case_seed(n_fft, B, F)
    sr, mm_ = dense_operands(B, n_fft, F, seed)
    if mm is not None:
        mm_ = mm_array(mm)
    g = cotangent(B, n_fft, F, seed + 2, impulse)
    w = R.window(window, n_fft, seed % 7)
    want, tol = frames_bwd_ref(g, sr, mm_, w, ALPHA, scale)
    for a in (sr, mm_, w, g, want, tol):
        a.setflags(write=False)
    return dict(sr=sr, mm=mm_, w=w, g=g, scale=scale, want=want, tol=tol)


def kbd_scale():
    """The generator's scale: sqrt(up_ratio - 1)."""
    return float(math.sqrt(UP_RATIO - 1.0))
