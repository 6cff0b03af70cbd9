"""Restatement of csrc/stereo.hip and of plans.stereo_figures for the tests (test code only), in numpy: the long-term cross-spectrum
of a channel pair from float64 framing and rfft, the band sums with the kernel's float64 operations in the kernel's order, the
figures, and the mid/side matrix in float32.  Also the inputs the host and the GPU tests share."""
import itertools
import math

import numpy as np

from _bandwidth_ref import frames_ref, window_ref

DEFAULTS = {'n_fft': 2048, 'hop': 1024}
LANES = 256


def split_bin_ref(hr_rate, lr_rate, n_fft):
    """The first bin at or above the low rate's Nyquist frequency (integer rates: exact)."""
    return -((-int(lr_rate) * n_fft) // (2 * int(hr_rate)))


def frame_values_ref(pair, n_fft, hop):
    """pair [2, L] -> [4, F, K] float64: per interior frame and bin |A|^2, |B|^2, Re(A conj B), Im(A conj B), scaled by (4 / n_fft)^2;
    A, B the rfft of the two channels' frames under the periodic Hann window."""
    x = np.asarray(pair, dtype=np.float64)
    assert x.ndim == 2 and x.shape[0] == 2
    F, K = frames_ref(x.shape[1], n_fft, hop), n_fft // 2 + 1
    if F == 0:
        return np.zeros((4, 0, K))
    w = window_ref(n_fft)
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    A, B = np.fft.rfft(x[0][idx] * w, axis=1), np.fft.rfft(x[1][idx] * w, axis=1)
    C = A * np.conj(B)
    return np.stack([A.real ** 2 + A.imag ** 2, B.real ** 2 + B.imag ** 2, C.real, C.imag]) * (4.0 / n_fft) ** 2


def xspec_ref(rows, n_fft, hop):
    """rows [2 G, L] -> xs [G, 4, K] float64: the sums over the frames (zeros for L < n_fft)."""
    x = np.asarray(rows, dtype=np.float64)
    assert x.shape[0] % 2 == 0
    return np.stack([frame_values_ref(x[2 * g:2 * g + 2], n_fft, hop).sum(axis=1) for g in range(x.shape[0] // 2)]) \
        if x.shape[0] else np.zeros((0, 4, n_fft // 2 + 1))


def frame_norms_ref(pair, n_fft, hop):
    """[F] float64: the 2-norm of every interior frame of the complex signal w x_L + i w x_R, sqrt(||w x_L||^2 + ||w x_R||^2)."""
    x = np.asarray(pair, dtype=np.float64)
    F, w = frames_ref(x.shape[1], n_fft, hop), window_ref(n_fft)
    return np.array([math.sqrt(((x[:, f * hop:f * hop + n_fft] * w) ** 2).sum()) for f in range(F)])


def band_sum_ref(v):
    """The kernel's sum of one band of one row: lane t of 256 adds v[t], v[t + 256], .. to +0.0 in ascending order, then the lanes
    fold as a tree, s[t] = s[t] + s[t + o] for o = 128, 64, .. 1."""
    v = np.asarray(v, dtype=np.float64)
    s = np.zeros(LANES, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(0, len(v), LANES):
            part = v[j:j + LANES]
            s[:len(part)] = s[:len(part)] + part
        o = LANES // 2
        while o:
            s[:o] = s[:o] + s[o:2 * o]
            o //= 2
    return s[0]


def bands_ref(xs, k_split):
    """xs [G, 4, K] float64 -> res [G, 8] float64: {S_ll, S_rr, Re, Im} over [0, k_split), then over [k_split, K)."""
    xs = np.asarray(xs, dtype=np.float64)
    G, _, K = xs.shape
    assert 1 <= k_split <= K - 1
    res = np.zeros((G, 8), dtype=np.float64)
    for g in range(G):
        for b, (lo, hi) in enumerate(((0, k_split), (k_split, K))):
            for q in range(4):
                res[g, 4 * b + q] = band_sum_ref(xs[g, q, lo:hi])
    return res


def ratio_db_ref(num, den):
    if num != num or den != den:
        return float('nan')
    if den <= 0.0:
        return None if num <= 0.0 else float('inf')
    if num <= 0.0:
        return float('-inf')
    return 10.0 * math.log10(num / den)


def band_figures_ref(ll, rr, re, im):
    """Four sums of a band -> its figures; None where a denominator is zero, +-inf where a ratio is."""
    den = math.sqrt(ll * rr) if ll * rr > 0.0 else 0.0
    return {'corr': None if den == 0.0 else re / den, 'coherence': None if den == 0.0 else math.hypot(re, im) / den,
            'side_db': ratio_db_ref(ll + rr - 2.0 * re, ll + rr + 2.0 * re), 'balance_db': ratio_db_ref(ll, rr)}


def figures_ref(res8):
    v = [float(t) for t in res8]
    return {'low': band_figures_ref(*v[:4]), 'high': band_figures_ref(*v[4:])}


def image_ref(waveform, hr_rate, lr_rate, n_fft=2048, hop=1024):
    """waveform [2, L] -> (figures, res8) of the restatement."""
    res = bands_ref(xspec_ref(waveform, n_fft, hop), split_bin_ref(hr_rate, lr_rate, n_fft))[0]
    return figures_ref(res), res


def figure_intervals(res8, tol8):
    """The consequence of |S - S_ref| <= tol on each of the eight sums for the figures: per band and figure the interval (lo, hi) the
    figure of any such S lies in.  corr, side_db and balance_db are monotone in each sum separately, so their extremes over the box
    stand at its corners; the coherence is monotone in |Re| and |Im|, so where an interval of those crosses zero, zero is a candidate
    too.  A corner with a vanished power (or a non-positive numerator) reads as the figure's limit there, +-inf."""
    out = {}
    for name, o in (('low', 0), ('high', 4)):
        s, t = [float(v) for v in res8[o:o + 4]], [float(v) for v in tol8[o:o + 4]]
        cands = [[max(s[i] - t[i], 0.0), s[i] + t[i]] for i in (0, 1)] + [[s[i] - t[i], s[i] + t[i]] + ([0.0] if abs(s[i]) < t[i] else []) for i in (2, 3)]
        vals = {k: [] for k in ('corr', 'coherence', 'side_db', 'balance_db')}
        for ll, rr, re, im in itertools.product(*cands):
            f = band_figures_ref(ll, rr, re, im)
            big = float('inf')
            vals['corr'].append(f['corr'] if f['corr'] is not None else (big if re > 0 else -big if re < 0 else 0.0))
            vals['coherence'].append(f['coherence'] if f['coherence'] is not None else big)
            for k in ('side_db', 'balance_db'):
                vals[k] += [f[k]] if f[k] is not None else [-big, big]
        out[name] = {k: (min(v), max(v)) for k, v in vals.items()}
    return out


def matrix_ref(x, a, guard_side=False):
    """x [2, L] float32 -> [2, L] float32: a * (x0 + s), a * (x0 - s) with s = x1 (guard_side: +0 where x1 is not finite); one float32
    rounding per operation."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and x.shape[0] == 2
    a = np.float32(a)
    s = np.where(np.isfinite(x[1]), x[1], np.float32(0.0)) if guard_side else x[1]
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([a * (x[0] + s), a * (x[0] - s)]).astype(np.float32)


# ------------------------------------------------------------------------------------------
# the inputs of the premises (tests/test_stereo_host.py) and of the GPU tests that use them
# ------------------------------------------------------------------------------------------
HR, LR = 48000, 8000                                               # the split of an n_fft of 256 is bin 22, 4125 Hz
N_FFT, HOP, SAMPLES = 256, 128, 8192


def _band_noise(n, rate, f_lo, f_hi, seed):
    x = np.random.default_rng(seed).standard_normal(n)
    X = np.fft.rfft(x)
    f = np.fft.rfftfreq(n, 1.0 / rate)
    X[(f < f_lo) | (f > f_hi)] = 0.0
    y = np.fft.irfft(X, n)
    return y / np.abs(y).max()


def premise_inputs():
    """name -> [2, SAMPLES] float32, fixed seeds, peaks under 1."""
    g = lambda seed: 0.2 * np.random.default_rng(seed).standard_normal(SAMPLES)      # noqa: E731
    left, other = g(1), g(2)
    common = 0.4 * _band_noise(SAMPLES, HR, 0.0, 3000.0, 3)        # (a gap around the split: the window's leakage stays out of it)
    hi_l, hi_r = 0.4 * _band_noise(SAMPLES, HR, 5500.0, 24000.0, 4), 0.4 * _band_noise(SAMPLES, HR, 5500.0, 24000.0, 5)
    pairs = {'same': (left, left), 'inverted': (left, -left), 'half': (left, 0.5 * left), 'independent': (left, other),
             'partial': (left, 0.6 * left + 0.8 * other), 'split': (common + hi_l, common + hi_r)}
    return {k: np.stack(v).astype(np.float32) for k, v in pairs.items()}


def check_premise(name, fig):
    """The cap of the issue's table on the figures `fig` ({'low', 'high'}) of input `name`; both bands unless the table names one."""
    bands = (fig['low'], fig['high'])
    if name == 'same':
        assert all(abs(b['corr'] - 1.0) <= 1e-12 for b in bands), fig
    elif name == 'inverted':
        assert all(abs(b['corr'] + 1.0) <= 1e-12 for b in bands), fig
    elif name == 'half':
        assert all(abs(b['balance_db'] - 6.0206) <= 1e-4 for b in bands), fig
    elif name == 'independent':
        assert all(abs(b['corr']) < 0.1 for b in bands), fig
    elif name == 'partial':
        assert all(abs(b['corr'] - 0.6) <= 0.05 for b in bands), fig
    elif name == 'split':
        assert fig['low']['corr'] > 0.95 and abs(fig['high']['corr']) < 0.1, fig
    else:
        raise KeyError(name)
