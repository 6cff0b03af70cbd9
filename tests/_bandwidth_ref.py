"""Restatement of csrc/bandwidth.hip for the tests (test code only): the long-term average spectrum from float64
torch.stft(center=False), and the band-edge decision in numpy with the kernel's float64 operations in the kernel's order."""
import numpy as np
import torch

DEFAULTS = {'n_fft': 2048, 'hop': 1024, 'band_bins': 8, 'threshold_db': 60.0}


def window_ref(n_fft):
    i = np.arange(n_fft, dtype=np.float64)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * i / n_fft))


def frames_ref(L, n_fft, hop):
    return 1 + (L - n_fft) // hop if L >= n_fft else 0


def frame_powers_ref(rows, n_fft, hop):
    """rows [R, L] -> [R, F, K] float64: P = |X|^2 (4 / n_fft)^2 of the frames that lie wholly inside the clip, periodic Hann window."""
    x = torch.as_tensor(np.asarray(rows, dtype=np.float64))
    R, L = x.shape
    K = n_fft // 2 + 1
    if L < n_fft:
        return np.zeros((R, 0, K), dtype=np.float64)
    X = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=torch.from_numpy(window_ref(n_fft)), center=False, return_complex=True)
    P = (X.real ** 2 + X.imag ** 2) * (4.0 / n_fft) ** 2                       # [R, K, F]
    return P.permute(0, 2, 1).contiguous().numpy()


def ltas_ref(rows, n_fft, hop):
    """rows [R, L] -> psd [R, K] float64: the sum of the frames' powers (zeros for L < n_fft)."""
    return frame_powers_ref(rows, n_fft, hop).sum(axis=1)


def frame_norms_ref(rows, n_fft, hop):
    """[R, F] float64: the 2-norm of every windowed interior frame."""
    x = np.asarray(rows, dtype=np.float64)
    F = frames_ref(x.shape[1], n_fft, hop)
    w = window_ref(n_fft)
    return np.stack([np.sqrt(((x[:, f * hop:f * hop + n_fft] * w) ** 2).sum(axis=1)) for f in range(F)], axis=1)


def rel_of(threshold_db):
    """What the host passes to the kernel: 10^(-threshold_db / 10), computed once."""
    return 10.0 ** (-float(threshold_db) / 10.0)


def decide_ref(psd, rows_per_group, band_bins, rel):
    """psd [G * Q, K] float64 -> res [G, 4] float64 = {k_top, b_top, ref, thr}, the kernel's arithmetic: rows added ascending, a
    band's bins added ascending and divided once by their count, ref folded from 0.0 with `>` (a NaN never wins), thr one product,
    both comparisons strict."""
    psd = np.asarray(psd, dtype=np.float64)
    Q, M = int(rows_per_group), int(band_bins)
    K = psd.shape[1]
    G = psd.shape[0] // Q
    rel = np.float64(rel)
    res = np.zeros((G, 4), dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for g in range(G):
            s = psd[g * Q].copy()
            for q in range(1, Q):
                s = s + psd[g * Q + q]
            B = (K + M - 1) // M
            levels = np.empty(B, dtype=np.float64)
            for b in range(B):
                k0, k1 = b * M, min(K, (b + 1) * M)
                t = s[k0]
                for k in range(k0 + 1, k1):
                    t = t + s[k]
                levels[b] = t / np.float64(k1 - k0)
            ref = np.float64(0.0)
            for l in levels:
                if l > ref:
                    ref = l
            thr = ref * rel
            b_top = -1
            for b in range(B):
                if levels[b] > thr:
                    b_top = b
            k_top = -1
            if b_top >= 0:
                for k in range(min(K, (b_top + 1) * M) - 1, b_top * M - 1, -1):
                    if s[k] > thr:
                        k_top = k
                        break
            res[g] = (k_top, b_top, ref, thr)
    return res


def margin_db(psd, rows_per_group, band_bins, rel):
    """How far, in dB, the nearest band level or bin of the deciding bands stands from thr (group 0): the smallest |10 log10(v / thr)|
    over every band level and over the bins of the top band and of the band above it.  inf where nothing passes or thr is 0."""
    psd = np.asarray(psd, dtype=np.float64)
    Q, M = int(rows_per_group), int(band_bins)
    K = psd.shape[1]
    s = psd[:Q].sum(axis=0)
    k_top, b_top, ref, thr = decide_ref(psd[:Q], Q, M, rel)[0]
    if b_top < 0 or not thr > 0.0:
        return float('inf')
    B = (K + M - 1) // M
    levels = np.array([s[b * M:min(K, (b + 1) * M)].mean() for b in range(B)])
    vals = list(levels) + list(s[int(b_top) * M:min(K, (int(b_top) + 2) * M)])
    vals = np.array([v for v in vals if v > 0.0])
    return float(np.abs(10.0 * np.log10(vals / thr)).min())


def bandwidth_ref(waveform, rate, plan=None):
    """waveform [C, L] -> (Hz, res4): the decision on the clip's channels as one group with `plan` (DEFAULTS where None); Hz =
    k_top * rate / n_fft, 0.0 where nothing passed."""
    p = dict(DEFAULTS, **(plan or {}))
    x = np.asarray(waveform, dtype=np.float64)
    if x.ndim == 1:
        x = x[None]
    psd = ltas_ref(x, p['n_fft'], p['hop'])
    res = decide_ref(psd, x.shape[0], p['band_bins'], rel_of(p['threshold_db']))[0]
    return (res[0] * rate / p['n_fft'] if res[0] >= 0 else 0.0), res


def brickwall_noise(n, rate, fc, seed):
    """White noise of n samples made brick-wall in the frequency domain: rfft, zero above fc, irfft; peak 0.5.  float64."""
    x = np.random.default_rng(seed).standard_normal(n)
    X = np.fft.rfft(x)
    f = np.fft.rfftfreq(n, 1.0 / rate)
    X[f > fc] = 0.0
    y = np.fft.irfft(X, n)
    return 0.5 * y / np.abs(y).max()
