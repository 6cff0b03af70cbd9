"""Float64 numpy restatement of the per-row evaluation metrics (csrc/metrics.hip, p2phd_audio_metrics_rows).  TEST
INFRASTRUCTURE ONLY.  The spectra and the moment matching are oracle.evaltail's; the band split and the segmental SNR are
stated here, per frame as well as per row.

Segmental SNR: frames of W samples start at f * H, f < F = (T - W) // H; window w[i] = 0.5 (1 - cos(2 pi (i + 1) / (W + 1)));
per frame v = clamp(10 log10(Es / (En + eps) + eps), -10, 35), Es = sum (w hr)^2, En = sum (w hr - w x)^2, eps = 2^-52; the
row's value is the mean of v, NaN when F < 1.
Band LSD: per STFT frame d_band = sqrt(mean_{k in band} (log10(P_hr[k] + 1e-6) - log10(P_sr'[k] + 1e-6))^2) with the bands
all bins / k < cut_bin / k >= cut_bin; a row's value is the mean of d_band over its frames."""
import numpy as np

from oracle import evaltail as E

NAMES = ("mse", "snr_sr", "snr_lr", "lsd", "lsd_lf", "lsd_hf", "ssnr_sr", "ssnr_lr")
EPS = 2.0 ** -52
SNR_MIN, SNR_MAX = -10.0, 35.0


def seg_geometry(rate):
    """(W, H) for a sampling rate: 30 ms segments every quarter of that."""
    return int(round(0.03 * rate)), int(np.floor(0.25 * 0.03 * rate))


def seg_window(W):
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, W + 1) / (W + 1)))


def seg_frame_count(T, W, H):
    return max(0, (T - W) // H)


def ssnr_frames(hr, x, W, H):
    """One row each (1-D) -> the clamped dB value of every frame, shape [F]."""
    hr, x = np.asarray(hr, np.float64), np.asarray(x, np.float64)
    F = seg_frame_count(hr.shape[-1], W, H)
    w = seg_window(W)
    idx = np.arange(W)[None, :] + H * np.arange(F)[:, None]
    a, b = w * hr[idx], w * x[idx]
    es, en = (a ** 2).sum(-1), ((a - b) ** 2).sum(-1)
    return np.clip(10.0 * np.log10(es / (en + EPS) + EPS), SNR_MIN, SNR_MAX)


def ssnr(hr, x, W, H):
    v = ssnr_frames(hr, x, W, H)
    return v.mean() if v.size else np.nan


def lsd_frames(hr, sr_matched, n_fft, hop, win, window2, center, cut_bin):
    """Rows [B, T] -> (d_all, d_lo, d_hi), each [B, frames]; n_fft / hop / win are the options' values, doubled here as
    compute_matrics doubles them."""
    ph = E.power_spectrogram(hr, 2 * n_fft, 2 * hop, 2 * win, window2, center)
    ps = E.power_spectrogram(sr_matched, 2 * n_fft, 2 * hop, 2 * win, window2, center)
    d2 = (np.log10(ph + 1e-6) - np.log10(ps + 1e-6)) ** 2                     # [B, bins, frames]
    return np.sqrt(d2.mean(-2)), np.sqrt(d2[:, :cut_bin].mean(-2)), np.sqrt(d2[:, cut_bin:].mean(-2))


def rows(hr, lr, sr, n_fft, hop, win, window2, center, cut_bin, W, H):
    """-> (rows [B, 8] float64 in the order of NAMES, sr moment-matched to hr [B, T])."""
    hr = np.atleast_2d(np.asarray(hr, np.float64))
    lr = np.atleast_2d(np.asarray(lr, np.float64))
    srm = E.match_moments(np.atleast_2d(np.asarray(sr, np.float64)), hr)
    out = np.empty((hr.shape[0], 8))
    with np.errstate(divide="ignore"):
        out[:, 0] = ((srm - hr) ** 2).mean(-1)
        out[:, 1] = 10 * np.log10((hr ** 2).sum(-1) / ((srm - hr) ** 2).sum(-1))
        out[:, 2] = 10 * np.log10((hr ** 2).sum(-1) / ((lr - hr) ** 2).sum(-1))
    for j, d in enumerate(lsd_frames(hr, srm, n_fft, hop, win, window2, center, cut_bin)):
        out[:, 3 + j] = d.mean(-1)
    for b in range(hr.shape[0]):
        out[b, 6] = ssnr(hr[b], srm[b], W, H)
        out[b, 7] = ssnr(hr[b], lr[b], W, H)
    return out, srm


def signals(B, T, W, H, seed):
    """Seeded noise plus a sine, float32 [B, T] each (hr, lr, sr); by row index modulo 3:
    0: hr silent over min(W + H + 1, T // 2) samples from T // 4 on; 1: lr == hr; 2: sr = 1.7 hr - 0.3 (so sr' ~ hr)."""
    g = np.random.default_rng(seed)
    t = np.arange(T)
    hr = 0.1 * g.standard_normal((B, T)) + 0.3 * np.sin(2 * np.pi * 0.031 * t + g.uniform(0, 6, (B, 1)))
    for b in range(0, B, 3):
        n = min(W + H + 1, T // 2)
        hr[b, T // 4:T // 4 + n] = 0.0
    hr = hr.astype(np.float32)
    lr = (hr + 0.05 * g.standard_normal((B, T))).astype(np.float32)
    sr = (1.3 * hr + 0.04 * g.standard_normal((B, T)) - 0.02).astype(np.float32)
    for b in range(1, B, 3):
        lr[b] = hr[b]
    for b in range(2, B, 3):
        sr[b] = np.float32(1.7) * hr[b] - np.float32(0.3)
    return hr, lr, sr
