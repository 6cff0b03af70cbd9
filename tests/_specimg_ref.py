"""Restatement of csrc/specimg.hip for the tests (test code only): the STFT in float64 on the CPU, and the renderer in numpy
with the kernel's own sequence of integer and float32 operations."""
import numpy as np
import torch

FLOOR_P = 1e-20
GAP_GREY = 64


def stft_db_ref(rows, n_fft, hop):
    """rows [R, L] (any float tensor or array) -> [R, F, K] float64: torch.stft in float64 with the periodic Hann window,
    centred, zero-padded; P = |X|^2 (4 / n_fft)^2; 10 log10(max(P, 1e-20))."""
    x = torch.as_tensor(np.asarray(rows, dtype=np.float64))
    i = torch.arange(n_fft, dtype=torch.float64)
    w = 0.5 * (1.0 - torch.cos(2.0 * torch.pi * i / n_fft))
    X = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode='constant', return_complex=True)
    P = (X.real ** 2 + X.imag ** 2) * (4.0 / n_fft) ** 2                       # [R, K, F]
    return (10.0 * torch.log10(torch.clamp(P, min=FLOOR_P))).permute(0, 2, 1).contiguous().numpy()


def window_ref(n_fft):
    i = np.arange(n_fft, dtype=np.float64)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * i / n_fft))


def frame_norms_ref(rows, n_fft, hop):
    """[R, F] float64: the 2-norm of every windowed frame, sqrt(sum_i (w[i] x[f hop - n_fft / 2 + i])^2)."""
    x = np.asarray(rows, dtype=np.float64)
    R, L = x.shape
    F = 1 + L // hop
    pad = np.zeros((R, n_fft // 2 + (F - 1) * hop + n_fft), dtype=np.float64)
    pad[:, n_fft // 2:n_fft // 2 + L] = x
    w = window_ref(n_fft)
    return np.stack([np.sqrt(((pad[:, f * hop:f * hop + n_fft] * w) ** 2).sum(axis=1)) for f in range(F)], axis=1)


def render_ref(db, top, range_db, width, height, gap, lut):
    """db [R, F, K] float32, top: a float32 value -> [R * height + (R - 1) * gap, width, 3] uint8, the kernel's sequence:
    integer index arithmetic, the maximum folded with fmax from -inf (NaN never wins), float32 v - lo and * scale, np.rint."""
    db = np.asarray(db, dtype=np.float32)
    R, F, K = db.shape
    W, H = int(width), int(height)
    lut = np.asarray(lut, dtype=np.uint8)
    rng = np.float32(range_db)
    with np.errstate(invalid='ignore', over='ignore'):
        lo = np.float32(top) - rng
        scale = np.float32(255.0) / rng
    img = np.full((R * H + (R - 1) * gap, W, 3), GAP_GREY, dtype=np.uint8)
    ninf = np.float32(-np.inf)
    for r in range(R):
        # frames of every column, then bins of every row
        cols = np.full((W, K), ninf, dtype=np.float32)
        for x in range(W):
            f0 = x * F // W
            f1 = max(f0 + 1, (x + 1) * F // W)
            cols[x] = np.fmax.reduce(db[r, f0:f1], axis=0, initial=ninf)
        v = np.full((H, W), ninf, dtype=np.float32)
        for y in range(H):
            yy = H - 1 - y
            k0 = yy * K // H
            k1 = max(k0 + 1, (yy + 1) * K // H)
            v[y] = np.fmax.reduce(cols[:, k0:k1], axis=1, initial=ninf)
        with np.errstate(invalid='ignore', over='ignore'):
            t = (v - lo).astype(np.float32) * scale
            t = np.rint(t.astype(np.float32))
        idx = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(255)))
        idx = np.where(v == np.float32(np.inf), np.float32(255), idx)
        idx = np.where(v == ninf, np.float32(0), idx).astype(np.int64)
        img[r * (H + gap):r * (H + gap) + H] = lut[idx]
    return img
