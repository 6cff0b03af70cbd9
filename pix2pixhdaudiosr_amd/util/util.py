"""Host-side helpers of the hot path with the reference's names (util/util.py)."""
import os

import numpy as np
import torch


def mkdir(path):
    """util/util.py:50-52 of the reference (options/base_options.py:100 and the visualizer call these)."""
    os.makedirs(path, exist_ok=True)


def mkdirs(paths):
    """util/util.py:43-48: one path or a list of them."""
    for p in ([paths] if isinstance(paths, str) else list(paths)):
        mkdir(p)


def tensor2im(image_tensor, imtype=np.uint8, normalize=True):
    """util/util.py:12-26: a [C, H, W] tensor (or a list of them) in [-1, 1] (`normalize`) or [0, 1] -> an [H, W, C] image
    array; a single channel, or more than three, gives the 2-D first channel."""
    if isinstance(image_tensor, list):
        return [tensor2im(t, imtype, normalize) for t in image_tensor]
    image_numpy = np.transpose(image_tensor.cpu().float().numpy(), (1, 2, 0))
    image_numpy = (image_numpy + 1) / 2.0 * 255.0 if normalize else image_numpy * 255.0
    image_numpy = np.clip(image_numpy, 0, 255)
    if image_numpy.shape[2] == 1 or image_numpy.shape[2] > 3:
        image_numpy = image_numpy[:, :, 0]
    return image_numpy.astype(imtype)


def save_image(image_numpy, image_path):
    """util/util.py:39-41 (the reference's Visualizer calls it, util/visualizer.py:61-64,126).  uint8 arrays -- what
    tensor2im and the reference's matplotlib renderings give -- are written as they are.  `get_current_visuals` of this
    build returns the plotted data itself, 2-D float arrays, which no 8-bit image format holds: those are min-max scaled
    to uint8 first."""
    from PIL import Image
    a = np.asarray(image_numpy)
    if a.dtype != np.uint8:
        a = a.astype(np.float64)
        lo, hi = (float(a.min()), float(a.max())) if a.size else (0.0, 0.0)
        a = np.round((a - lo) * (255.0 / (hi - lo) if hi > lo else 0.0)).astype(np.uint8)
    Image.fromarray(a).save(image_path)


def kbdwin(N: int, beta: float = 12.0, device='cpu') -> torch.Tensor:
    """MATLAB-style Kaiser-Bessel-derived window, same arithmetic as util/util.py:186-193
    of the reference (a one-off host constant: the kernels only read it)."""
    assert N % 2 == 0, "N must be even"
    w = torch.kaiser_window(window_length=N // 2 + 1, beta=beta * torch.pi, periodic=False, device=device)
    w_sum = w.sum()
    wdw_half = torch.sqrt(torch.cumsum(w, dim=0) / w_sum)[:-1]
    return torch.cat((wdw_half, wdw_half.flip(dims=(0,))), dim=0)


def lowband_keep_rows(bins, up_ratio):
    """Rows of a `bins`-row spectrogram that the low-rate input carried: util/util.py:113 of the reference (all of them at
    up_ratio <= 1)."""
    return int(bins * (1 / up_ratio)) if up_ratio > 1 else int(bins)


def check_lowband_fade(lowband_fade, keep, who="imdct"):
    """The fade of the low-band splice is a whole number of rows in [0, keep]; returns it as an int."""
    if isinstance(lowband_fade, bool) or not isinstance(lowband_fade, (int, np.integer)):
        raise ValueError(f"{who}: lowband_fade must be an int (rows), got {lowband_fade!r}")
    if not 0 <= lowband_fade <= keep:
        raise ValueError(f"{who}: lowband_fade {lowband_fade} outside [0, {keep}] (the rows the input carried)")
    return int(lowband_fade)


def imdct(spectro, pha, norm_param, _imdct, min_value=1e-7, up_ratio=1, explicit_encoding=False, lr_spectro=None, lowband_fade=0):
    """Generation tail of the reference (util/util.py:104-131, caller generate_audio.py:40-42): de-normalise, dB ->
    amplitude, restore the sign (LR sign on the low band, sign(ch0 - ch1) -- or a random sign without explicit
    encoding -- above it), and run the inverse transform `_imdct` on [B, frames, bins]; returns `_imdct(.) / 2`.
    One HIP launch (p2phd_spectro_decode_signed) replaces the elementwise chain and the permute.

    `lr_spectro` (default None: the chain above, unchanged): the input's own encoding, shaped like `spectro` and under the same
    `norm_param` -- the fourth value of `model.inference`.  The rows below `keep = int(M / up_ratio)`, whose sign already
    comes from the input, then take their amplitude from it as well (p2phd_spectro_decode_spliced): rows < keep -
    lowband_fade are the input's, rows >= keep the generator's, and the `lowband_fade` rows between cross-fade the two
    decoded values with the input's weight cos^2(pi (j + 1/2) / (2 lowband_fade)).  This rests on one fact: the mask noise of
    `to_spectro` fills the top int(M * (1 - 1 / up_ratio)) rows, and M - int(M * (1 - 1 / up_ratio)) >= int(M / up_ratio)
    = keep, so every noise row is a row >= keep and the spliced rows of `lr_spectro` never hold noise.  With up_ratio <= 1
    keep = M: every row is the input's, and the result is the input's own transform round trip.

    A `norm_param` with 'rows' (the [B, 8] table of `to_spectro(..., norm='rows')`, one range per row) goes through the same two
    kernels with row b's (min, max) read at rows[b, 0:2] (p2phd_spectro_decode_signed_rows, p2phd_spectro_decode_spliced_rows)."""
    from .. import _lib
    dev = spectro.device
    _lib.require_gpu_tensor(spectro, "spectro")
    x = spectro.float()
    if x.dim() == 3:
        x = x.unsqueeze(1)
    x = x.contiguous()
    B, Cc, M, Fr = x.shape
    if explicit_encoding and Cc != 2:
        raise ValueError(f"imdct: explicit encoding needs 2 channels, got {Cc}")
    if not explicit_encoding and Cc != 1:
        raise ValueError(f"imdct: plain encoding needs 1 channel, got {Cc}")
    p = pha.to(dev).float().reshape(-1, M, Fr)
    if p.shape[0] != B:
        raise ValueError(f"imdct: pha batch {p.shape[0]} != spectro batch {B}")
    keep = int(M * (1 / up_ratio)) if up_ratio > 1 else M
    lr = None
    if lr_spectro is not None:
        if not isinstance(lr_spectro, torch.Tensor) or not lr_spectro.is_cuda:
            raise _lib.P2PHDError("lr_spectro: expected a tensor on the GPU (this build has no CPU path)")
        lr = lr_spectro.float()
        if lr.dim() == 3:
            lr = lr.unsqueeze(1)
        if lr.shape != x.shape:
            raise ValueError(f"imdct: lr_spectro shape {tuple(lr.shape)} != spectro shape {tuple(x.shape)}")
        lr = lr.contiguous()
        fade = check_lowband_fade(lowband_fade, keep)
    if not explicit_encoding and keep < M:
        pseudo = (2 * torch.randint(low=0, high=2, size=(B, M, Fr), device=dev) - 1).float()
        p = torch.cat((p[:, :keep], pseudo[:, keep:]), dim=1)
    p = p.contiguous()
    rows = norm_param.get('rows') if isinstance(norm_param, dict) else None
    if rows is not None:                                                    # one range per row: to_spectro(..., norm='rows')
        if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.float32 or tuple(rows.shape) != (B, 8):
            raise ValueError(f"imdct: norm_param['rows'] must be a float32 tensor [{B}, 8] on the GPU, got "
                             f"{tuple(rows.shape) if isinstance(rows, torch.Tensor) else rows!r}")
        rows = rows.contiguous()
        spec = torch.empty((B, Fr, M), dtype=torch.float32, device=dev)
        if lr is not None:
            _lib.check(_lib.lib().p2phd_spectro_decode_spliced_rows(_lib.ptr(x), _lib.ptr(lr), _lib.ptr(p), _lib.ptr(rows), B, Fr, M, Cc,
                                                                    keep, fade, float(min_value), 1.0, _lib.ptr(spec), _lib.stream_ptr()),
                       "spectro_decode_spliced_rows")
        else:
            _lib.check(_lib.lib().p2phd_spectro_decode_signed_rows(_lib.ptr(x), _lib.ptr(p), _lib.ptr(rows), B, Fr, M, Cc, keep,
                                                                   float(min_value), 1.0, _lib.ptr(spec), _lib.stream_ptr()),
                       "spectro_decode_signed_rows")
        return _imdct(spec) / 2
    mm = torch.stack([torch.as_tensor(norm_param['min']).float().reshape(()),
                      torch.as_tensor(norm_param['max']).float().reshape(())]).to(dev).contiguous()
    spec = torch.empty((B, Fr, M), dtype=torch.float32, device=dev)
    if lr is not None:
        _lib.check(_lib.lib().p2phd_spectro_decode_spliced(_lib.ptr(x), _lib.ptr(lr), _lib.ptr(p), _lib.ptr(mm), B, Fr, M, Cc, keep,
                                                           fade, float(min_value), 1.0, _lib.ptr(spec), _lib.stream_ptr()),
                   "spectro_decode_spliced")
        return _imdct(spec) / 2
    _lib.check(_lib.lib().p2phd_spectro_decode_signed(_lib.ptr(x), _lib.ptr(p), _lib.ptr(mm), B, Fr, M, Cc, keep,
                                                      float(min_value), 1.0, _lib.ptr(spec), _lib.stream_ptr()),
               "spectro_decode_signed")
    return _imdct(spec) / 2


_STFT_TABLES = {}


def _stft_tables(n2, device):
    from .. import _lib
    key = (n2, str(device))
    if key not in _STFT_TABLES:
        host = torch.empty(_lib.lib().p2phd_stft_tables_floats(n2), dtype=torch.float32)
        _lib.check(_lib.lib().p2phd_stft_tables_fill(n2, _lib.ptr(host)), "stft_tables_fill")
        _STFT_TABLES[key] = host.to(device)
    return _STFT_TABLES[key]


def audio_metrics(hr_audio, lr_audio, sr_audio, n_fft, hop_length, win_length, center=True):
    """Device-side compute_matrics: returns (result4 tensor [mse, snr_sr, snr_lr, lsd] on the GPU, sr moment-matched to
    hr).  No host synchronisation; `compute_matrics` below is the reference-shaped wrapper."""
    from .. import _lib
    _lib.require_gpu_tensor(sr_audio, "sr_audio")
    dev = sr_audio.device
    T = sr_audio.shape[-1]
    sr = sr_audio.float().reshape(-1, T).contiguous()
    hr = hr_audio.to(dev).float().reshape(-1, T).contiguous()
    lr = lr_audio.to(dev).float().reshape(-1, T).contiguous()
    if hr.shape != sr.shape or lr.shape != sr.shape:
        raise ValueError(f"compute_matrics: shapes differ: hr {tuple(hr.shape)} lr {tuple(lr.shape)} sr {tuple(sr.shape)}")
    B = sr.shape[0]
    n2, hop2, win2 = 2 * int(n_fft), 2 * int(hop_length), 2 * int(win_length)
    window2 = kbdwin(win2).to(dev).contiguous()
    L = _lib.lib()
    nbytes = L.p2phd_metrics_workspace_bytes(B, T, n2, hop2, win2, int(bool(center)))
    if nbytes == 0:
        raise _lib.P2PHDError("compute_matrics: " + L.p2phd_last_error().decode("utf-8", "replace"))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    matched = torch.empty_like(sr)
    result = torch.empty(4, dtype=torch.float32, device=dev)
    _lib.check(L.p2phd_audio_metrics(_lib.ptr(hr), _lib.ptr(lr), _lib.ptr(sr), B, T, n2, hop2, win2, _lib.ptr(window2),
                                     _lib.ptr(_stft_tables(n2, dev)), int(bool(center)), _lib.ptr(matched), _lib.ptr(result),
                                     _lib.ptr(ws), _lib.stream_ptr()), "audio_metrics")
    return result, matched.reshape(sr_audio.shape)


def compute_matrics(hr_audio, lr_audio, sr_audio, opt):
    """MSE / SNR / LSD of the reference (util/util.py:133-184); same 7-tuple `(mse, snr_sr, snr_lr, 0, 0, 0, lsd)` of
    Python floats (the segmental-SNR and PESQ slots are constant zeros there too)."""
    result, _ = audio_metrics(hr_audio, lr_audio, sr_audio, opt.n_fft, opt.hop_length, opt.win_length, opt.center)
    mse, snr_sr, snr_lr, lsd = result.tolist()
    return mse, snr_sr, snr_lr, 0, 0, 0, lsd


METRIC_ROW_NAMES = ("mse", "snr_sr", "snr_lr", "lsd", "lsd_lf", "lsd_hf", "ssnr_sr", "ssnr_lr")


def metric_rows_geometry(n_fft, hr_sampling_rate, lr_sampling_rate):
    """(cut_bin, seg_win, seg_hop) of audio_metrics_rows.  cut_bin: the bin of the low rate's Nyquist frequency in the
    2*n_fft-point STFT -- the first bin of the high band (equal rates: n_fft, the high band is the Nyquist bin alone).
    Segments of 30 ms every quarter of that (240 / 60 samples at 8 kHz, 1440 / 360 at 48 kHz)."""
    hr_rate, lr_rate = int(hr_sampling_rate), int(lr_sampling_rate)
    cut_bin = (2 * int(n_fft) * lr_rate) // (2 * hr_rate)
    return cut_bin, int(round(0.03 * hr_rate)), int(np.floor(0.25 * 0.03 * hr_rate))


def audio_metrics_rows(hr_audio, lr_audio, sr_audio, n_fft, hop_length, win_length, center, hr_sampling_rate, lr_sampling_rate):
    """Per-row metrics on the device: returns (rows [B, 8] float32 on the GPU, columns METRIC_ROW_NAMES, every row measured on
    its own; sr moment-matched to hr).  One call for any number of rows, no host synchronisation.  Beside the four figures of
    `audio_metrics` a row holds the LSD of the bins below / from the low rate's Nyquist frequency (lsd_lf, lsd_hf) and the
    segmental SNR of sr and lr (NaN for a row shorter than one segment and one hop); definitions: csrc/metrics.hip."""
    from .. import _lib
    _lib.require_gpu_tensor(sr_audio, "sr_audio")
    dev = sr_audio.device
    T = sr_audio.shape[-1]
    sr = sr_audio.float().reshape(-1, T).contiguous()
    hr = hr_audio.to(dev).float().reshape(-1, T).contiguous()
    lr = lr_audio.to(dev).float().reshape(-1, T).contiguous()
    if hr.shape != sr.shape or lr.shape != sr.shape:
        raise ValueError(f"audio_metrics_rows: shapes differ: hr {tuple(hr.shape)} lr {tuple(lr.shape)} sr {tuple(sr.shape)}")
    B = sr.shape[0]
    n2, hop2, win2 = 2 * int(n_fft), 2 * int(hop_length), 2 * int(win_length)
    cut_bin, seg_win, seg_hop = metric_rows_geometry(n_fft, hr_sampling_rate, lr_sampling_rate)
    window2 = kbdwin(win2).to(dev).contiguous()
    L = _lib.lib()
    nbytes = L.p2phd_metrics_rows_workspace_bytes(B, T, n2, hop2, win2, int(bool(center)), cut_bin, seg_win, seg_hop)
    if nbytes == 0:
        raise _lib.P2PHDError("audio_metrics_rows: " + L.p2phd_last_error().decode("utf-8", "replace"))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    matched = torch.empty_like(sr)
    rows = torch.empty((B, len(METRIC_ROW_NAMES)), dtype=torch.float32, device=dev)
    _lib.check(L.p2phd_audio_metrics_rows(_lib.ptr(hr), _lib.ptr(lr), _lib.ptr(sr), B, T, n2, hop2, win2, _lib.ptr(window2),
                                          _lib.ptr(_stft_tables(n2, dev)), int(bool(center)), cut_bin, seg_win, seg_hop,
                                          _lib.ptr(matched), _lib.ptr(rows), _lib.ptr(ws), _lib.stream_ptr()), "audio_metrics_rows")
    return rows, matched.reshape(sr_audio.shape)


def compute_matrics_ext(hr_audio, lr_audio, sr_audio, opt):
    """The eight per-row figures as Python floats: a list with one dict (METRIC_ROW_NAMES -> float) per row of the inputs, from
    one device call and one copy to the host.  `compute_matrics` above keeps the reference's 7-tuple and its zeros."""
    rows, _ = audio_metrics_rows(hr_audio, lr_audio, sr_audio, opt.n_fft, opt.hop_length, opt.win_length, opt.center,
                                 opt.hr_sampling_rate, opt.lr_sampling_rate)
    return [dict(zip(METRIC_ROW_NAMES, row)) for row in rows.tolist()]
