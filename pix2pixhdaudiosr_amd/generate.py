"""Whole-file super-resolution: wav in, wav out, on the device from the waveform to the waveform.

    python -m pix2pixhdaudiosr_amd.generate --input in.wav --output out.wav --load_pretrain DIR [--overlap 0.25]
    python -m pix2pixhdaudiosr_amd.generate --input DIR_IN --output DIR_OUT --load_pretrain DIR --channels all [--metrics_csv m.csv [--metrics_ext]]

    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver(model, opt).enhance_file("in.wav", "out.wav")["sr"]

The chain is the reference's generate_audio.py:27-47 -- segments of `opt.segment_length` samples, `model.inference` and
`util.imdct` per group of `batchSize` segments, the pieces put back together and scaled by sqrt(up_ratio - 1) -- with two
differences.  The segments are cut and joined by two kernels (csrc/stitch.hip), and by default neighbours share
`overlap * segment_length` samples that are cross-faded, where the reference butts the pieces together.  `overlap=0` is the
reference's chain exactly, its amplitude included: with MDCT2 the reference's output is half of sqrt(up_ratio - 1) * x,
because its util.imdct halves what IMDCT2 already returns at unit gain.  With overlapping segments the pipeline returns the
full amplitude -- 6 dB more; `SuperResolver(reference_amplitude=...)` and `--reference_amplitude 0|1` choose explicitly.

A group is semantics: `to_spectro` normalises by the min / max of the whole batch tensor (pix2pixHD_model.py:165-168 of the
reference), so a group holds exactly the segments the reference's loader would put in it and a last, smaller group runs at
its own size -- padding it with silent segments would change its normalisation.  For the same reason a channel of a file is
a clip of its own: a group never mixes channels, and channel c of a [C, L] clip is grouped exactly as the mono clip audio[c].

The two ends of the file path run on the device as well (csrc/pcm.hip): the data chunk of the input goes up as bytes and is
decoded there, the output is encoded there and comes back as the payload to write; the host only moves bytes.

The output stage is opt-in and on the device too: `--report_peaks` (peak, clipped and non-finite samples per channel),
`--clip guard [--ceiling_dbfs X]` (one gain for the whole file so that nothing clips), `--clip error` (refuse to write a
file that would clip) and `--dither tpdf` (PCM16).  Without them every byte written and every line printed is as before:
the integer encodings clamp, silently.

`--crossover input` (opt-in, csrc/xover.hip) puts a time-domain crossover behind the stitch: a linear-phase complementary
filter pair, so that below `--crossover_hz` (default: 0.95 of the low rate's Nyquist frequency) the written clip is the input
and above it the generator's output.
"""
import argparse
import ast
import math
import os
import struct
import sys
from types import SimpleNamespace

import torch


def segment_plan(L, T, overlap=0.0):
    """(S, stride, V) for a clip of L samples: segments of T samples that start every `stride = T - V` samples,
    `V = int(overlap * T)` of them shared with the next one, `S = max(1, ceil((L - V) / stride))` segments -- the fewest
    whose span (S - 1) * stride + T reaches L.  overlap 0: ceil(L / T), the count of the reference's seg_pad_audio."""
    L, T = int(L), int(T)
    if T < 1 or L < 0:
        raise ValueError("segment_plan: need segment_length >= 1 and a length >= 0, got %d and %d" % (T, L))
    if not 0.0 <= overlap <= 0.5:
        raise ValueError("segment_plan: overlap must be in [0, 0.5], got %r" % (overlap,))
    V = int(overlap * T)
    stride = T - V
    S = max(1, -((V - L) // stride))
    return S, stride, V


def segments_gather(audio, T, stride, S):
    """audio [L] f32 on the GPU -> [S, T]: row s holds audio[s * stride : s * stride + T], zeros beyond the end."""
    from . import _lib
    a = _lib.require_gpu_tensor(audio, "segments_gather: audio", torch.float32)
    if a.dim() != 1:
        raise ValueError("segments_gather: expected a 1-D waveform, got shape %s" % (tuple(a.shape),))
    out = torch.empty((max(int(S), 0), max(int(T), 0)), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().p2phd_segments_gather(_lib.ptr(a), a.numel(), int(T), int(stride), int(S), _lib.ptr(out),
                                                _lib.stream_ptr()), "segments_gather")
    return out


def segments_stitch(seg, stride, gain=1.0, out_length=None):
    """seg [S, T] f32 on the GPU -> [out_length] (default: the whole span): gain * the segments laid `stride` apart, the
    T - stride shared samples of neighbours cross-faded with sin^2 / cos^2 weights."""
    from . import _lib
    s = _lib.require_gpu_tensor(seg, "segments_stitch: seg", torch.float32)
    if s.dim() != 2:
        raise ValueError("segments_stitch: expected [S, T], got shape %s" % (tuple(s.shape),))
    S, T = s.shape
    L_out = (S - 1) * int(stride) + T if out_length is None else int(out_length)
    out = torch.empty((max(L_out, 0),), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_segments_stitch(_lib.ptr(s), S, T, int(stride), float(gain), _lib.ptr(out), L_out,
                                                _lib.stream_ptr()), "segments_stitch")
    return out


def _rows(t, name):
    """A [C, L] f32 GPU tensor whose rows are contiguous (a row pitch >= L is fine) -> (tensor, C, L, pitch)."""
    from . import _lib
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise _lib.P2PHDError("%s: expected a float32 tensor on the GPU (this build has no CPU path)" % name)
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError("%s: expected [C, L] with C >= 1, got shape %s" % (name, tuple(t.shape)))
    C, L = t.shape
    if L > 1 and t.stride(1) != 1 or C > 1 and t.stride(0) < L:
        raise _lib.P2PHDError("%s: expected rows that are contiguous" % name)
    return t, C, L, (t.stride(0) if C > 1 else max(L, 1))


def segments_gather_planar(audio, T, stride, S):
    """audio [C, L] f32 on the GPU (rows contiguous, any row pitch) -> [C * S, T], channel-major: row c * S + s holds
    audio[c, s * stride : s * stride + T], zeros beyond the end.  One launch whatever C is."""
    from . import _lib
    a, C, L, ld = _rows(audio, "segments_gather_planar: audio")
    out = torch.empty((C * max(int(S), 0), max(int(T), 0)), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().p2phd_segments_gather_planar(_lib.ptr(a), C, max(ld, L), L, int(T), int(stride), int(S), _lib.ptr(out),
                                                       _lib.stream_ptr()), "segments_gather_planar")
    return out


def segments_stitch_planar(seg, C, stride, gain=1.0, out_length=None, ld=None):
    """seg [C * S, T] f32 on the GPU, channel-major -> [C, out_length]: segments_stitch on every channel's S rows, in one
    launch.  `ld`: row pitch of the buffer the result is a view of (default: out_length)."""
    from . import _lib
    s = _lib.require_gpu_tensor(seg, "segments_stitch_planar: seg", torch.float32)
    C = int(C)
    if s.dim() != 2 or C < 1 or s.shape[0] % C:
        raise ValueError("segments_stitch_planar: expected [C * S, T] with C = %d, got shape %s" % (C, tuple(s.shape)))
    S, T = s.shape[0] // C, s.shape[1]
    L_out = (S - 1) * int(stride) + T if out_length is None else int(out_length)
    ld = max(L_out, 0) if ld is None else int(ld)
    out = torch.empty((C, max(ld, 0)), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_segments_stitch_planar(_lib.ptr(s), C, S, T, int(stride), float(gain), _lib.ptr(out), ld, L_out,
                                                       _lib.stream_ptr()), "segments_stitch_planar")
    return out[:, :max(L_out, 0)]


# (format tag, bits per sample) of a RIFF fmt chunk -> P2PHD_PCM_* code of include/p2phd.h: the set wavio.info accepts
PCM_FORMATS = {(1, 8): 0, (1, 16): 1, (1, 24): 2, (1, 32): 3, (3, 32): 4, (3, 64): 5}
# encoding of wavio.save / wavio.write_payload -> (P2PHD_PCM_* code, bytes per sample)
PCM_ENCODINGS = {'pcm16': (1, 2), 'pcm24': (2, 3), 'float32': (4, 4)}


def pcm_decode(payload, frames, channels, format_tag, bits):
    """payload: uint8 tensor on the GPU holding the interleaved little-endian samples of a data chunk (any byte offset into
    its storage) -> [channels, frames] f32, bit-identical to what wavio.load returns for the file."""
    from . import _lib
    b = _lib.require_gpu_tensor(payload, "pcm_decode: payload", torch.uint8)
    fmt = PCM_FORMATS.get((int(format_tag), int(bits)))
    if fmt is None:
        raise ValueError("pcm_decode: unsupported format (tag %s, %s bit)" % (format_tag, bits))
    frames, channels = int(frames), int(channels)
    if b.numel() < frames * channels * (int(bits) // 8):
        raise ValueError("pcm_decode: %d bytes do not hold %d frames of %d x %d bit" % (b.numel(), frames, channels, bits))
    out = torch.empty((channels, frames), dtype=torch.float32, device=b.device)
    _lib.check(_lib.lib().p2phd_pcm_decode(_lib.ptr(b), frames, channels, fmt, _lib.ptr(out), frames, _lib.stream_ptr()), "pcm_decode")
    return out


def pcm_encode(waveform, encoding='pcm16', gain=None, dither=None, seed=0, first_index=0):
    """waveform [C, L] f32 on the GPU (rows contiguous) -> uint8 tensor of L * C samples, interleaved: the payload
    wavio.write_payload takes.  'pcm16' gives the bytes wavio.save writes; NaN encodes as 0 in the integer formats.
    `gain`: a float32 tensor of one element on the GPU (pcm_peaks' fourth value) that the kernel reads: every sample is
    multiplied by it first.  `dither`: None or 'tpdf' (pcm16 only): +-1 LSB of triangular noise in front of the rounding,
    a hash of (`seed`, `first_index` + the sample's index in the payload) -- encoding a clip in pieces with the right
    `first_index` gives the bytes of one call.  With none of the four given: p2phd_pcm_encode, as ever."""
    from . import _lib
    if encoding not in PCM_ENCODINGS:
        raise ValueError("pcm_encode: encoding must be one of %s, got %r" % (sorted(PCM_ENCODINGS), encoding))
    w, C, L, ld = _rows(waveform, "pcm_encode: waveform")
    fmt, nbytes = PCM_ENCODINGS[encoding]
    out = torch.empty((L * C * nbytes,), dtype=torch.uint8, device=w.device)
    if gain is None and dither is None and seed == 0 and first_index == 0:
        _lib.check(_lib.lib().p2phd_pcm_encode(_lib.ptr(w), L, C, max(ld, L), fmt, _lib.ptr(out), _lib.stream_ptr()), "pcm_encode")
        return out
    check_dither(dither, encoding, "pcm_encode")
    if gain is not None:
        gain = _lib.require_gpu_tensor(gain, "pcm_encode: gain", torch.float32)
        if gain.numel() != 1:
            raise ValueError("pcm_encode: gain must hold one value, got shape %s" % (tuple(gain.shape),))
    if int(first_index) < 0:
        raise ValueError("pcm_encode: first_index must be >= 0, got %r" % (first_index,))
    _lib.check(_lib.lib().p2phd_pcm_encode_ex(_lib.ptr(w), L, C, max(ld, L), fmt, _lib.ptr(gain), 1 if dither else 0,
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index), _lib.ptr(out), _lib.stream_ptr()),
               "pcm_encode_ex")
    return out


DITHERS = (None, 'tpdf')
CLIP_MODES = ('clamp', 'guard', 'error')


def check_dither(dither, encoding, who):
    if dither not in DITHERS:
        raise ValueError("%s: dither must be None or 'tpdf', got %r" % (who, dither))
    if dither is not None and encoding != 'pcm16':
        raise ValueError("%s: dither is for pcm16 (a 24-bit or float32 file carries the signal's own low bits), got encoding %r"
                         % (who, encoding))


def encoding_limit(encoding):
    """The largest sample value the encoding holds: (2^(bits-1) - 1) / 2^(bits-1) for the integer ones, 1 for float32."""
    half = {'pcm16': 32768.0, 'pcm24': 8388608.0}.get(encoding)
    return 1.0 if half is None else (half - 1.0) / half


def ceiling_from_dbfs(ceiling_dbfs, encoding):
    """The `ceiling` of pcm_peaks for a level in dBFS (<= 0): 10^(dB / 20), or None -- the encoding's own limit -- where
    that is not below the limit (or no level is given)."""
    if ceiling_dbfs is None:
        return None
    level = 10.0 ** (float(ceiling_dbfs) / 20.0)
    return level if level < encoding_limit(encoding) else None


def _pcm_peaks_packed(waveform, encoding, ceiling, who):
    """-> (the four results of pcm_peaks as views of one byte buffer, the buffer): one copy brings all of them back."""
    from . import _lib
    if encoding not in PCM_ENCODINGS:
        raise ValueError("%s: encoding must be one of %s, got %r" % (who, sorted(PCM_ENCODINGS), encoding))
    ceiling = 0.0 if ceiling is None else float(ceiling)
    if not ceiling >= 0.0 or ceiling == float('inf'):
        raise ValueError("%s: ceiling must be a finite level > 0, or None for the encoding's own limit, got %r" % (who, ceiling))
    w, C, L, ld = _rows(waveform, "%s: waveform" % who)
    buf = torch.empty((20 * C + 4,), dtype=torch.uint8, device=w.device)       # over[C] i64 | nonfinite[C] i64 | peak[C] f32 | gain f32
    over, nonfinite = buf[:8 * C].view(torch.int64), buf[8 * C:16 * C].view(torch.int64)
    peak, gain = buf[16 * C:20 * C].view(torch.float32), buf[20 * C:].view(torch.float32)
    _lib.check(_lib.lib().p2phd_pcm_peak(_lib.ptr(w), L, C, max(ld, L), PCM_ENCODINGS[encoding][0], ceiling, _lib.ptr(peak),
                                         _lib.ptr(over), _lib.ptr(nonfinite), _lib.ptr(gain), _lib.stream_ptr()), "pcm_peak")
    return (peak, over, nonfinite, gain), buf


def pcm_peaks(waveform, encoding='pcm16', ceiling=None):
    """What `encoding` would meet in waveform [C, L] f32 on the GPU (rows contiguous) -> (peak [C] f32, over [C] i64,
    nonfinite [C] i64, gain [1] f32), all on the GPU, nothing waited for: per channel the largest |x| among the finite samples,
    the number of samples the encoder would clamp (above the encoding's limit or below -1; beyond +-1 for float32) and the
    number of NaN / inf samples; and the one gain for all channels that brings the largest peak down to `ceiling` (a linear
    level; None: the encoding's limit) -- 1 where it already is.  The same bits on every run."""
    return _pcm_peaks_packed(waveform, encoding, ceiling, "pcm_peaks")[0]


def check_output_options(encoding, clip='clamp', ceiling_dbfs=None, dither=None, dither_seed=0, report_peaks=False, who="enhance_file"):
    """Validates the output-stage options; -> None when all of them are at their defaults (the plain encoder runs and
    nothing is reported), else a dict {'clip', 'ceiling' (linear, or None), 'dither', 'seed', 'report'}."""
    if encoding not in PCM_ENCODINGS:
        raise ValueError("%s: encoding must be one of %s, got %r" % (who, sorted(PCM_ENCODINGS), encoding))
    if clip not in CLIP_MODES:
        raise ValueError("%s: clip must be one of %s, got %r" % (who, CLIP_MODES, clip))
    check_dither(dither, encoding, who)
    if ceiling_dbfs is not None:
        if isinstance(ceiling_dbfs, bool) or not isinstance(ceiling_dbfs, (int, float)) or not -1000.0 <= ceiling_dbfs <= 0.0:
            raise ValueError("%s: ceiling_dbfs must be a level <= 0 dBFS, got %r" % (who, ceiling_dbfs))
        if clip != 'guard':
            raise ValueError("%s: ceiling_dbfs is the level clip='guard' scales to; clip is %r" % (who, clip))
    if isinstance(dither_seed, bool) or not isinstance(dither_seed, int):
        raise ValueError("%s: dither_seed must be an int, got %r" % (who, dither_seed))
    if clip == 'clamp' and ceiling_dbfs is None and dither is None and dither_seed == 0 and not report_peaks:
        return None
    return {'clip': clip, 'ceiling': ceiling_from_dbfs(ceiling_dbfs, encoding), 'dither': dither, 'seed': dither_seed,
            'report': bool(report_peaks)}


def _dbfs(level):
    return 20.0 * math.log10(level) if level > 0.0 else float('-inf')


def select_channels(channels, available):
    """How many leading channels of a file with `available` channels are enhanced and written: 'first' -> 1, 'all' -> every
    one, an int N -> the first N (all of them where the file has fewer)."""
    if channels == 'first':
        return 1
    if channels == 'all':
        return int(available)
    if isinstance(channels, bool) or not isinstance(channels, int) or channels < 1:
        raise ValueError("channels must be 'first', 'all' or an int >= 1, got %r" % (channels,))
    return min(channels, int(available))


LOWBANDS = ('model', 'input')


def check_lowband(lowband, lowband_fade, bins, up_ratio):
    """Validates the low-band options of SuperResolver for a spectrogram of `bins` rows: `lowband` is 'model' or 'input' and
    `lowband_fade` a whole number of rows in [0, keep], keep = int(bins / up_ratio) -- the rows the low-rate input carried
    (all of them at up_ratio <= 1).  Returns (lowband, lowband_fade, keep)."""
    from .util.util import check_lowband_fade, lowband_keep_rows
    if lowband not in LOWBANDS:
        raise ValueError("SuperResolver: lowband must be 'model' or 'input', got %r" % (lowband,))
    keep = lowband_keep_rows(bins, up_ratio)
    return lowband, check_lowband_fade(lowband_fade, keep, "SuperResolver"), keep


CROSSOVERS = (None, 'input')
CROSSOVER_BETA = 8.96                                                       # Kaiser window, 90 dB
CROSSOVER_ATTEN_DB = 90.0
CROSSOVER_MAX_TAPS = 4095


def crossover_width_hz(hr_rate, taps):
    """Transition width of a Kaiser-windowed sinc of `taps` coefficients at 90 dB (Kaiser's formula), in Hz at `hr_rate`."""
    return float('inf') if taps <= 1 else (CROSSOVER_ATTEN_DB - 7.95) * hr_rate / (14.36 * (taps - 1))


def crossover_plan(hr_rate, lr_rate, crossover_hz=None, taps=None):
    """The low-pass of the time-domain crossover, host arithmetic only -> (taps, cutoff, beta) for p2phd_xover_taps_fill:
    `cutoff` = crossover_hz / hr_rate (cycles per sample, the -6 dB point), beta = 8.96.  `crossover_hz` defaults to 0.95 of
    the low rate's Nyquist frequency; `taps` to the smallest odd count whose transition band, crossover_hz +- width / 2 with
    width = (90 - 7.95) * hr_rate / (14.36 * (taps - 1)), ends at or below that frequency -- everything the filter takes
    from the input is then something the input carried."""
    hr_rate, lr_rate = float(hr_rate), float(lr_rate)
    if not 0.0 < lr_rate < hr_rate:
        raise ValueError("crossover_plan: nothing to cross over: the low rate %g must be above 0 and below the high rate %g" % (lr_rate, hr_rate))
    nyquist = lr_rate / 2.0
    if crossover_hz is None:
        crossover_hz = 0.95 * nyquist
    crossover_hz = float(crossover_hz)
    if not 0.0 < crossover_hz < nyquist:
        raise ValueError("crossover_plan: crossover_hz must lie in (0, %g), below the low rate's Nyquist frequency, got %g" % (nyquist, crossover_hz))

    def fits(n):
        return crossover_hz + crossover_width_hz(hr_rate, n) / 2.0 <= nyquist

    if taps is None:
        # n - 1 >= width constant / (2 * room), then to the odd count next to it and to the exact edge of `fits`
        n = int(math.ceil((CROSSOVER_ATTEN_DB - 7.95) * hr_rate / (14.36 * 2.0 * (nyquist - crossover_hz)))) + 1
        n = max(3, min(n | 1, 2 ** 40 + 1))
        while n > 3 and fits(n - 2):
            n -= 2
        while not fits(n):
            n += 2
        if n > CROSSOVER_MAX_TAPS:
            raise ValueError("crossover_plan: a transition band from %g Hz that ends at %g Hz needs %d taps at %g Hz, more than %d: lower "
                             "crossover_hz" % (crossover_hz, nyquist, n, hr_rate, CROSSOVER_MAX_TAPS))
        taps = n
    else:
        if isinstance(taps, bool) or not isinstance(taps, int) or not 1 <= taps <= CROSSOVER_MAX_TAPS or taps % 2 == 0:
            raise ValueError("crossover_plan: taps must be an odd int in [1, %d], got %r" % (CROSSOVER_MAX_TAPS, taps))
        if not fits(taps):
            raise ValueError("crossover_plan: with %d taps the transition band is %g Hz wide and ends at %g Hz, above the low rate's Nyquist "
                             "frequency %g Hz: use more taps or a lower crossover_hz"
                             % (taps, crossover_width_hz(hr_rate, taps), crossover_hz + crossover_width_hz(hr_rate, taps) / 2.0, nyquist))
    return taps, crossover_hz / hr_rate, CROSSOVER_BETA


def crossover_coefficients(taps, cutoff, beta):
    """The coefficients of p2phd_xover_taps_fill as a float32 tensor on the host (no GPU needed)."""
    import ctypes
    from . import _lib
    h = torch.empty((max(int(taps), 1),), dtype=torch.float32)
    _lib.check(_lib.lib().p2phd_xover_taps_fill(int(taps), float(cutoff), float(beta), ctypes.c_void_p(h.data_ptr())), "xover_taps_fill")
    return h


def crossover(sr, lr, level, taps_dev):
    """sr, lr: [C, L] f32 on the GPU (rows contiguous, any row pitch), taps_dev: an odd number (<= 4095) of f32 coefficients on
    the GPU -> a new [C, L]: sr + LP * (level * lr - sr), the difference zero-extended beyond the clip (p2phd_xover_fwd)."""
    from . import _lib
    s, C, L, ld_s = _rows(sr, "crossover: sr")
    l, Cl, Ll, ld_l = _rows(lr, "crossover: lr")
    if (C, L) != (Cl, Ll):
        raise ValueError("crossover: sr and lr must have one shape, got %s and %s" % (tuple(s.shape), tuple(l.shape)))
    h = _lib.require_gpu_tensor(taps_dev, "crossover: taps_dev", torch.float32)
    if h.dim() != 1 or not 1 <= h.numel() <= CROSSOVER_MAX_TAPS or h.numel() % 2 == 0:
        raise ValueError("crossover: taps_dev must hold an odd number of coefficients in [1, %d], got shape %s" % (CROSSOVER_MAX_TAPS, tuple(h.shape)))
    out = torch.empty((C, L), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_xover_fwd(_lib.ptr(s), max(ld_s, L), _lib.ptr(l), max(ld_l, L), float(level), _lib.ptr(h), h.numel(), C, L,
                                          _lib.ptr(out), max(L, 1), _lib.stream_ptr()), "xover_fwd")
    return out


def check_crossover(crossover, crossover_hz, crossover_taps, hr_rate, lr_rate):
    """Validates the crossover options of SuperResolver -> None (off), or crossover_plan's (taps, cutoff, beta)."""
    if crossover not in CROSSOVERS:
        raise ValueError("SuperResolver: crossover must be None or 'input', got %r" % (crossover,))
    if crossover is None:
        if crossover_hz is not None or crossover_taps is not None:
            raise ValueError("SuperResolver: crossover_hz / crossover_taps are options of crossover='input'; crossover is None")
        return None
    return crossover_plan(hr_rate, lr_rate, crossover_hz, crossover_taps)


def plan_folder(dir_in, dir_out):
    """[(relative path, input path, output path)] of every *.wav under dir_in, recursive, sorted by relative path; the
    output keeps the relative path under dir_out.  Other files are ignored."""
    if not os.path.isdir(dir_in):
        raise NotADirectoryError("%s is not a directory" % dir_in)
    if os.path.exists(dir_out) and not os.path.isdir(dir_out):
        raise NotADirectoryError("--input is a directory, so --output must be one too: %s is a file" % dir_out)
    rel = []
    for root, _, files in os.walk(dir_in):
        for f in files:
            if f.lower().endswith('.wav'):
                rel.append(os.path.relpath(os.path.join(root, f), dir_in))
    return [(r, os.path.join(dir_in, r), os.path.join(dir_out, r)) for r in sorted(rel)]


class SuperResolver:
    """`model`: anything with `.inference(lr_audio, inst, noise=None) -> (sr_spectro, lr_pha, norm_param, lr_spectro)`
    (Pix2PixHDModel); its `mdct_type` picks the inverse transform.  `overlap`: shared fraction of a segment, [0, 0.5].
    `batch`: segments per group (default opt.batchSize).  `graph`: capture the chain of a full group once and replay it
    (options that draw random numbers inside the chain -- mask_mode 'mode1', the single-channel encodings -- run eagerly).
    `reference_amplitude` (mdct2 only): True keeps the amplitude of the reference's generate_audio.py, which is
    sqrt(up_ratio - 1) * x / 2 for a spectrogram that encodes x; False returns sqrt(up_ratio - 1) * x.  Default: True at
    overlap 0, the reference-exact mode, False with overlapping segments.
    `lowband`: 'model' (default) decodes every row of the generator's spectrogram; 'input' keeps the input's own low band:
    the rows below keep = int(bins / up_ratio), which the low-rate input carried, are decoded from the input's spectrogram
    (the fourth value of `inference`) and only the rows from keep come from the generator (util.imdct, `lr_spectro`).
    `lowband_fade`: rows below keep over which the two are cross-faded, 0 (a hard switch at keep) .. keep.  Both are fixed
    for the object's life, so the captured chain holds them.  With up_ratio <= 1 keep is every row: 'input' is accepted and
    returns the input's own transform round trip.
    `crossover`: None (default), or 'input': behind the stitch the clip goes through a time-domain crossover (csrc/xover.hip),
    out = sr + LP * ((gain / 2) * lr - sr) with LP a zero-delay Kaiser-windowed sinc: below `crossover_hz` (default 0.95 of the
    low rate's Nyquist frequency) the result is the input at the level the pipeline returns a passed-through signal at, above
    it the generator's output.  `crossover_taps`: the filter's length (odd, <= 4095; default: the shortest whose transition
    band ends under that Nyquist frequency, crossover_plan).  Fixed for the object's life; the coefficients are filled once and
    stay on the device.  One launch per clip, outside the captured chain; orthogonal to `lowband`.  Needs lr_sampling_rate <
    hr_sampling_rate."""

    def __init__(self, model, opt, overlap=0.25, batch=None, graph=True, reference_amplitude=None, lowband='model',
                 lowband_fade=0, crossover=None, crossover_hz=None, crossover_taps=None):
        from .models.mdct import IMDCT2, IMDCT4
        from .util import util as U
        self.model, self.opt = model, opt
        self.T = int(opt.segment_length)
        self.overlap = float(overlap)
        segment_plan(0, self.T, self.overlap)                               # validates both
        self.batch = int(batch if batch is not None else getattr(opt, 'batchSize', 1))
        if self.batch < 1:
            raise ValueError("SuperResolver: batch must be >= 1, got %d" % self.batch)
        self.graph = bool(graph)
        self.device = torch.device(getattr(model, 'device', None) or 'cuda')
        self.up_ratio = opt.hr_sampling_rate / opt.lr_sampling_rate
        self.mdct_type = getattr(model, 'mdct_type', None) or getattr(opt, 'mdct_type', None) or 'mdct4'
        kw = dict(window=U.kbdwin, win_length=opt.win_length, hop_length=opt.hop_length, n_fft=opt.n_fft,
                  center=getattr(opt, 'center', True), out_length=self.T, device=self.device)
        if self.mdct_type == 'mdct2':
            from .dct.dct import IDCT
            self._imdct = IMDCT2(idct_op=IDCT(), **kw)                      # generate_audio.py:23-25
        elif self.mdct_type == 'mdct4':
            self._imdct = IMDCT4(**kw)
        else:
            raise ValueError("SuperResolver: mdct_type must be 'mdct2' or 'mdct4', got %r" % (self.mdct_type,))
        if self.up_ratio < 1:
            raise ValueError("SuperResolver: lr_sampling_rate above hr_sampling_rate")
        bins = int(opt.n_fft) if self.mdct_type == 'mdct2' else int(opt.n_fft) // 2
        self.lowband, self.lowband_fade, _ = check_lowband(lowband, lowband_fade, bins, self.up_ratio)
        # Both inverse transforms return x for the spectrogram of x and util.imdct halves that (util/util.py:127 of the
        # reference), so the hand-composed chain is a factor 2 short of generate_audio.py:47's sqrt(up_ratio - 1) * x; the
        # stitch gain puts the factor back.  The reference's own output (MDCT2, back-to-back segments; tests/golden/generate.npz)
        # carries the halving, and overlap = 0 is the mode that reproduces the reference bit for bit: there -- and only for
        # mdct2, nothing of the reference runs MDCT4 -- the factor is left out, unless the caller decides otherwise.
        if reference_amplitude is None:
            reference_amplitude = self.overlap == 0.0
        self.reference_amplitude = bool(reference_amplitude) and self.mdct_type == 'mdct2'
        self.gain = math.sqrt(self.up_ratio - 1) * (1.0 if self.reference_amplitude else 2.0)
        # The inverse-transform chain returns x / 2 for the spectrogram of x and the stitch multiplies by `gain`: a signal the
        # generator passes through comes out as (gain / 2) * x, with or without reference_amplitude -- the level the input enters
        # the crossover at.
        self.crossover, self.crossover_hz, self.crossover_taps = crossover, crossover_hz, crossover_taps
        self.crossover_plan = check_crossover(crossover, crossover_hz, crossover_taps, opt.hr_sampling_rate, opt.lr_sampling_rate)
        self._xover_taps = None                                             # the coefficients on the device, filled at first use
        self._g = None                                                      # captured chain of a full group
        self._pins = {}                                                     # pinned host buffers of the file path, grow-only

    # -- one group ---------------------------------------------------------------------------------
    def noise_shape(self, b):
        """Shape of the mask noise `inference` draws for a group of b segments (the model's `mask_noise_shape`), or None when
        the model draws none."""
        f = getattr(self.model, 'mask_noise_shape', None)
        return f(b, self.T) if callable(f) else None

    def _graph_ok(self):
        """Random draws must stay outside the graph, or replay would repeat them: the mask noise is handed in, but mask_mode
        'mode1' draws signs and the single-channel phase encodings draw phase noise inside to_spectro.  Those options run eagerly."""
        o = self.opt
        if getattr(o, 'mask', False) and getattr(o, 'mask_mode', None) == 'mode1':
            return False
        if not getattr(o, 'explicit_encoding', False):
            return getattr(o, 'phase_encoding_mode', None) in (None, 'scale') and self.up_ratio <= 1     # (util.imdct's random sign)
        return True

    def _group(self, seg, noise):
        """[b, T] low-rate segments -> [b, T] generated ones, before the sqrt(up_ratio - 1) gain (generate_audio.py:34-44)."""
        from .util import util as U
        sr_spectro, lr_pha, norm_param, lr_spectro = self.model.inference(seg, None, noise=noise)
        splice = {} if self.lowband == 'model' else dict(lr_spectro=lr_spectro, lowband_fade=self.lowband_fade)
        audio = U.imdct(spectro=sr_spectro.abs(), pha=lr_pha.squeeze(1), norm_param=norm_param, _imdct=self._imdct,
                        up_ratio=self.up_ratio, explicit_encoding=bool(getattr(self.opt, 'explicit_encoding', False)), **splice)
        audio = audio.reshape(seg.shape[0], -1)
        if audio.shape[1] != self.T:
            raise ValueError("SuperResolver: segment_length %d does not come back from the transform (got %d samples): use "
                             "a multiple of hop_length" % (self.T, audio.shape[1]))
        return audio

    def _run_graphed(self, seg, noise):
        """The chain of a full group through a graph over static buffers.  The first use runs the chain once eagerly on the
        buffers (packed weights, tables and workspaces exist before capture), then captures it; every use replays.  Weights
        that changed since (load_network, an optimiser step) make the capture stale: it is redone."""
        from . import _ops
        g = self._g
        if g is None or g['epoch'] != _ops._WEIGHT_EPOCH[0]:
            shape = self.noise_shape(self.batch)
            g = self._g = {'epoch': _ops._WEIGHT_EPOCH[0], 'graph': None, 'out': None,
                           'seg': torch.empty((self.batch, self.T), dtype=torch.float32, device=self.device),
                           'noise': None if shape is None else torch.empty(shape, dtype=torch.float32, device=self.device)}
        g['seg'].copy_(seg)
        if g['noise'] is not None:
            g['noise'].copy_(noise)
        if g['graph'] is None:
            self._group(g['seg'], g['noise'])
            torch.cuda.synchronize()
            # as _train_step_graphed captures: a side stream behind the current (step) stream, thread-local capture mode,
            # no flush of the caching allocator
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                graph.capture_begin(capture_error_mode="thread_local")
                g['out'] = self._group(g['seg'], g['noise'])
                graph.capture_end()
            torch.cuda.current_stream().wait_stream(side)
            g['graph'] = graph
        g['graph'].replay()
        return g['out']

    # -- one clip ----------------------------------------------------------------------------------
    def enhance_lr(self, lr_audio, noise=None):
        """lr_audio: [C, L] or [L] on the GPU, already at the high rate -> the generated clip [C, L] ([1, L] for [L]).  Every
        channel is a clip of its own: its S segments are grouped as if it were a mono clip, so
        enhance_lr(x)[c] == enhance_lr(x[c:c+1])[0] given the same noise rows.  `noise`: the mask noise of all C * S segments,
        [C * S, channels, mask_rows, frames], channel-major, sliced per group; drawn per group (one torch.randn) when absent."""
        run = getattr(self.model, '_on_step_stream', None)
        with torch.no_grad():
            return run(self._enhance_lr, lr_audio, noise) if callable(run) else self._enhance_lr(lr_audio, noise)

    def _enhance_lr(self, lr_audio, noise):
        x = lr_audio.to(self.device).float()
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError("enhance_lr: expected a [C, L] or [L] waveform, got shape %s" % (tuple(lr_audio.shape),))
        x = x.contiguous()
        C, L = x.shape
        S, stride, V = segment_plan(L, self.T, self.overlap)
        seg = segments_gather_planar(x, self.T, stride, S)
        out = torch.empty_like(seg)
        for c in range(C):
            for s0 in range(0, S, self.batch):
                b = min(self.batch, S - s0)
                r0 = c * S + s0
                shape = self.noise_shape(b)
                nz = None
                if shape is not None:
                    nz = noise[r0:r0 + b] if noise is not None else torch.randn(shape, device=self.device)
                    if tuple(nz.shape) != shape:
                        raise ValueError("enhance_lr: noise for segments %d..%d of channel %d has shape %s, expected %s"
                                         % (s0, s0 + b - 1, c, tuple(nz.shape), shape))
                if self.graph and b == self.batch and self._graph_ok():
                    out[r0:r0 + b].copy_(self._run_graphed(seg[r0:r0 + b], nz))
                else:
                    out[r0:r0 + b].copy_(self._group(seg[r0:r0 + b], nz))
        sr = segments_stitch_planar(out, C, stride, self.gain, L)
        if self.crossover_plan is None:
            return sr
        if self._xover_taps is None:
            self._xover_taps = crossover_coefficients(*self.crossover_plan).to(self.device)
        return crossover(sr, x, self.gain / 2.0, self._xover_taps)

    # -- files -------------------------------------------------------------------------------------
    def _pinned(self, slot, nbytes):
        """Grow-only pinned byte buffer `slot`, free to be overwritten: the copy that last read it has finished.  Allocating
        one goes through the HIP runtime: call from the thread that owns the device."""
        t, busy = self._pins.get(slot, (None, None))
        if busy is not None:
            busy.synchronize()
        if t is None or t.numel() < nbytes:
            t = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, pin_memory=True)
        self._pins[slot] = (t, None)
        return t

    def _read(self, path, slot='in0'):
        """Host I/O only: the file's data chunk into pinned buffer `slot` -> (the bytes as a host tensor, WavInfo)."""
        from .data import wavio
        payload, meta = wavio.read_payload(path, into=lambda n: self._pinned(slot, n).numpy())
        return self._pins[slot][0][:len(payload)], meta, slot

    def _decode(self, host, meta, slot):
        """The host bytes of a data chunk -> [channels, frames] f32 on the GPU: one copy, one kernel."""
        if host.numel() == 0:
            return torch.zeros((meta.num_channels, 0), dtype=torch.float32, device=self.device)
        dev = torch.empty((host.numel(),), dtype=torch.uint8, device=self.device)
        dev.copy_(host, non_blocking=True)
        busy = torch.cuda.Event()
        busy.record()
        self._pins[slot] = (self._pins[slot][0], busy)
        return pcm_decode(dev, meta.num_frames, meta.num_channels, meta.format_tag, meta.bits_per_sample)

    def _write(self, path_out, sr, encoding, stage=None):
        """[C, L] on the GPU -> encoded on the device -> one copy back -> header + payload.  `stage`: the output-stage options
        (check_output_options), or None for the plain encoder.  With a stage the peak kernel runs in front of the encoder,
        which for clip 'guard' reads the gain from device memory, and the figures come back with the payload behind the
        one synchronisation; they are returned as the result's 'output'.  path_out None: the figures only."""
        from .data import wavio
        w = sr.contiguous()
        packed = None
        if stage is None:
            dev = pcm_encode(w, encoding)
        else:
            (peak, over, nonfinite, gain), packed = _pcm_peaks_packed(w, encoding, stage['ceiling'], "enhance_file")
            dev = None if path_out is None else pcm_encode(w, encoding, gain=gain if stage['clip'] == 'guard' else None,
                                                           dither=stage['dither'], seed=stage['seed'])
        host = None
        if dev is not None:
            host = self._pinned('out', dev.numel())[:dev.numel()]
            host.copy_(dev, non_blocking=True)
        if packed is not None:
            stats = self._pinned('peaks', packed.numel())[:packed.numel()]
            stats.copy_(packed, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        output = None
        if packed is not None:
            C = w.shape[0]
            raw = stats.numpy()
            peak = [float(v) for v in raw[16 * C:20 * C].view('<f4')]
            output = {'peak': peak, 'peak_dbfs': [_dbfs(v) for v in peak],
                      'clipped': [int(v) for v in raw[:8 * C].view('<i8')], 'nonfinite': [int(v) for v in raw[8 * C:16 * C].view('<i8')],
                      'gain': float(raw[20 * C:].view('<f4')[0]) if stage['clip'] == 'guard' else 1.0}
            if stage['clip'] == 'error' and any(output['clipped']):
                raise ValueError("%s: %d samples would clip in %s (peak %+.2f dBFS); nothing was written -- clip='guard' scales "
                                 "the file down, encoding='float32' keeps the samples"
                                 % (path_out, sum(output['clipped']), encoding, max(output['peak_dbfs'])))
        if host is not None:
            folder = os.path.dirname(os.path.abspath(path_out))
            os.makedirs(folder, exist_ok=True)
            wavio.write_payload(path_out, host.numpy(), int(self.opt.hr_sampling_rate), sr.shape[0], encoding)
        return output

    def _enhance_payload(self, read, path_out, is_lr_input, channels, encoding, extended_metrics=False, stage=None):
        from .data.audio_dataset import lr_round_trip
        from .util import util as U
        o = self.opt
        host, meta, slot = read
        if encoding not in PCM_ENCODINGS:
            raise ValueError("enhance_file: encoding must be one of %s, got %r" % (sorted(PCM_ENCODINGS), encoding))
        k = select_channels(channels, meta.num_channels)
        rate = meta.sample_rate
        raw = self._decode(host, meta, slot)[:k]
        lr = lr_round_trip(raw, rate, o.lr_sampling_rate, o.hr_sampling_rate, is_lr_input)
        has_hr = not is_lr_input and int(rate) == int(o.hr_sampling_rate)
        if has_hr:
            lr = lr[..., :raw.shape[-1]]                                    # the round trip rounds the length up
        sr = self.enhance_lr(lr)
        metrics = ext = None
        if has_hr and extended_metrics:
            # every written channel in one call and one copy back; the 7-tuples are read off the same rows
            ext = U.compute_matrics_ext(raw, lr, sr, o)
            metrics = [(e['mse'], e['snr_sr'], e['snr_lr'], 0, 0, 0, e['lsd']) for e in ext]
            if channels == 'first':
                metrics = metrics[0]
        elif has_hr and channels == 'first':
            metrics = U.compute_matrics(raw, lr, sr, o)
        elif has_hr:
            metrics = [U.compute_matrics(raw[c:c + 1], lr[c:c + 1], sr[c:c + 1], o) for c in range(k)]
        output = None
        if path_out is not None or stage is not None:
            output = self._write(path_out, sr, encoding, stage)
        res = {'sr': sr, 'lr': lr, 'hr': raw if has_hr else None, 'metrics': metrics, 'info': meta}
        if extended_metrics:
            res['metrics_ext'] = ext
        if stage is not None:
            res['output'] = output
        return res

    def enhance_file(self, path_in, path_out=None, is_lr_input=False, channels='first', encoding='pcm16', extended_metrics=False,
                     clip='clamp', ceiling_dbfs=None, dither=None, dither_seed=0, report_peaks=False):
        """wav -> the low-rate round trip of AudioTestDataset (or, with `is_lr_input`, a plain upsample of a clip that is
        already band-limited) -> enhance_lr -> wav at opt.hr_sampling_rate.  `channels`: 'first' (the default), 'all', or an
        int N (the first N).  `encoding` of the output: 'pcm16' | 'pcm24' | 'float32'.  The data chunk is decoded and the
        output encoded on the device (csrc/pcm.hip).  Returns {'sr', 'lr', 'hr', 'metrics', 'info'}: [C, L] tensors on the GPU;
        'hr' and 'metrics' are None unless the input is a full-band clip at the high rate; 'metrics' is
        util.compute_matrics against the input with 'first', else a list with one such 7-tuple per written channel, each
        computed on that channel alone; 'info' is the input's wavio.WavInfo.  `extended_metrics`: the result gains
        'metrics_ext', util.compute_matrics_ext of all written channels from one device call -- a list with one dict
        (util.METRIC_ROW_NAMES -> float) per written channel, also with 'first'; None where 'metrics' is None -- and 'metrics'
        holds the same rows' figures.
        The output stage (all opt-in; 'sr' and the metrics are the unscaled clip whatever it does, only the written bytes
        change).  `clip`: 'clamp' (default: the integer encodings clamp to their range, silently), 'guard' (the whole file, all
        channels alike, is scaled down so that its peak sits at `ceiling_dbfs` -- None: the encoding's own limit; a file that
        fits is left alone) or 'error' (ValueError naming the file, its peak and the clipped count, before anything is
        written).  `dither`: None or 'tpdf' (pcm16 only: +-1 LSB of triangular noise in front of the rounding, fixed by
        `dither_seed`).  `report_peaks`: measure only.  With any of the five given the result gains 'output': {'peak',
        'peak_dbfs', 'clipped', 'nonfinite' (a list each, one entry per written channel, measured on the unscaled clip for
        `encoding`), 'gain' (the factor applied: 1.0 unless 'guard' scaled)}."""
        stage = check_output_options(encoding, clip, ceiling_dbfs, dither, dither_seed, report_peaks)
        return self._enhance_payload(self._read(path_in), path_out, is_lr_input, channels, encoding, extended_metrics, stage)

    def enhance_folder(self, dir_in, dir_out, is_lr_input=False, channels='first', encoding='pcm16', seed=None, report=None,
                       extended_metrics=False, clip='clamp', ceiling_dbfs=None, dither=None, dither_seed=0, report_peaks=False):
        """Every *.wav under dir_in (plan_folder: sorted, recursive) -> the same relative path under dir_out, with one model
        and one captured graph for the whole run.  A file that does not parse is reported and skipped.  `seed`: re-seed the
        generator in front of every file, so that a file comes out as a run of its own with that seed would write it.
        `report(record)` is called after every file.  Returns one record per file: {'path' (relative), 'rate', 'channels',
        'frames' (of the input), 'written_channels', 'out_frames', 'metrics' (as enhance_file(channels != 'first') returns
        them: a list per channel, or None), 'error' (None, or the text of what went wrong)}; with `extended_metrics` also
        'metrics_ext' (as enhance_file returns it).  `clip`, `ceiling_dbfs`, `dither`, `dither_seed`, `report_peaks`: the output
        stage of enhance_file, per file (a guard gain is one file's); file k of the plan is dithered with seed `dither_seed` + k;
        with any of them given a record gains 'output' (as enhance_file returns it, None for a skipped file).  clip 'error'
        ends the run at the first file that would clip."""
        stage = check_output_options(encoding, clip, ceiling_dbfs, dither, dither_seed, report_peaks, "enhance_folder")
        records = []
        for k, (rel, path_in, path_out) in enumerate(plan_folder(dir_in, dir_out)):
            rec = {'path': rel, 'rate': None, 'channels': None, 'frames': None, 'written_channels': 0, 'out_frames': 0,
                   'metrics': None, 'error': None}
            if extended_metrics:
                rec['metrics_ext'] = None
            if stage is not None:
                rec['output'] = None
            try:
                read = self._read(path_in)
            except (ValueError, OSError, EOFError, struct.error) as e:
                rec['error'] = '%s: %s' % (type(e).__name__, e)
            else:
                if seed is not None:
                    torch.manual_seed(int(seed))
                res = self._enhance_payload(read, path_out, is_lr_input, channels, encoding, extended_metrics,
                                            None if stage is None else dict(stage, seed=dither_seed + k))
                m, meta = res['metrics'], res['info']
                rec.update(rate=meta.sample_rate, channels=meta.num_channels, frames=meta.num_frames,
                           written_channels=res['sr'].shape[0], out_frames=res['sr'].shape[-1],
                           metrics=[m] if m is not None and channels == 'first' else m)
                if extended_metrics:
                    rec['metrics_ext'] = res['metrics_ext']
                if stage is not None:
                    rec['output'] = res['output']
            records.append(rec)
            if report is not None:
                report(rec)
        return records


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
def parse_opt_file(path):
    """The `key: value` dump every reference run writes (options/base_options.py:102-107) -> dict.  Values go through
    ast.literal_eval where that parses (numbers, booleans, None, lists), `inf` / `-inf` / `nan` become floats, anything
    else stays a string.  The dashed first and last lines are skipped; any other line without `key: value` is an error."""
    if not os.path.isfile(path):
        raise FileNotFoundError("options file %s does not exist (pass --opt_file; a reference run writes opt.txt beside its "
                                "checkpoints)" % path)
    out = {}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            line = line.strip()
            if not line or (line.startswith('-') and line.endswith('-')):
                continue
            key, sep, value = line.partition(':')
            key, value = key.strip(), value.strip()
            if not sep or not key.isidentifier():
                raise ValueError("%s:%d: expected `key: value`, got %r" % (path, no, line))
            try:
                out[key] = ast.literal_eval(value)
            except (ValueError, SyntaxError):
                out[key] = float(value) if value in ('inf', '-inf', 'nan') else value
    if not out:
        raise ValueError("%s holds no `key: value` line" % path)
    return out


def opt_from_file(path, **overrides):
    """Namespace for create_model from an options dump: the file's values, inference on GPU 0, then `overrides`."""
    d = parse_opt_file(path)
    d.update(gpu_ids=[0], isTrain=False)
    d.update(overrides)
    return SimpleNamespace(**d)


def _channels_arg(text):
    if text in ("all", "first"):
        return text
    try:
        n = int(text)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError("expected all, first or a count >= 1, got %r" % text)
    return n


def check_paths(path_in, path_out):
    """-> True for folder mode (both are directories; the output one may not exist yet), False for one file.  Mixing a file
    and a directory is an error."""
    if os.path.isdir(path_in):
        if os.path.isfile(path_out):
            raise ValueError("--input %s is a directory, so --output must be a directory too, and %s is a file" % (path_in, path_out))
        return True
    if os.path.isdir(path_out):
        raise ValueError("--input %s is a file, so --output must be a file too, and %s is a directory" % (path_in, path_out))
    return False


METRICS_COLUMNS = ("file", "channel", "frames", "mse", "snr_sr", "snr_lr", "lsd")
METRICS_COLUMNS_EXT = METRICS_COLUMNS + ("lsd_lf", "lsd_hf", "ssnr_sr", "ssnr_lr")     # --metrics_ext


def _nanmean(values):
    kept = [v for v in values if v == v]
    return sum(kept) / len(kept) if kept else float('nan')


METRICS_COLUMNS_PEAKS = ("peak_dbfs", "clipped", "gain")                                # --report_peaks


def metrics_rows(records, extended=False, peaks=False):
    """records of enhance_folder -> the rows of --metrics_csv: one per written channel that has metrics, then the `mean` row
    (the plain mean of each column over the rows above, what the reference's eval_matric.py averages); no mean row when
    nothing was measured.  `extended`: the records carry 'metrics_ext' and a row has the columns of METRICS_COLUMNS_EXT; the
    mean of a column then runs over its entries that are not NaN (a clip too short for one segment has no segmental SNR).
    `peaks`: the records carry 'output' and a row ends with the columns of METRICS_COLUMNS_PEAKS -- the channel's peak in
    dBFS, its clipped samples and the file's gain; the mean row holds their plain means."""
    rows = []
    if extended:
        for r in records:
            for c, e in enumerate(r['metrics_ext'] or ()):
                rows.append((r['path'], c, r['out_frames']) + tuple(e[name] for name in METRICS_COLUMNS_EXT[3:]))
        if rows:
            rows.append(("mean", "", "") + tuple(_nanmean([row[k] for row in rows]) for k in range(3, len(METRICS_COLUMNS_EXT))))
    else:
        for r in records:
            for c, m in enumerate(r['metrics'] or ()):
                rows.append((r['path'], c, r['out_frames'], m[0], m[1], m[2], m[6]))
        if rows:
            rows.append(("mean", "", "") + tuple(sum(row[k] for row in rows) / len(rows) for k in range(3, 7)))
    if peaks and rows:
        tail = []
        for r in records:
            o = r['output']
            for c in range(len((r['metrics_ext'] if extended else r['metrics']) or ())):
                tail.append((o['peak_dbfs'][c], o['clipped'][c], o['gain']))
        tail.append(tuple(sum(t[k] for t in tail) / len(tail) for k in range(3)))
        rows = [row + t for row, t in zip(rows, tail)]
    return rows


def write_metrics_csv(path, records, extended=False, peaks=False):
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow((METRICS_COLUMNS_EXT if extended else METRICS_COLUMNS) + (METRICS_COLUMNS_PEAKS if peaks else ()))
        for row in metrics_rows(records, extended, peaks):
            w.writerow([repr(v) if isinstance(v, float) else v for v in row])


def _parser():
    ap = argparse.ArgumentParser(prog="python -m pix2pixhdaudiosr_amd.generate", description=__doc__.split("\n")[0])
    ap.add_argument("--input", required=True, help="wav file to enhance, or a folder: every *.wav below it")
    ap.add_argument("--output", required=True, help="wav file to write (at hr_sampling_rate), or the folder that takes the "
                                                    "outputs at the inputs' relative paths")
    ap.add_argument("--channels", type=_channels_arg, default="first", metavar="all|first|N",
                    help="channels of a file to enhance and write: the first one (default), all, or the first N; every "
                         "channel is enhanced as a clip of its own")
    ap.add_argument("--encoding", default="pcm16", choices=sorted(PCM_ENCODINGS), help="sample format of the output (default pcm16)")
    ap.add_argument("--metrics_csv", default=None, metavar="PATH",
                    help="write file, channel, frames, mse, snr_sr, snr_lr, lsd of every written channel that has a full-band "
                         "original, and a last `mean` row")
    ap.add_argument("--metrics_ext", action="store_true",
                    help="also measure, per channel, the log-spectral distance below and from the low rate's Nyquist frequency "
                         "(lsd_lf, lsd_hf) and the segmental SNR of the output and of the low-rate input (ssnr_sr, ssnr_lr): "
                         "printed, and four more columns of --metrics_csv")
    ap.add_argument("--load_pretrain", required=True, help="folder with <which_epoch>_net_G.pth (and opt.txt)")
    ap.add_argument("--opt_file", default=None, help="options dump of the training run (default: <load_pretrain>/opt.txt)")
    ap.add_argument("--which_epoch", default=None)
    ap.add_argument("--overlap", type=float, default=0.25, help="shared fraction of neighbouring segments, 0 .. 0.5 (0: the reference's chain)")
    ap.add_argument("--batchSize", type=int, default=None, help="segments per group")
    ap.add_argument("--is_lr_input", action="store_true", help="the input is a low-rate clip: upsample it, no round trip")
    ap.add_argument("--no_graph", action="store_true", help="run every group eagerly")
    ap.add_argument("--reference_amplitude", type=int, choices=(0, 1), default=None,
                    help="MDCT2 checkpoints: 1 keeps the half amplitude of the reference's generate_audio.py, 0 writes the full "
                         "one, 6 dB more (default: 1 at --overlap 0, the reference-exact mode, else 0)")
    ap.add_argument("--lowband", default="model", choices=LOWBANDS,
                    help="where the band the input already had comes from: the generator's spectrogram like every other row "
                         "(model, default), or the input's own spectrogram (input): only the rows from the low rate's Nyquist "
                         "frequency up are then the generator's")
    ap.add_argument("--lowband_fade", type=int, default=0, metavar="N",
                    help="--lowband input: cross-fade input and generator over the N spectrogram rows below that frequency "
                         "(default 0: a hard switch)")
    ap.add_argument("--crossover", default=None, choices=("input",),
                    help="time-domain crossover behind the stitch: below --crossover_hz the written clip is the input itself, above "
                         "it the generator's output (a linear-phase complementary filter pair; default: off)")
    ap.add_argument("--crossover_hz", type=float, default=None, metavar="F",
                    help="--crossover input: the crossover frequency (default: 0.95 of the low rate's Nyquist frequency)")
    ap.add_argument("--crossover_taps", type=int, default=None, metavar="N",
                    help="--crossover input: length of the filter, odd, <= 4095 (default: the shortest whose transition band ends "
                         "under the low rate's Nyquist frequency)")
    ap.add_argument("--clip", default="clamp", choices=CLIP_MODES,
                    help="samples beyond the range of --encoding: clamp them, silently (default); guard: scale the whole file down, "
                         "all channels alike, so that its peak sits at --ceiling_dbfs; error: write nothing and stop")
    ap.add_argument("--ceiling_dbfs", type=float, default=None, metavar="DB",
                    help="--clip guard: the level the peak is brought down to, <= 0 (default: the limit of --encoding)")
    ap.add_argument("--dither", default=None, choices=("tpdf",),
                    help="pcm16 only: +-1 LSB of triangular noise in front of the rounding, so that the quantisation error of quiet "
                         "passages is noise and not distortion")
    ap.add_argument("--dither_seed", type=int, default=0, help="seed of --dither (file k of a folder uses seed + k)")
    ap.add_argument("--report_peaks", action="store_true",
                    help="print peak (dBFS), clipped and non-finite samples and the gain of every file; three more columns "
                         "(peak_dbfs, clipped, gain) of --metrics_csv")
    ap.add_argument("--fp16", action="store_true", help="16-bit activation storage")
    ap.add_argument("--mdct_type", default=None, choices=("mdct2", "mdct4"),
                    help="transform of the checkpoint (default: the options file's, else $P2PHD_MDCT_TYPE, else mdct2 -- "
                         "the one the reference's train.py, which writes opt.txt, is hard-wired to)")
    return ap


def _print_metrics(m, prefix=''):
    mse, snr_sr, snr_lr, _, _, _, lsd = m
    print('%sMSE: %.4f' % (prefix, mse))                                    # generate_audio.py:53-59
    print('%sSNR_SR: %.4f' % (prefix, snr_sr))
    print('%sSNR_LR: %.4f' % (prefix, snr_lr))
    print('%sLSD: %.4f' % (prefix, lsd))


def _print_metrics_ext(e, prefix=''):
    print('%sLSD_LF: %.4f' % (prefix, e['lsd_lf']))
    print('%sLSD_HF: %.4f' % (prefix, e['lsd_hf']))
    print('%sSSNR_SR: %.4f' % (prefix, e['ssnr_sr']))
    print('%sSSNR_LR: %.4f' % (prefix, e['ssnr_lr']))


def _print_peaks(name, o):
    print('%s: peak %s dBFS, %d clipped, %d non-finite, gain %.6f' % (name, ' '.join('%+.2f' % v for v in o['peak_dbfs']),
                                                                    sum(o['clipped']), sum(o['nonfinite']), o['gain']))


def _print_unwritten(name, available, written):
    if written < available:
        print('%s: %d of %d channels enhanced and written (--channels all writes every channel)' % (name, written, available))


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    try:
        folder_mode = check_paths(a.input, a.output)
    except ValueError as e:
        ap.error(str(e))
    try:                                                                    # before anything is loaded
        check_output_options(a.encoding, a.clip, a.ceiling_dbfs, a.dither, a.dither_seed, a.report_peaks, "generate")
    except ValueError as e:
        ap.error(str(e))
    stage = dict(clip=a.clip, ceiling_dbfs=a.ceiling_dbfs, dither=a.dither, dither_seed=a.dither_seed, report_peaks=a.report_peaks)
    folder = os.path.abspath(a.load_pretrain)
    over = dict(checkpoints_dir=os.path.dirname(folder), name=os.path.basename(folder), load_pretrain='', continue_train=False)
    for k in ("which_epoch", "batchSize"):
        if getattr(a, k) is not None:
            over[k] = getattr(a, k)
    if a.fp16:
        over["fp16"] = True
    opt = opt_from_file(a.opt_file or os.path.join(folder, "opt.txt"), **over)
    if a.mdct_type is not None or not hasattr(opt, 'mdct_type'):
        opt.mdct_type = a.mdct_type or os.environ.get('P2PHD_MDCT_TYPE', 'mdct2')
    try:                                                                    # before the model is built
        check_lowband(a.lowband, a.lowband_fade, int(opt.n_fft) if opt.mdct_type == 'mdct2' else int(opt.n_fft) // 2,
                      opt.hr_sampling_rate / opt.lr_sampling_rate)
        check_crossover(a.crossover, a.crossover_hz, a.crossover_taps, opt.hr_sampling_rate, opt.lr_sampling_rate)
    except ValueError as e:
        ap.error(str(e))
    from .models.models import create_model
    model = create_model(opt)
    model.eval()
    seed = getattr(opt, 'seed', None)
    if seed is not None:
        torch.manual_seed(int(seed))                                        # the mask noise: one run, one result
    sr = SuperResolver(model, opt, overlap=a.overlap, graph=not a.no_graph,
                       reference_amplitude=None if a.reference_amplitude is None else bool(a.reference_amplitude),
                       lowband=a.lowband, lowband_fade=a.lowband_fade, crossover=a.crossover, crossover_hz=a.crossover_hz,
                       crossover_taps=a.crossover_taps)
    print('amplitude: %s; low band: %s' % ("the reference's (half of sqrt(up_ratio - 1) * x)" if sr.reference_amplitude else 'full',
                                           "the model's" if sr.lowband == 'model' else
                                           "the input's (fade over %d rows)" % sr.lowband_fade))
    if sr.crossover_plan is not None:                                       # (without the option: no line more than before)
        print('crossover: the input below %g Hz (%d taps)' % (sr.crossover_plan[1] * opt.hr_sampling_rate, sr.crossover_plan[0]))
    rate = int(opt.hr_sampling_rate)
    try:
        return _run(a, sr, stage, seed, rate, folder_mode)
    except ValueError as e:
        if a.clip != 'error' or 'would clip' not in str(e):
            raise
        print('error: %s' % e, file=sys.stderr)                             # --clip error: the file that would clip
        return 1


def _run(a, sr, stage, seed, rate, folder_mode):
    if folder_mode:
        def report(r):
            if r['error'] is not None:
                print('skipped %s: %s' % (r['path'], r['error']))
                return
            _print_unwritten(r['path'], r['channels'], r['written_channels'])
            print('wrote %s (%d samples at %d Hz, %d channel%s)' % (os.path.join(a.output, r['path']), r['out_frames'], rate,
                                                                   r['written_channels'], '' if r['written_channels'] == 1 else 's'))
            if a.report_peaks:
                _print_peaks(r['path'], r['output'])
        # every file starts from the seed, so it comes out as a run of its own would write it
        records = sr.enhance_folder(a.input, a.output, a.is_lr_input, a.channels, a.encoding, seed=seed, report=report,
                                    extended_metrics=a.metrics_ext, **stage)
        done = [r for r in records if r['error'] is None]
        print('%d of %d files enhanced, %d skipped' % (len(done), len(records), len(records) - len(done)))
        rows = metrics_rows(records, a.metrics_ext)                       # (the printed means: no peak columns)
        if rows:
            print('mean over %d channels: MSE %.4f  SNR_SR %.4f  SNR_LR %.4f  LSD %.4f' % ((len(rows) - 1,) + rows[-1][3:7]))
            if a.metrics_ext:
                print('mean over %d channels: LSD_LF %.4f  LSD_HF %.4f  SSNR_SR %.4f  SSNR_LR %.4f' % ((len(rows) - 1,) + rows[-1][7:]))
    else:
        res = sr.enhance_file(a.input, a.output, a.is_lr_input, a.channels, a.encoding, extended_metrics=a.metrics_ext, **stage)
        m, written = res['metrics'], res['sr'].shape[0]
        ext = res.get('metrics_ext')
        _print_unwritten(a.input, res['info'].num_channels, written)
        if m is not None and a.channels == 'first':
            _print_metrics(m)
            if ext is not None:
                _print_metrics_ext(ext[0])
        elif m is not None:
            for c, mc in enumerate(m):
                _print_metrics(mc, 'channel %d ' % c)
                if ext is not None:
                    _print_metrics_ext(ext[c], 'channel %d ' % c)
        if written == 1:
            print('wrote %s (%d samples at %d Hz)' % (a.output, res['sr'].shape[-1], rate))
        else:
            print('wrote %s (%d samples at %d Hz, %d channels)' % (a.output, res['sr'].shape[-1], rate, written))
        if a.report_peaks:
            _print_peaks(a.output, res['output'])
        records = [{'path': os.path.basename(a.input), 'out_frames': res['sr'].shape[-1],
                    'metrics': [m] if m is not None and a.channels == 'first' else m, 'metrics_ext': ext, 'output': res.get('output')}]
    if a.metrics_csv:
        write_metrics_csv(a.metrics_csv, records, a.metrics_ext, a.report_peaks)
        print('metrics: %s' % a.metrics_csv)
    return 0


if __name__ == '__main__':
    sys.exit(main())
