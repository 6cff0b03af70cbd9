"""Whole-file generation: SuperResolver -- the options of the two entry points, the per-file flow between the rows of a clip
(generate/rows.py) and the two ends of the file path (generate/fileio.py), a folder's records and the folder drivers."""
import inspect
import math
import os
import struct
from collections import namedtuple

import torch

from .fileio import FilePath, _set                                                                                                  # noqa: F401
from .ops import (_loudness_views, _speech_level_views, bandwidth as _bandwidth, loudness_gate, loudness_hops, loudness_range, loudness_short_term,
                  rate_convert, spectrogram_rgb, speech_level as _speech_level, speech_level_packed_bytes, stereo_image as _stereo_image, stft_db)
from .plans import (LOUDNESS_MAX_CHANNELS, SPEECH_LEVEL_MAX_CHANNELS, bandwidth_notes, check_bandwidth, check_container, check_dither, check_encoding,
                    check_limiter, check_loudness, check_loudness_rate, check_loudness_scope, check_output_options, check_output_rate, check_pack_files,
                    check_spectrogram, check_speech_level, check_speech_level_rate, check_stereo_report, check_stream, check_true_peak, group_rows_plan,
                    loudness_channel_weights, pack_plan, plan_folder, segment_plan, select_channels, stereo_figures, stereo_notes, stereo_split_bin)
from .rows import ClipPath
from .stream import StreamPath

# The validated options of enhance_file / enhance_folder (SuperResolver._options), each None where it is off: the output stage,
# the true-peak, limiter, spectrogram, loudness, bandwidth, stereo-report and output-rate options, the album (loudness_scope 'folder')
# and the FLAC container.
_Options = namedtuple('_Options', 'stage tp lim spec loud bw st rc album flac sl', defaults=(None, None))

# The keys a folder record may carry behind the eight it always has (and 'written'), in the record's order; each is also the key
# of enhance_file's result that fills it ('album': enhance_album's own).  Which of them a run has: SuperResolver._present.
_RECORD_KEYS = ('metrics_ext', 'output', 'spectrogram', 'loudness', 'speech_level', 'album', 'bandwidth', 'crossover', 'stereo', 'output_rate', 'norm', 'flac')

# The same keys (but the album's) in the order enhance_file's result carries them behind the five it always has.
_RESULT_KEYS = ('norm', 'spectrogram', 'loudness', 'speech_level', 'bandwidth', 'crossover', 'stereo', 'output_rate', 'metrics_ext', 'output', 'flac')

# The measurements that ride back with the payload: `key` of the result, of a record, of _write's keyword and of the pinned slot;
# `field` of _Options; the method that queues the device work (-> a dict with 'packed') and the one that reads what _fetch brought
# back.  `levels`: False -- taken in _reports on (lr, generated, original); True -- taken in _level on (lr, generated), and its 'gain'
# multiplies the clip unless the option's mode is 'report'.  `channels`: None, or the one written channel count it is taken at.
_Measured = namedtuple('_Measured', 'key field measure result levels channels')
_MEASURED = (_Measured('bandwidth', 'bw', '_measure_bandwidth', '_bandwidth_result', False, None),
             _Measured('stereo', 'st', '_measure_stereo', '_stereo_result', False, 2),
             _Measured('speech_level', 'sl', '_measure_speech_level', '_speech_level_result', True, None),
             _Measured('loudness', 'loud', '_measure_loudness', '_loudness_result', True, None))


class _File:
    """One file between the stages of the per-file flow: `clip` the generated clip as the latest stage left it, `lr` the clip the
    generator was given, `hr` the original where the input is one (else None), `meta` the input's WavInfo / FlacInfo, `metrics` and
    `ext` (None until the metrics stage, and without an original), `norm` and `crossover`: the object's last_norm and a copy of
    its last_crossover behind this file's enhance_lr (None without norm_scope 'clip' or segment_norm / crossover_hz 'auto')."""
    __slots__ = ('clip', 'lr', 'hr', 'meta', 'metrics', 'ext', 'norm', 'crossover')

    def __init__(self, clip, lr, hr, meta, norm, crossover):
        self.clip, self.lr, self.hr, self.meta, self.norm, self.crossover = clip, lr, hr, meta, norm, crossover
        self.metrics = self.ext = None


def first_channel_metrics(metrics, channels):
    """The per-channel list of 7-tuples (or None) as enhance_file returns it: with 'first' the one tuple itself."""
    return metrics[0] if metrics is not None and channels == 'first' else metrics


def per_channel_metrics(metrics, channels):
    """What enhance_file returned as 'metrics' -> the list with one 7-tuple per written channel (or None)."""
    return [metrics] if metrics is not None and channels == 'first' else metrics


def _spectrogram(rows, top_db, plan):
    """The device work of spectrogram_image -> (the picture, the dB planes, the top as a float32 tensor of one element)."""
    db = stft_db(rows, plan['n_fft'], plan['hop'])
    if db.shape[0] < 1 or db.shape[1] < 1:
        raise ValueError("spectrogram_image: a picture needs at least one row of at least one sample, got shape %s" % (tuple(rows.shape),))
    if top_db is None:
        top = db.amax().reshape(1)
    else:
        top = torch.full((1,), float(top_db), dtype=torch.float32, device=db.device)
    return spectrogram_rgb(db, top, plan['range_db'], plan['width'], plan['height'], plan['gap']), db, top


def spectrogram_image(rows, top_db=None, **plan):
    """rows [R, L] f32 on the GPU, one clip per panel -> the picture [R * height + (R - 1) * gap, width, 3] uint8 on the GPU
    (util.save_image writes it once it is on the host): panel r is the spectrogram of rows[r] -- ops.stft_db, a Hann-windowed
    STFT in dB where a full-scale sine reads 0 -- the whole clip left to right, 0 Hz in the panel's bottom row and the Nyquist
    frequency in its top row; all panels share the dB scale, from `top_db` - range_db (the palette's first colour) to `top_db`
    (its last).  `top_db`: None -- the largest value of all panels, taken on the device and read there by the renderer -- or
    a fixed level.  `plan`: n_fft, hop, width, height (of one panel), range_db, gap (plans.check_spectrogram;
    SPECTROGRAM_DEFAULTS where left out).  Two launches of the family "specimg", nothing is waited for."""
    return _spectrogram(rows, top_db, check_spectrogram(top_db=top_db, who="spectrogram_image", **plan))[0]


def _named(local):
    """The locals of an entry point -> those that are options of SuperResolver._options, by name."""
    return {name: local[name] for name in _OPTION_NAMES if name in local}


class SuperResolver(ClipPath, FilePath, StreamPath):
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
    hr_sampling_rate.  `crossover_hz` 'auto': the crossover follows the band each clip has.  The clip's band edge is measured on
    the device in front of the generator (ops.bandwidth with BANDWIDTH_DEFAULTS, all channels one programme), edge = min(the low
    rate's Nyquist frequency, where the band ends), and the filter is plans.crossover_auto_plan's: the crossover at 0.95 of the edge,
    the transition band ending at the edge -- a telephone-band input in a 16 kHz file keeps its 3.4 kHz and the generator fills the
    rest, where the fixed crossover would copy an empty band.  An input that reaches the Nyquist frequency gets the default plan and
    the default bytes.  The 32 bytes of the measurement come back on a side stream behind an event recorded in front of the first
    group, so the host waits for two small launches, not for the generator; coefficients are cached per band edge.
    `last_crossover` then holds {'hz', 'taps', 'edge_hz'} of the latest clip.
    `stereo`: 'lr' (the default) | 'ms', fixed for the object's life.  With 'lr' every channel is a clip of its own, so the band
    above the low rate's Nyquist frequency of a two-channel clip is invented twice, independently.  'ms' generates mid and side
    instead: a [2, L] clip is encoded as ((L + R) / 2, (L - R) / 2) (csrc/stereo.hip), goes through the unchanged per-channel
    pipeline -- mask-noise row block 0 is the mid signal's, block 1 the side's; the crossover's low band is the encoded input -- and
    is decoded as (M + S, M - S), a non-finite side sample read as 0: what the channels share is invented once.  The auto
    crossover's measurement stays on left / right.  Two launches of the family "stereo" per two-channel clip; one channel runs as
    with 'lr', more than two are a ValueError.
    `norm_scope`: 'group' (the default) | 'clip', fixed for the object's life: what the dB spectrogram is normalised by.  With
    'group' it is the minimum and maximum of each group of `batch` segments, the reference's chain: the written file depends on
    the batch size and on which segments share a group, and a group of digital silence (max == min) comes out as NaN.  With 'clip'
    a clip -- one channel of a file; with stereo='ms' the mid or the side signal -- has one range, over all of its segments: a pass
    in front of the clip's first group (model.clip_norm: the transform of every segment once more, one read of each spectrum,
    nothing kept, nothing brought to the host) leaves it in 8 floats on the device and every group's encode reads it there
    (model.inference(..., norm=)); the captured chain reads it from a static buffer filled in front of every replay, so one
    capture serves every clip.  A range of zero scales by 0: a clip of digital silence is written as silence.  The launches are
    those of the family "normscope": ceil(S / batch) range calls and one noise fold per clip, one encode per group.
    `last_norm` then holds the [C, 2] tensor on the GPU of the latest call's (min, max) per clip, in dB.
    `segment_norm`: False (the default) | True, fixed for the object's life; not with norm_scope 'clip'.  Every segment is
    normalised by its own range -- what 'group' means at batch 1, at any batch --: the encode takes each row's statistics on the
    device (model.inference(..., norm='rows')) and util.imdct decodes each row under its own, the launches of the family
    "normrows", two per group.  The rows of a group then no longer know of one another, so the C * S rows of a clip are walked in
    groups of `batch` without regard to channel (plans.group_rows_plan) and the last group is filled up with rows of zeros, whose
    range of zero encodes as zeros and whose output is dropped: every group has `batch` rows, the graphed run and the eager run
    are the same launches, and one capture serves every clip, channel count and length.  The file does not depend on the batch
    beyond what the generator itself does with it; a silent segment is written as silence.  No pre-pass, no held noise.
    `last_norm` then holds the [C, S, 2] tensor on the GPU of the latest call's (min, max) per segment, in dB."""

    @staticmethod
    def _limiter_option(limiter, lookahead_ms, hold_ms, true_peak, stage, encoding, hr_rate, who):
        """check_limiter and check_true_peak for enhance_file / enhance_folder -> (stage, tp, lim): the limiter switches the
        true-peak measurement on, and takes its rate and ceiling from it."""
        lim = check_limiter(limiter, lookahead_ms, hold_ms, stage, encoding, hr_rate, who)
        stage, tp = check_true_peak(true_peak, stage, encoding, hr_rate, who)
        if lim is not None:
            if tp is None:
                stage, tp = check_true_peak(True, stage, encoding, hr_rate, who)
            lim = {'lookahead': lim['lookahead'], 'hold': lim['hold'], 'rate': tp['rate'], 'ceiling': tp['ceiling']}
        return stage, tp, lim

    def _check_written_channels(self, o, channels, available):
        """ValueError where an option does not take the channels that would be written of a file with `available`, before
        anything of the file runs -- on the per-file path the file's refusal, in a folder a skipped file (_open) --, in this order:
        the spectrogram's channel is not among them; stereo='ms' generates one or two; a FLAC stream holds 8; the speech level is
        measured over SPEECH_LEVEL_MAX_CHANNELS."""
        if o.spec is None and self.stereo != 'ms' and o.flac is None and o.sl is None:
            return                                                          # (`channels` itself is refused by _front_clip: never a skipped file)
        k = select_channels(channels, available)
        if o.spec is not None and o.spec['channel'] >= k:
            raise ValueError("spectrogram_channel %d: the file has %d channel%s and channels=%r writes %d"
                             % (o.spec['channel'], available, '' if available == 1 else 's', channels, k))
        if self.stereo == 'ms' and k > 2:
            raise ValueError("stereo='ms' takes one or two channels, %d would be written" % k)
        if o.flac is not None and k > 8:
            raise ValueError("a FLAC stream holds at most 8 channels, %d would be written" % k)
        if o.sl is not None and k > SPEECH_LEVEL_MAX_CHANNELS:
            raise ValueError("the active speech level is measured over at most %d channels, %d would be written" % (SPEECH_LEVEL_MAX_CHANNELS, k))

    @staticmethod
    def _render_picture(spec, lr, sr, hr):
        """The device work of the spectrogram option: channel spec['channel'] of the clips a file leaves, one panel each."""
        rows = torch.stack([t[spec['channel']] for t in (lr, sr, hr) if t is not None])
        image, db, top = _spectrogram(rows, spec['top_db'], spec['plan'])
        return {'image': image, 'top': top, 'panels': db.shape[0], 'frames': db.shape[1], 'bins': db.shape[2]}

    @staticmethod
    def _save_picture(spec, picture):
        """The fetched picture -> the PNG -> the result's 'spectrogram'."""
        from ..util import util as U
        os.makedirs(os.path.dirname(os.path.abspath(spec['path'])), exist_ok=True)
        U.save_image(picture['image'].numpy(), spec['path'])
        return {'path': spec['path'], 'panels': picture['panels'], 'frames': picture['frames'], 'bins': picture['bins'],
                'top_db': float(picture['top'][0]), 'range_db': spec['plan']['range_db']}

    def _measure_loudness(self, loud, lr, sr):
        """The device work of the loudness option: the clip the generator was given and the generated clip through the hop and
        gate kernels (four launches of the family "loudness") -> {'packed': both gate results in one buffer of 80 bytes, 'gain':
        the f32 on the device that brings `sr` to the wanted level (1 with 'report')}.  With loud['range'] the hop energies of
        either clip also go through the short-term and the range kernel (at most four launches more; the generated clip's powers
        take the gain from device memory, so the figures are those of the clip as this stage leaves it) and 'packed' holds their
        two res8 behind the gate results, 208 bytes in all.  With loud['out_rate'] (the output-rate option) `sr` is the converted
        clip: it is measured at that rate, the input still at the model's."""
        rate = int(self.opt.hr_sampling_rate)
        rate_out = loud.get('out_rate', rate)
        weights = loudness_channel_weights(sr.shape[0])
        ranged = loud.get('range', False)
        packed = torch.empty((208 if ranged else 80,), dtype=torch.uint8, device=sr.device)
        z_in = loudness_hops(lr, rate)
        res_in, _ = loudness_gate(z_in, rate, weights, out=packed[:40])
        wanted = {'report': {}, 'input': {'target_dev': res_in}, 'target': {'target': loud['target']}}[loud['mode']]
        z_out = loudness_hops(sr, rate_out)
        _, gain = loudness_gate(z_out, rate_out, weights, max_gain_db=loud['max_gain_db'], out=packed[40:80], **wanted)
        if ranged:
            loudness_range(loudness_short_term(z_in, rate, weights), out=packed[80:144].view(torch.float64))
            loudness_range(loudness_short_term(z_out, rate_out, weights, gain_dev=gain), out=packed[144:208].view(torch.float64))
        return {'packed': packed, 'gain': gain}

    @staticmethod
    def _loudness_result(loud, measure):
        """The fetched measurement -> the result's 'loudness'."""
        (res_in, _), (res_out, gain) = _loudness_views(measure['packed'][:40]), _loudness_views(measure['packed'][40:80])
        level_in, measured = float(res_in[0]), float(res_out[0])
        gain_db = 0.0 if loud['mode'] == 'report' else 20.0 * math.log10(float(gain[0]))
        result = {'input': level_in, 'measured': measured, 'gain_db': gain_db, 'output': measured + gain_db,
                  'momentary_max': float(res_out[1]) + gain_db,
                  'target': {'report': None, 'input': level_in, 'target': loud['target']}[loud['mode']]}
        if loud.get('range', False):
            r_in, r_out = (measure['packed'][a:a + 64].view(torch.float64).tolist() for a in (80, 144))
            result['range'] = {'input': r_in[0], 'output': r_out[0], 'low': r_out[1], 'high': r_out[2], 'threshold': r_out[3],
                               'blocks': int(r_out[4]), 'short_term_max': r_out[5]}
        return result

    def _measure_speech_level(self, sl, lr, sr):
        """The device work of the speech-level option: the clip the generator was given and the generated clip through the
        envelope, the counts and the decision (six launches of the family "speechlevel") -> {'packed': both packed results in one
        buffer, the input's first, 'gain': the f32 on the device that brings `sr` to the wanted active level (1 with 'report'),
        'channels': the rows of either clip}.  With sl['out_rate'] (the output-rate option) `sr` is the converted clip: it is
        measured at that rate, the input still at the model's."""
        rate = int(self.opt.hr_sampling_rate)
        rate_out = sl.get('out_rate', rate)
        n_in, n_out = speech_level_packed_bytes(lr.shape[0]), speech_level_packed_bytes(sr.shape[0])
        packed = torch.empty((n_in + n_out,), dtype=torch.uint8, device=sr.device)
        res_in, _ = _speech_level(lr, rate, out=packed[:n_in])
        wanted = {'report': {}, 'input': {'target_dev': res_in[lr.shape[0]]}, 'target': {'target': sl['target']}}[sl['mode']]
        _, gain = _speech_level(sr, rate_out, max_gain_db=sl['max_gain_db'], out=packed[n_in:], **wanted)
        return {'packed': packed, 'gain': gain, 'channels': (lr.shape[0], sr.shape[0])}

    @staticmethod
    def _speech_level_result(sl, measure):
        """The fetched measurement -> the result's 'speech_level'."""
        c_in, c_out = measure['channels']
        n_in = speech_level_packed_bytes(c_in)
        (res_in, _), (res_out, gain) = _speech_level_views(measure['packed'][:n_in], c_in), _speech_level_views(measure['packed'][n_in:], c_out)
        res_in, res_out = res_in.tolist(), res_out.tolist()
        level_in, measured = res_in[c_in][0], res_out[c_out][0]
        gain_db = 0.0 if sl['mode'] == 'report' else 20.0 * math.log10(float(gain[0]))
        return {'input': level_in, 'measured': measured, 'gain_db': gain_db, 'output': measured + gain_db,
                'target': {'report': None, 'input': level_in, 'target': sl['target']}[sl['mode']],
                'long_term': res_out[c_out][1] + gain_db, 'activity': res_out[c_out][2], 'activity_input': res_in[c_in][2],
                'channels': [{'active': r[0] + gain_db, 'long_term': r[1] + gain_db, 'activity': r[2]} for r in res_out[:c_out]]}

    def _measure_bandwidth(self, bw, lr, sr, hr):
        """The device work of the bandwidth option: the clip the generator was given, the generated clip and, where there is one, the
        original through the spectrum and the decision kernel (two launches of the family "bandwidth" each; all channels of a clip
        one programme) -> {'packed': their results of 32 bytes one behind the other, 'clips', 'frames'}."""
        clips = [t for t in (lr, sr, hr) if t is not None]
        packed = torch.empty((32 * len(clips),), dtype=torch.uint8, device=sr.device)
        rate = float(self.opt.hr_sampling_rate)
        for i, clip in enumerate(clips):
            _bandwidth(clip, rate, bw, out=packed[32 * i:32 * i + 32].view(torch.float64))
        L = sr.shape[-1]
        return {'packed': packed, 'clips': len(clips), 'frames': 1 + (L - bw['n_fft']) // bw['hop'] if L >= bw['n_fft'] else 0}

    def _bandwidth_result(self, bw, measure):
        """The fetched measurement -> the result's 'bandwidth'."""
        rate, nyquist = float(self.opt.hr_sampling_rate), float(self.opt.lr_sampling_rate) / 2.0
        tops = [float(measure['packed'][32 * i:32 * i + 8].view(torch.float64)[0]) for i in range(measure['clips'])]
        hz = [k * rate / bw['n_fft'] if k >= 0 else 0.0 for k in tops] + [None]
        return {'input': hz[0], 'output': hz[1], 'original': hz[2], 'lr_nyquist': nyquist, 'threshold_db': bw['threshold_db'],
                'n_fft': bw['n_fft'], 'hop': bw['hop'], 'band_bins': bw['band_bins'], 'frames': measure['frames'],
                'notes': bandwidth_notes(hz[0], hz[2], nyquist)}

    def _measure_stereo(self, st, lr, sr, hr):
        """The device work of the stereo report on a two-channel file: the clip the generator was given, the generated clip and,
        where there is one, the original through the cross-spectrum and the band sums (two launches of the family "stereo" each) ->
        {'packed': their results of 64 bytes one behind the other, 'clips', 'frames'}."""
        clips = [t for t in (lr, sr, hr) if t is not None]
        packed = torch.empty((64 * len(clips),), dtype=torch.uint8, device=sr.device)
        hr_rate, lr_rate = self.opt.hr_sampling_rate, self.opt.lr_sampling_rate
        for i, clip in enumerate(clips):
            _stereo_image(clip, hr_rate, lr_rate, st, out=packed[64 * i:64 * i + 64].view(torch.float64))
        L = sr.shape[-1]
        return {'packed': packed, 'clips': len(clips), 'frames': 1 + (L - st['n_fft']) // st['hop'] if L >= st['n_fft'] else 0}

    def _stereo_result(self, st, measure):
        """The fetched measurement -> the result's 'stereo'."""
        figures = [stereo_figures(measure['packed'][64 * i:64 * i + 64].view(torch.float64).tolist()) for i in range(measure['clips'])] + [None]
        mode = self.stereo
        k = stereo_split_bin(self.opt.hr_sampling_rate, self.opt.lr_sampling_rate, st['n_fft'])
        return {'input': figures[0], 'output': figures[1], 'original': figures[2], 'split_hz': k * float(self.opt.hr_sampling_rate) / st['n_fft'],
                'n_fft': st['n_fft'], 'hop': st['hop'], 'frames': measure['frames'], 'mode': mode, 'notes': stereo_notes(figures[1], mode)}

    @staticmethod
    def _output_rate_result(rc):
        """The output-rate option -> the result's 'output_rate'."""
        p = rc['plan']
        return {'rate': rc['rate'], 'model_rate': rc['model_rate'], 'o': p['o'], 'n': p['n'], 'taps_per_phase': p['taps_per_phase'],
                'passband_hz': p['passband_hz'], 'stopband_hz': p['stopband_hz'], 'atten_db': p['atten_db']}

    def _output_rate_option(self, output_rate, who, loudness_scope, spectrogram):
        """check_output_rate for enhance_file / enhance_folder -> (rc, the rate the output stage runs at)."""
        rc = check_output_rate(output_rate, self.opt.hr_sampling_rate, who, loudness_scope, spectrogram)
        return rc, (self.opt.hr_sampling_rate if rc is None else rc['rate'])

    @staticmethod
    def _loudness_at(loud, rc, who):
        """With the output-rate option the loudness option learns the rate the generated clip is measured at, which must be one the
        K-weighting entry takes."""
        return loud if loud is None or rc is None else dict(loud, out_rate=check_loudness_rate(rc['rate'], who))

    def _options(self, who, folder, *, encoding, clip, ceiling_dbfs, dither, dither_seed, report_peaks, spectrogram, spectrogram_channel,
                 spectrogram_opts, loudness, loudness_max_gain_db, true_peak, limiter, limiter_lookahead_ms, limiter_hold_ms, loudness_range,
                 loudness_scope, bandwidth, bandwidth_opts, stereo_report, stereo_report_opts, output_rate, dither_curve, dither_chunk,
                 container, flac_block, flac_md5, flac_lpc, speech_level, speech_level_max_gain_db, album_cache_bytes=None):
        """The options of enhance_file (`folder` False) / enhance_folder (True), validated before a file is opened -> _Options.
        Each is handed over under the name the entry point has it by (_named): none can take another's place, and one that is
        left out is a TypeError.  The order of the checks decides which ValueError a bad combination raises first: it does not
        move.  container None reads as 'wav'."""
        hr_rate = self.opt.hr_sampling_rate
        container = 'wav' if container is None else container
        bw = check_bandwidth(bandwidth, bandwidth_opts, loudness_scope, who)
        st = check_stereo_report(stereo_report, stereo_report_opts, loudness_scope, who)
        stage = check_output_options(encoding, clip, ceiling_dbfs, dither, dither_seed, report_peaks, who, dither_curve, dither_chunk)
        rc, out_rate = self._output_rate_option(output_rate, who, loudness_scope, spectrogram)
        check_dither(dither, encoding, who, out_rate, dither_curve, dither_chunk)
        stage, tp, lim = self._limiter_option(limiter, limiter_lookahead_ms, limiter_hold_ms, true_peak, stage, encoding, out_rate, who)
        spec = self._spectrogram_spec(spectrogram, spectrogram_channel, spectrogram_opts, who)
        loud = self._loudness_at(check_loudness(loudness, hr_rate, who, loudness_max_gain_db, loudness_range), rc, who)
        album = check_loudness_scope(loudness_scope, loud, who, folder, limiter, spectrogram, album_cache_bytes)
        fl = check_container(container, flac_block, flac_md5, encoding, out_rate, who, **_set(flac_lpc=flac_lpc))
        sl = check_speech_level(speech_level, who, speech_level_max_gain_db, loudness)
        if sl is not None:
            check_speech_level_rate(hr_rate, who)
            if rc is not None:
                sl = dict(sl, out_rate=check_speech_level_rate(rc['rate'], who))
        return _Options(stage, tp, lim, spec, loud, bw, st, rc, album, fl, sl)

    # -- one file: the stages of the flow, in the order their launches take on the stream ------------------------------
    def _front(self, read, is_lr_input, channels, encoding, o, who):
        """(a) What _read returned -> the checks that need the file's header, decode, the low-rate round trip, enhance_lr ->
        the _File.  `who`: "enhance_file" on the per-file path, also from a folder; "enhance_folder" from the album."""
        lr, hr, meta = self._front_clip(read, is_lr_input, channels, encoding, o, who)
        clip = self.enhance_lr(lr)
        # norm_scope 'clip', segment_norm: this file's ranges, on the device; crossover_hz 'auto': the crossover this file got
        return _File(clip, lr, hr, meta, self.last_norm, dict(self.last_crossover) if self.crossover_auto else None)

    def _front_clip(self, read, is_lr_input, channels, encoding, o, who):
        """_front's part in front of enhance_lr -> (the clip the generator is given, the original or None, the input's info)."""
        from ..data import audio_dataset                                    # (looked up per call: the tests replace lr_round_trip)
        host, meta, slot = read
        check_encoding(encoding, who)
        k = select_channels(channels, meta.num_channels)
        self._check_written_channels(o, channels, meta.num_channels)
        # only here, not in _open: in a folder it ends the run where the other channel limits skip the file; the speech
        # level, checked above, excludes loudness, so the two never compete for which comes first
        if o.loud is not None and k > LOUDNESS_MAX_CHANNELS:
            raise ValueError("loudness is measured over at most %d channels, %d would be written" % (LOUDNESS_MAX_CHANNELS, k))
        rate = meta.sample_rate
        raw = self._decode(host, meta, slot)[:k]
        lr = audio_dataset.lr_round_trip(raw, rate, self.opt.lr_sampling_rate, self.opt.hr_sampling_rate, is_lr_input)
        has_hr = not is_lr_input and int(rate) == int(self.opt.hr_sampling_rate)
        if has_hr:
            lr = lr[..., :raw.shape[-1]]                                    # the round trip rounds the length up
        return lr, raw if has_hr else None, meta

    def _measure(self, f, o, levels):
        """The measurements of _MEASURED with this `levels` whose option is on, queued in the table's order -> key -> the
        measurement.  One that is taken at one channel count only is left out for a file written with another."""
        taken = {}
        for m in _MEASURED:
            option = getattr(o, m.field)
            if m.levels != levels or option is None or m.channels not in (None, f.clip.shape[0]):
                continue
            taken[m.key] = getattr(self, m.measure)(option, f.lr, f.clip, *(() if levels else (f.hr,)))
            if levels and option['mode'] != 'report':
                f.clip = f.clip * taken[m.key]['gain']
        return taken

    def _reports(self, f, o):
        """(b) The bandwidth and the stereo measurement -> key -> the measurement, for those that are on.  Both see the generated
        clip behind the crossover and the mid/side decode and in front of the loudness gain: the figures are relative, a gain
        does not move them.  A file written with another channel count than two has no stereo image."""
        return self._measure(f, o, False)

    def _metrics(self, f, extended_metrics):
        """(c) Where the input is a full-band original: f.metrics, one 7-tuple per written channel, and with `extended_metrics`
        f.ext -- every written channel in one call and one copy back, the 7-tuples read off the same rows."""
        from ..util import util as U
        if f.hr is not None and extended_metrics:
            f.ext = U.compute_matrics_ext(f.hr, f.lr, f.clip, self.opt)
            f.metrics = [(e['mse'], e['snr_sr'], e['snr_lr'], 0, 0, 0, e['lsd']) for e in f.ext]
        elif f.hr is not None:
            f.metrics = [U.compute_matrics(f.hr[c:c + 1], f.lr[c:c + 1], f.clip[c:c + 1], self.opt) for c in range(f.hr.shape[0])]

    def _level(self, f, o):
        """(d) The output rate, then the loudness or the speech-level measurement (the options exclude each other: one gain) and its
        gain on f.clip -> key -> the measurement, for the one that is on.  The converter
        (one launch of the family "rateconv") sits behind everything that compares the generated clip with the input and the
        original at the model's rate; the loudness stage behind the metrics, which moment-match and stay those of the unscaled
        clip.  Both sit in front of everything that sees the written level."""
        if o.rc is not None:
            f.clip = rate_convert(f.clip, o.rc['model_rate'], o.rc['rate'], o.rc['plan'])
        return self._measure(f, o, True)

    def _present(self, o, extended_metrics):
        """Which of the optional keys (_RECORD_KEYS) this run's results and records carry: key -> bool.  The one table behind a
        blank record and a result, so that a skipped file's record has the keys an enhanced one's has."""
        return dict(metrics_ext=bool(extended_metrics), output=o.stage is not None, spectrogram=o.spec is not None, loudness=o.loud is not None,
                    speech_level=o.sl is not None, album=o.album is not None, bandwidth=o.bw is not None, crossover=self.crossover_auto,
                    stereo=o.st is not None, output_rate=o.rc is not None, norm=self.norm_scope == 'clip' or self.segment_norm,
                    flac=o.flac is not None)

    def _deliver(self, f, path_out, encoding, extended_metrics, o, measured, picture):
        """(f) _write -- the output stage, the encoder, the one synchronisation and the file -- where there is anything to encode
        or to bring back, then enhance_file's result: the five keys it always has, then those of _RESULT_KEYS that are present.
        `measured`: what _reports and _level queued."""
        output = None
        flac = o.flac and dict(o.flac)
        if path_out is not None or o.stage is not None or picture is not None or measured:
            output = self._write(path_out, f.clip, encoding, o.stage, **measured, **_set(
                picture=picture, true_peak=o.tp and dict(o.tp), limiter=o.lim and dict(o.lim),    # (one file's: they take the file's buffers)
                rate=o.rc and o.rc['rate'], flac=flac))
        # where a present key's value comes from, read behind _write; a measurement that was not taken (the stereo image of a file
        # not written with two channels) is None
        source = {'norm': lambda: f.norm, 'spectrogram': lambda: self._save_picture(o.spec, picture), 'crossover': lambda: f.crossover,
                  'output_rate': lambda: self._output_rate_result(o.rc), 'metrics_ext': lambda: f.ext, 'output': lambda: output,
                  'flac': lambda: flac.get('result')}                       # (None where no file was asked for)
        for m in _MEASURED:
            source[m.key] = lambda m=m: getattr(self, m.result)(getattr(o, m.field), measured[m.key]) if m.key in measured else None
        res = {'sr': f.clip, 'lr': f.lr, 'hr': f.hr, 'metrics': f.metrics, 'info': f.meta}
        present = self._present(o, extended_metrics)                        # (without an option: no key more than before)
        res.update((key, source[key]()) for key in _RESULT_KEYS if present[key])
        return res

    def _enhance_payload(self, read, path_out, is_lr_input, channels, encoding, extended_metrics, o):
        """One file from its bytes (what _read returned) to the written output -> enhance_file's result, with 'metrics' in one
        shape: a list with one 7-tuple per written channel, or None.  `o`: the _Options, its stage and spectrogram this file's."""
        return self._finish(self._front(read, is_lr_input, channels, encoding, o, "enhance_file"), path_out, encoding, extended_metrics, o)

    def _finish(self, f, path_out, encoding, extended_metrics, o):
        """Stages (b) to (f) of one file behind its enhance_lr -> enhance_file's result."""
        measured = self._reports(f, o)
        self._metrics(f, extended_metrics)
        measured.update(self._level(f, o))
        picture = None if o.spec is None else self._render_picture(o.spec, f.lr, f.clip, f.hr)       # (e)
        return self._deliver(f, path_out, encoding, extended_metrics, o, measured, picture)

    # -- a folder: what both loudness scopes share ---------------------------------------------------------------
    def _blank_record(self, rel, path_out, written_from, extended_metrics, o):
        """The record of a file that nothing is known of yet: the eight keys every record has, 'written' (with input_formats: the
        output's path relative to the folder `written_from`; None: no such key), and one key of _RECORD_KEYS, None, per option
        that is on."""
        rec = {'path': rel, 'rate': None, 'channels': None, 'frames': None, 'written_channels': 0, 'out_frames': 0, 'metrics': None, 'error': None}
        if written_from is not None:
            rec['written'] = os.path.relpath(path_out, written_from)
        present = self._present(o, extended_metrics)
        rec.update((key, None) for key in _RECORD_KEYS if present[key])
        return rec

    @staticmethod
    def _fill_record(rec, res):
        """The record of an enhanced file <- enhance_file's result, or as much of one as there is (the album's phase A)."""
        meta = res['info']
        rec.update(rate=meta.sample_rate, channels=meta.num_channels, frames=meta.num_frames, written_channels=res['sr'].shape[0],
                   out_frames=res['sr'].shape[-1], metrics=res['metrics'])
        rec.update((key, res[key]) for key in _RECORD_KEYS if key in rec and key in res)

    def _open(self, path_in, channels, verify_input, o, rec, slot=None):
        """_read and the checks that make a skipped file -> what _read returned, or None with the reason in rec['error'].  `slot`:
        None, or the pinned buffer to read into where it is not _read's own."""
        try:
            read = self._read(path_in, **_set(slot=slot, verify=True if verify_input else None))
            self._check_written_channels(o, channels, read[1].num_channels)
            return read
        except (ValueError, OSError, EOFError, struct.error) as e:
            rec['error'] = '%s: %s' % (type(e).__name__, e)
            return None

    def enhance_file(self, path_in, path_out=None, is_lr_input=False, channels='first', encoding='pcm16', extended_metrics=False,
                     clip='clamp', ceiling_dbfs=None, dither=None, dither_seed=0, report_peaks=False, spectrogram=None,
                     spectrogram_channel=0, spectrogram_opts=None, loudness=None, loudness_max_gain_db=None, true_peak=False,
                     limiter=False, limiter_lookahead_ms=None, limiter_hold_ms=None, loudness_range=False, loudness_scope='file',
                     bandwidth=False, bandwidth_opts=None, stereo_report=False, stereo_report_opts=None, output_rate=None, dither_curve=None,
                     dither_chunk=None, verify_input=False, container='wav', flac_block=None, flac_md5=False, flac_lpc=None, speech_level=None,
                     speech_level_max_gain_db=None, pack_files=1, stream_seconds=None):
        """wav -> the low-rate round trip of AudioTestDataset (or, with `is_lr_input`, a plain upsample of a clip that is
        already band-limited) -> enhance_lr -> wav at opt.hr_sampling_rate.  `channels`: 'first' (the default), 'all', or an
        int N (the first N).  `encoding` of the output: 'pcm16' | 'pcm24' | 'float32'.  The data chunk is decoded and the
        output encoded on the device (csrc/pcm.hip).  Returns {'sr', 'lr', 'hr', 'metrics', 'info'}: [C, L] tensors on the GPU;
        'hr' and 'metrics' are None unless the input is a full-band clip at the high rate; 'metrics' is
        util.compute_matrics against the input with 'first', else a list with one such 7-tuple per written channel, each
        computed on that channel alone; 'info' is the input's wavio.WavInfo.  A FLAC input (told by its first bytes, not its name) is
        read as it stands: its bytes and frame index are copied and csrc/flac.hip decodes them on the device (two launches of the
        family "flac" in place of the PCM decoder's one); 'info' is then its flacio.FlacInfo, everything else is what the same
        samples in a wav give.  An AIFF / AIFF-C, AU or NIST SPHERE input (first bytes 'FORM', '.snd', 'NIST'; data/containers.py) is
        read as it stands too: one copy and one decoder launch, 'info' is its containers.AudioInfo, the rest is what its WAV twin
        gives; a coding that is not read is a ValueError that names file and coding.  `verify_input`: a FLAC input is first decoded
        on the host and refused with a ValueError where its samples do not have STREAMINFO's MD5.  `extended_metrics`: the result gains
        'metrics_ext', util.compute_matrics_ext of all written channels from one device call -- a list with one dict
        (util.METRIC_ROW_NAMES -> float) per written channel, also with 'first'; None where 'metrics' is None -- and 'metrics'
        holds the same rows' figures.
        The output stage (all opt-in; 'sr' and the metrics are the unscaled clip whatever it does, only the written bytes
        change).  `clip`: 'clamp' (default: the integer encodings clamp to their range, silently), 'guard' (the whole file, all
        channels alike, is scaled down so that its peak sits at `ceiling_dbfs` -- None: the encoding's own limit; a file that
        fits is left alone) or 'error' (ClipError, a ValueError, naming the file, its peak and the clipped count, before anything is
        written).  `dither`: None or 'tpdf' (pcm16 only: +-1 LSB of triangular noise in front of the rounding, fixed by
        `dither_seed`), or 'shaped' (pcm16 written at 44100 or 48000 Hz only; csrc/shaper.hip, one launch of the family "shaper" in
        place of the encoder's): the same noise in front of an error-feedback quantiser that moves the 16-bit floor out of 2-5 kHz
        and up above 15 kHz -- `dither_curve`: a name of plans.DITHER_CURVES (None: 'lipshitz9'); `dither_chunk`: samples after
        which the error history starts again at zero, which is what makes the recursion parallel and part of what is computed
        (None: 4096; a multiple of 64 in [256, 2^20]; one at least as long as the clip is the plain sequential recursion).  'output'
        then gains 'dither': {'kind', 'curve', 'taps' (how many), 'chunk'}.  Another written rate, or either option without
        'shaped', is a ValueError before the file is opened.
        `report_peaks`: measure only.  With any of the five given the result gains 'output': {'peak',
        'peak_dbfs', 'clipped', 'nonfinite' (a list each, one entry per written channel, measured on the unscaled clip for
        `encoding`), 'gain' (the factor applied: 1.0 unless 'guard' scaled)}.
        `spectrogram` (opt-in): path of a PNG to write after the wav -- spectrogram_image of written channel
        `spectrogram_channel`: the input the generator was given ('lr'), the generated clip ('sr', what is encoded into the wav)
        and, where the result has one, the original ('hr'), top to bottom on one time, frequency and dB scale.
        `spectrogram_opts`: None or a dict of n_fft, hop, width, height, range_db, gap, top_db (plans.check_spectrogram).  The
        picture is rendered on the device (two launches, family "specimg") and comes back with the payload behind the same
        synchronisation.  The result gains 'spectrogram': {'path', 'panels', 'frames', 'bins', 'top_db' (the level of the
        palette's last colour), 'range_db'}.  A channel that is not among the written ones is a ValueError, before anything is
        enhanced or written.
        `loudness` (opt-in): the integrated loudness after ITU-R BS.1770-4 / EBU R 128 (csrc/loudness.hip; K-weighting, 400 ms
        blocks, gates at -70 LUFS and 10 LU under the ungated mean; all written channels as one programme, weights
        plans.loudness_channel_weights) of the clip the generator was given ('lr') and of the generated clip, and what is done
        with it: 'report' measures only; 'input' makes the written clip as loud as 'lr'; a number in [-70, 0] makes it that loud,
        in LUFS.  The gain, at most `loudness_max_gain_db` either way (None: 40 dB), multiplies the clip on the device in front of
        the output stage: the peak report, the clip guard, the dither, the encoder, the picture and the result's 'sr' see the written
        level; 'metrics' and 'metrics_ext' are those of the clip in front of the gain.  Four launches of the family "loudness" per
        file; the figures come back with the payload behind the same synchronisation.  The result gains 'loudness': {'input',
        'measured' (the generated clip in front of the gain), 'gain_db', 'output' (= measured + gain_db, the written clip unless the
        output stage scales or clamps it), 'momentary_max' (the loudest 400 ms block of the written clip), 'target' (the level
        aimed at, None with 'report')}, in LUFS; -inf for a clip shorter than 400 ms or a silent one, which is left as it is.  A
        high rate that is not a multiple of 10 in [8000, 384000] Hz is a ValueError before the file is opened.
        `loudness_range` (opt-in, a bool; an option of `loudness`): also measure the loudness range after EBU Tech 3342 of both
        clips and the maximum short-term loudness of the generated one, from the hop energies the loudness measurement already has:
        3 s blocks at a 100 ms step, gates at -70 LUFS and 20 LU under the mean of what passed, the 10th to the 95th percentile of
        what is left (exact order statistics, found on the device).  At most four launches more; the figures travel in the same
        buffer behind the same synchronisation.  'loudness' gains 'range': {'input', 'output' (LU), 'low', 'high' (the two
        percentile levels), 'threshold' (the relative gate), 'blocks' (behind both gates), 'short_term_max'}; 'low' to
        'short_term_max' are the generated clip's, in LUFS, and all of them include the loudness gain: they describe the clip as
        the loudness stage leaves it, like 'output'.  The limiter and the clip guard act behind this point, so a limited file's
        range can be smaller than the figure, just as its integrated loudness can.  A clip under 3 s has range 0.0 and levels
        -inf; a clip with a NaN block has range NaN.  Without `loudness` it is a ValueError before the file is opened.
        `true_peak` (opt-in, a bool): also measure the true peak after ITU-R BS.1770-4 Annex 2 (csrc/truepeak.hip: the clip
        oversampled to at least 192 kHz, plans.truepeak_plan) where the peak is measured -- on the clip the encoder sees, behind the
        loudness gain and the crossover.  The result's 'output' -- which then exists also with every other output option at its
        default -- gains 'true_peak' (linear) and 'true_peak_dbtp', a list each with one entry per written channel, measured on the
        unscaled clip like 'peak'.  clip 'guard' then takes its gain from the true peak: `ceiling_dbfs` is read as dBTP (None: the
        encoding's limit) and 'gain' reports it; clip 'error' also refuses a file whose samples fit but whose true peak exceeds the
        encoding's limit; 'clamp' only reports.  One launch of the family "truepeak" per file; the figures come back with the payload
        behind the same synchronisation.
        `limiter` (opt-in, a bool; an option of clip='guard'): a look-ahead true-peak limiter (csrc/limiter.hip) in front of the
        guard.  Where a few crests stand over `ceiling_dbfs`, the guard alone scales the whole file down by the excess; the limiter
        turns only the crests down -- one gain curve for all channels, the smoothed minimum of what every sample and the oversampled
        crests next to it need, looking `limiter_lookahead_ms` ahead (None: 5 ms) and held for `limiter_hold_ms` (None: 20 ms;
        plans.limiter_plan) -- and the loudness just reached stays.  It switches the true-peak measurement on as `true_peak` does.
        The guard's one gain then runs on the limited clip and removes what is left, normally a rounding.  Two launches of the family
        "limiter" per file, in front of the peak kernels; the figures come back with the payload behind the same synchronisation.
        'output' gains 'limiter': {'lookahead', 'hold' (samples), 'max_reduction_db' (the curve's lowest point, <= 0),
        'limited_samples' (samples with a gain under 1), 'input_true_peak_dbtp' (the true peak in front of the limiter)}; its 'peak',
        'true_peak' and 'clipped' are then those of the limited clip and its 'gain' the guard's residual gain.  'sr' and the metrics
        stay the clip in front of the output stage.  Anything but clip='guard' with it is a ValueError before the file is opened.
        `loudness_scope`: 'file'.  'folder' -- one gain for a whole folder -- is an option of enhance_folder and a ValueError here.
        `bandwidth` (opt-in, a bool): where the band of each clip actually ends (csrc/bandwidth.hip) -- of the clip the generator was
        given ('lr'), of the generated clip (behind the crossover, in front of the loudness gain: the figure is relative to the clip's
        own strongest band, so a gain does not move it) and, where the result has one, of the original: the long-term average
        spectrum over the frames that lie wholly inside the clip (all written channels one programme), the levels of bands of
        `band_bins` bins, and the highest bin of the highest band that stands within `threshold_db` of the strongest band.
        `bandwidth_opts`: None or a dict of n_fft, hop, band_bins, threshold_db (plans.check_bandwidth; BANDWIDTH_DEFAULTS).  At
        most six launches of the family "bandwidth" per file; the three results of 32 bytes come back with the payload behind the
        same synchronisation.  The result gains 'bandwidth': {'input', 'output', 'original' (Hz, k_top * rate / n_fft; 0.0 where
        nothing passed -- silence, a clip shorter than n_fft; 'original' None without one), 'lr_nyquist', 'threshold_db', 'n_fft',
        'hop', 'band_bins', 'frames', 'notes' (a list of strings: an input whose band ends under 0.9 of the low rate's Nyquist
        frequency; an original whose band ends at or under 1.05 times it, so that LSD-HF compares against an empty band)}.
        With SuperResolver(crossover_hz='auto') -- whatever `bandwidth` is -- the result gains 'crossover': {'hz', 'taps', 'edge_hz'},
        the crossover this clip got.
        `stereo_report` (opt-in, a bool): the stereo image of a file written with exactly two channels (csrc/stereo.hip) -- how its
        left and right channel relate below and above the low rate's Nyquist frequency, for the clip the generator was given, for the
        generated clip (behind the crossover and the mid/side decode, in front of the loudness gain, where the bandwidth report
        measures) and, where the result has one, for the original: the long-term cross-spectrum over the frames wholly inside the
        clip, summed over the bins below the split and over those at and above it (plans.stereo_split_bin), and on the host
        plans.stereo_figures of the eight sums.  `stereo_report_opts`: None or a dict of n_fft, hop (plans.check_stereo_report;
        STEREO_DEFAULTS).  At most six launches of the family "stereo" per file; the three results of 64 bytes come back with the
        payload behind the same synchronisation.  The result gains 'stereo': {'input', 'output', 'original' ({'low', 'high'}, each
        {'corr', 'coherence', 'side_db', 'balance_db'}; 'original' None without one), 'split_hz', 'n_fft', 'hop', 'frames', 'mode'
        (the object's `stereo`), 'notes' (a list of strings: with mode 'lr', a generated clip whose correlation above the split is
        more than STEREO_NOTE_DROP under the one below it)}; None for a file written with another channel count.
        `output_rate` (opt-in; None or opt.hr_sampling_rate: nothing changes): write the file at this rate, an int >= 8000 Hz, 44100
        for instance.  The generated clip goes through a rational polyphase converter (csrc/rateconv.hip; ops.rateconv_plan: a
        Kaiser-windowed sinc, flat to 0.907 of the lower rate's Nyquist frequency, 120 dB down from where aliases or images would fold
        under it) behind the metrics, the bandwidth and the stereo report, which compare the clips at the model's rate, and in front
        of the loudness measurement of the generated clip, the true-peak measurement, the limiter, the guard and the encoder, which
        all run on the converted clip at the output rate: the loudness, the true peak and the dither of the delivered file are the
        ones this stage set.  The input's loudness is still measured at the model's rate.  One launch of the family "rateconv" per
        file.  'sr' is then the clip at the output rate ('lr' and 'hr' stay at the model's) and the result gains 'output_rate':
        {'rate', 'model_rate', 'o', 'n' (the two rates over their common divisor), 'taps_per_phase', 'passband_hz', 'stopband_hz',
        'atten_db'}.  Not built with `spectrogram` or loudness_scope 'folder'; rates between which the filter is not built (48000 ->
        8000, or a pair with a tiny common divisor) are refused: a ValueError each, before the file is opened.
        `container`: 'wav' (default: nothing changes) or 'flac': the payload the encoder leaves on the device -- with the guard's
        gain, the limiter, the dither and the output rate in it -- goes through the FLAC encoder there (csrc/flacenc.hip, three
        launches of the family "flacenc"; the stream contract of include/p2phd.h: CONSTANT, VERBATIM and FIXED subframes, Rice
        partitions, the four stereo assignments, every choice on exact bit counts), so that the file, decoded, is the data chunk the
        wav would have held, byte for byte.  The frames come back at their worst-case size -- about what the wav path copies -- with
        their lengths behind the same one synchronisation, and the host writes "fLaC", STREAMINFO and the frames.  `flac_block`:
        samples per frame, 16 .. 65535 (None: 4096).  `flac_md5`: also bring the payload back (a second copy of its size) and write
        its MD5 into STREAMINFO, which is otherwise zeros ("not computed").  `flac_lpc`: None, or the largest LPC order M in 0 .. 12 the
        encoder tries beside the fixed predictors (include/p2phd.h, "FLAC output, LPC": every order 1 .. M, chosen on exact bit counts,
        the file never longer than without it; flac_block at most 16384 with M > 0); 'flac' then gains 'lpc': M.  The result gains 'flac': {'block', 'frames', 'bytes'
        (the file's), 'pcm_bytes' (the payload's), 'md5' (hex, or None)}; None where no file is written.  encoding 'float32', more
        than 8 written channels, a block outside the range, a written rate above 1048575 Hz, or either option without 'flac': a
        ValueError before the output is opened.
        `speech_level` (opt-in): the active speech level after ITU-T P.56 method B (csrc/speechlevel.hip; include/p2phd.h, "Active
        speech level": the level while somebody is speaking, in dBov, with a 200 ms hangover, and the activity factor) of the clip the
        generator was given ('lr', at the model's rate) and of the generated clip (behind the output-rate converter, at the rate
        written), and what is done with it: 'report' measures only; 'input' brings the written clip to the input's active level; a
        number in [-70, 0] brings it to that level in dBov (-26 is the convention of speech corpora and listening tests).  Every
        channel is measured on its own; the file's figure is that of the channel with the highest active level and ONE gain, at most
        `speech_level_max_gain_db` either way (None: 40 dB; 0 .. 120), multiplies all channels where the loudness gain would -- in
        front of the true-peak measurement, the limiter, the guard, the dither and the encoder; 'sr' is the scaled clip.  Six
        launches of the family "speechlevel" per file; the figures come back with the payload behind the same synchronisation.
        The result gains 'speech_level': {'input' (the input's active level), 'measured' (the generated clip's in front of the
        gain), 'gain_db', 'output' ('measured' + 'gain_db'), 'target' (None with 'report'), 'long_term' and 'activity' (the
        generated clip's, the level with the gain), 'activity_input', 'channels': [{'active', 'long_term', 'activity'}, ..] (the
        generated clip's rows, with the gain)}.  A clip without activity has the level -inf and the gain 1.  Not together with
        `loudness` (two claims on one gain), not over more than 8 written channels, and only at rates in 8000 .. 192000: a
        ValueError each, the first and the last before a file is opened.
        `pack_files`: 1.  More -- files that share generator groups -- is an option of enhance_folder and a ValueError here, before
        the file is opened; the two entry points take the same options.
        `stream_seconds` (opt-in, an option of SuperResolver(segment_norm=True); None, the default: nothing changes): the file goes
        through the pipeline in windows of about this many seconds (generate/stream.py; plans.stream_plan: whole segments, whole
        groups) -- each read, decoded, taken through the low-rate round trip, gathered, generated, stitched (csrc/stitch.hip,
        p2phd_segments_stitch_stream: two launches of the family "stitch" per window), encoded and appended to the output while the
        next is read -- so that device and pinned memory are a window's whatever the file's length and the first bytes are written
        when the second window is queued.  The written file is byte for byte the one written without the option where the model
        draws no mask noise and a row of the generator does not depend on its batch neighbours; a group's noise is one torch.randn
        drawn in window order, the unstreamed order with one written channel only.  The result's 'sr', 'lr', 'hr' and 'metrics' are
        None -- no clip is kept and nothing is compared --, 'norm' is the [C, S, 2] tensor as ever and the result gains 'stream':
        {'windows', 'segments_per_window', 'groups', 'frames', 'out_frames', 'window_seconds'}.  Only samples of a fixed size stream
        (PCM, float, G.711; WAV, AIFF, AU, SPHERE): a FLAC or IMA ADPCM input is a ValueError naming file and coding.  Not built with
        anything that needs the whole clip or a figure of the whole file (plans.check_stream: the crossover, loudness, speech_level,
        clip other than 'clamp', true_peak, limiter, report_peaks, spectrogram, bandwidth, stereo_report, output_rate,
        extended_metrics, container 'flac', dither 'shaped', pack_files > 1, loudness_scope 'folder'), and not without
        segment_norm: a ValueError each, before the file is opened."""
        o = self._options("enhance_file", False, **_named(locals()))
        if check_pack_files(pack_files, self.segment_norm, loudness_scope, "enhance_file") > 1:
            raise ValueError("enhance_file: pack_files %d lets the files of a folder share groups: it is an option of enhance_folder" % pack_files)
        window = self._stream_option("enhance_file", stream_seconds, locals())
        if window is not None:
            return self._enhance_stream(path_in, path_out, is_lr_input, channels, encoding, o, window)
        read = self._read(path_in, **_set(verify=True if verify_input else None))
        res = self._enhance_payload(read, path_out, is_lr_input, channels, encoding, extended_metrics, o)
        res['metrics'] = first_channel_metrics(res['metrics'], channels)
        return res

    def _stream_option(self, who, stream_seconds, local):
        """check_stream for enhance_file / enhance_folder, on the entry point's own arguments -> None (off), or the window in seconds."""
        names = ('loudness', 'speech_level', 'clip', 'true_peak', 'limiter', 'report_peaks', 'spectrogram', 'bandwidth', 'stereo_report',
                 'output_rate', 'extended_metrics', 'container', 'dither', 'pack_files', 'loudness_scope')
        return check_stream(stream_seconds, who, self.segment_norm, getattr(self, 'crossover', None), self.opt.hr_sampling_rate,
                            **{name: local[name] for name in names})

    @staticmethod
    def _spectrogram_spec(path, channel, opts, who):
        """Validates the spectrogram option -> None (off), or {'path', 'channel', 'top_db', 'plan'}."""
        if path is None:
            if channel != 0 or opts is not None:
                raise ValueError("%s: spectrogram_channel / spectrogram_opts are options of spectrogram=PATH; spectrogram is None" % who)
            return None
        opts = dict(opts or {})
        top_db = opts.pop('top_db', None)
        unknown = sorted(set(opts) - {'n_fft', 'hop', 'width', 'height', 'range_db', 'gap'})
        if unknown:
            raise ValueError("%s: unknown spectrogram_opts %s" % (who, unknown))
        return {'path': os.fspath(path), 'channel': channel, 'top_db': top_db,
                'plan': check_spectrogram(top_db=top_db, channel=channel, who=who, **opts)}

    def enhance_folder(self, dir_in, dir_out, is_lr_input=False, channels='first', encoding='pcm16', seed=None, report=None,
                       extended_metrics=False, clip='clamp', ceiling_dbfs=None, dither=None, dither_seed=0, report_peaks=False,
                       spectrogram=None, spectrogram_channel=0, spectrogram_opts=None, loudness=None, loudness_max_gain_db=None,
                       true_peak=False, limiter=False, limiter_lookahead_ms=None, limiter_hold_ms=None, loudness_range=False,
                       loudness_scope='file', album_cache_bytes=None, bandwidth=False, bandwidth_opts=None, stereo_report=False,
                       stereo_report_opts=None, output_rate=None, dither_curve=None, dither_chunk=None, input_formats=None,
                       verify_input=False, container='wav', flac_block=None, flac_md5=False, flac_lpc=None, speech_level=None,
                       speech_level_max_gain_db=None, pack_files=1, stream_seconds=None):
        """Every *.wav under dir_in (plan_folder: sorted, recursive) -> the same relative path under dir_out, with one model
        and one captured graph for the whole run.  A file that does not parse is reported and skipped.  `seed`: re-seed the
        generator in front of every file, so that a file comes out as a run of its own with that seed would write it.
        `report(record)` is called after every file.  Returns one record per file: {'path' (relative), 'rate', 'channels',
        'frames' (of the input), 'written_channels', 'out_frames', 'metrics' (as enhance_file(channels != 'first') returns
        them: a list per channel, or None), 'error' (None, or the text of what went wrong)}; with `extended_metrics` also
        'metrics_ext' (as enhance_file returns it).  `clip`, `ceiling_dbfs`, `dither`, `dither_seed`, `report_peaks`: the output
        stage of enhance_file, per file (a guard gain is one file's); file k of the plan is dithered with seed `dither_seed` + k
        (`dither_curve`, `dither_chunk`: enhance_file's, for dither 'shaped', in either loudness scope);
        with any of them given a record gains 'output' (as enhance_file returns it, None for a skipped file).  clip 'error'
        ends the run at the first file that would clip.  `spectrogram`: a folder that takes one picture per enhanced file, at
        <relative path>.png (enhance_file's `spectrogram`, `spectrogram_channel`, `spectrogram_opts`); a record then gains
        'spectrogram' (as enhance_file returns it; None for a skipped file).  A file without channel `spectrogram_channel` is
        reported like one that does not parse: its record carries the 'error' and neither its wav nor its picture is written.
        `loudness`, `loudness_max_gain_db`, `loudness_range`: enhance_file's, per file (every file is measured and normalised on its own, unless `loudness_scope` says otherwise); a record
        then gains 'loudness' (as enhance_file returns it; None for a skipped file).  `true_peak`: enhance_file's, per file; a
        record's 'output' then carries the true-peak figures.  `limiter`, `limiter_lookahead_ms`, `limiter_hold_ms`: enhance_file's,
        per file; a record's 'output' then carries 'limiter'.
        `loudness_scope` (an option of `loudness`): 'file' (default: the above), or 'folder': the folder is one programme, as EBU R 128
        normalises an album (generate/album.py).  Every enhanced file's clip contributes its own 400 ms blocks (a block never spans
        two files; its file's channel weights), both gates run over the union of them, for the generated clips and for the inputs
        the generator was given, and one loudness gain -- towards the target, or with 'input' towards the inputs' album loudness,
        clamped as above -- multiplies every file: the level differences between the files survive.  With clip 'guard' there is one
        guard gain too: the largest peak (with `true_peak`: true peak) of any file behind the loudness gain sits at the ceiling.
        With clip 'error' a folder in which any file would clip writes no file at all; the ClipError names the first such file of
        the plan.  Every file is generated and measured before the first is written: the generated clips wait on the device while
        they total at most `album_cache_bytes` (None: 4 GiB; 0: none) and on the host beyond that.  Six launches of the family
        "loudness" per file and two per folder; one synchronisation brings back every figure of the folder, then one per file
        written, as before.  A record's 'loudness' keeps its keys: 'input' and 'measured' are the track's own, 'gain_db' is the
        album's, 'output' = 'measured' + 'gain_db', 'target' is the album's; a record gains 'album', the same dict in every
        enhanced file's record (None for a skipped file): {'input', 'measured', 'gain_db', 'output', 'target' (the album's levels in
        LUFS), 'files', 'blocks_in', 'blocks_out' (blocks of the inputs and of the generated clips), 'kept' (blocks of the generated
        clips behind both gates)}; with an output stage its 'output' carries the folder's guard gain as 'gain' beside the file's own
        peak figures.  `report` is called file by file in phase C, when the file has been written.  `limiter`, `loudness_range` and
        `spectrogram` are not built for this scope: a ValueError each, as is the scope without `loudness`.
        `bandwidth`, `bandwidth_opts`: enhance_file's, per file; a record then gains 'bandwidth' (as enhance_file returns it; None for
        a skipped file).  Not built for loudness_scope 'folder' either: a ValueError.  With SuperResolver(crossover_hz='auto') a
        record gains 'crossover' (the file's; None for a skipped file), in either scope.
        `stereo_report`, `stereo_report_opts`: enhance_file's, per file; a record then gains 'stereo' (as enhance_file returns it; None
        for a skipped file and for one written with another channel count than two).  Not built for loudness_scope 'folder': a
        ValueError.  With SuperResolver(stereo='ms') a file of which more than two channels would be written is skipped, its record
        carrying the 'error', in either scope.
        `output_rate`: enhance_file's, one rate for every file; a record's 'out_frames' is then the written length at that rate and a
        record gains 'output_rate' (as enhance_file returns it; None for a skipped file).  Not built for loudness_scope 'folder' or
        with `spectrogram`: a ValueError.
        `input_formats`: None (the above: *.wav only), or the extensions to list, ('wav', 'flac') for instance (plan_folder's
        `formats`): x.flac is written as x.wav, a record then gains 'written' (the output's relative path), and two inputs that would
        be written to one path are a ValueError before any file is opened.  `verify_input`: enhance_file's, per FLAC file; a mismatch
        is a skipped file.  Both hold in either loudness scope.
        `container`, `flac_block`, `flac_md5`: enhance_file's; with 'flac' every output is named .flac (plan_folder's `ext`: x.wav is
        written as x.flac, and x.wav beside x.flac in one folder is the same ValueError), a record gains 'written' and 'flac', and
        the album flow writes through the same encoder and the same writer.
        `speech_level`, `speech_level_max_gain_db`: enhance_file's, per file; a record then gains 'speech_level' (as enhance_file
        returns it; None for a skipped file).  A file of which more than 8 channels would be written is skipped, its record carrying
        the 'error'.
        `pack_files` (an option of SuperResolver(segment_norm=True); 1, the default: nothing changes): up to this many consecutive
        files of the plan that open share generator groups (plans.pack_plan: a pack also closes before the file with which its
        float32 clips would exceed plans.PACK_MAX_BYTES; a larger file is a pack of its own; a file that does not open takes no
        place).  Every file of a pack is read into a pinned buffer of its own ('pack0', 'pack1', ..), decoded and taken through the
        low-rate round trip; one enhance_lr_many generates all of them, ceil(R / batch) groups for the R rows of the pack where file
        by file each rounds up on its own; then each file goes through the stages behind enhance_lr as ever -- its own options,
        `dither_seed` + k with k its place in the plan, its own synchronisation.  Records and `report` calls stay in plan order.  With
        `seed` a file is given the mask noise a run of its own would draw: the generator is re-seeded per file and that file's
        ceil(R_i / batch) draws of a full group are made, their first rows kept, and handed on as given noise.  A file's rows,
        ranges and noise are then bit for bit those of pack_files=1; what the generator does with the other rows of a batch is all
        that differs.  Without segment_norm, or with loudness_scope 'folder', a ValueError before a file is opened.
        `stream_seconds`: enhance_file's, file by file on the per-file flow; a record gains 'stream' (as enhance_file returns it; None
        for a skipped file) and 'norm'.  A file whose coding does not stream (FLAC, IMA ADPCM) is skipped, its record carrying the
        'error'.  The same refusals, before a file is opened."""
        o = self._options("enhance_folder", True, **_named(locals()))
        pack_files = check_pack_files(pack_files, self.segment_norm, loudness_scope, "enhance_folder")
        window = self._stream_option("enhance_folder", stream_seconds, locals())
        plan = plan_folder(dir_in, dir_out, **_set(formats=input_formats, ext='.flac' if o.flac is not None else None))
        written_from = None if input_formats is None and o.flac is None else dir_out          # a record then says where its file was written
        if o.album is not None:
            from .album import enhance_album
            return enhance_album(self, plan, written_from, is_lr_input, channels, encoding, seed, report, extended_metrics, o, dither_seed, verify_input)
        if pack_files > 1:
            return self._enhance_packed(plan, written_from, is_lr_input, channels, encoding, seed, report, extended_metrics, o, dither_seed,
                                        verify_input, pack_files)
        if window is not None:
            return self._stream_folder(plan, written_from, is_lr_input, channels, encoding, seed, report, o, dither_seed, window)
        records = []
        for k, (rel, path_in, path_out) in enumerate(plan):
            rec = self._blank_record(rel, path_out, written_from, extended_metrics, o)
            read = self._open(path_in, channels, verify_input, o, rec)
            if read is not None:
                if seed is not None:
                    torch.manual_seed(int(seed))
                mine = o._replace(stage=o.stage and dict(o.stage, seed=dither_seed + k),
                                  spec=o.spec and dict(o.spec, path=os.path.join(o.spec['path'], rel + '.png')))
                self._fill_record(rec, self._enhance_payload(read, path_out, is_lr_input, channels, encoding, extended_metrics, mine))
            records.append(rec)
            if report is not None:
                report(rec)
        return records

    def _stream_folder(self, plan, written_from, is_lr_input, channels, encoding, seed, report, o, dither_seed, window):
        """enhance_folder with stream_seconds -> the records: every file streamed on its own (generate/stream.py); one that does not
        parse, or whose coding does not stream, is a skipped file."""
        records = []
        for k, (rel, path_in, path_out) in enumerate(plan):
            rec = self._blank_record(rel, path_out, written_from, False, o)
            rec['stream'] = None
            try:
                meta = self._stream_info(path_in)
                self._check_written_channels(o, channels, meta.num_channels)
            except (ValueError, OSError, EOFError, struct.error) as e:
                rec['error'] = '%s: %s' % (type(e).__name__, e)
            else:
                if seed is not None:
                    torch.manual_seed(int(seed))
                mine = o._replace(stage=o.stage and dict(o.stage, seed=dither_seed + k))
                res = self._enhance_stream(path_in, path_out, is_lr_input, channels, encoding, mine, window)
                rec.update(rate=meta.sample_rate, channels=meta.num_channels, frames=meta.num_frames, written_channels=res['norm'].shape[0],
                           out_frames=res['stream']['out_frames'], norm=res['norm'], stream=res['stream'])
            records.append(rec)
            if report is not None:
                report(rec)
        return records

    # -- a folder whose files share groups (pack_files > 1) -----------------------------------------------------------
    def _clip_bytes(self, meta, channels):
        """The bytes of the float32 clip the generator is given for a file with this header: its written channels at the high rate."""
        frames = -(-int(meta.num_frames) * int(self.opt.hr_sampling_rate) // max(int(meta.sample_rate), 1))
        return 4 * select_channels(channels, meta.num_channels) * frames

    def _pack_noise(self, seed, clips):
        """`seed` with a pack: the mask noise of the pack's rows, every file's as a run of its own draws it -- the generator re-seeded,
        ceil(R_i / batch) draws of a full group's shape as _walk_rows makes them, the first rows of each kept.  None where the model
        draws none."""
        shape = self.noise_shape(self.batch)
        if shape is None:
            return None
        parts = []
        for lr in clips:
            rows = lr.shape[0] * segment_plan(lr.shape[-1], self.T, self.overlap)[0]
            torch.manual_seed(int(seed))
            parts.extend(torch.randn(shape, device=self.device)[:n] for _, n in group_rows_plan(rows, self.batch))
        return torch.cat(parts)

    def _enhance_packed(self, plan, written_from, is_lr_input, channels, encoding, seed, report, extended_metrics, o, dither_seed,
                        verify_input, pack_files):
        """enhance_folder with pack_files > 1 -> the records.  The files are opened in plan order; `waiting` holds, in that order, the
        records since the last pack was finished -- a file that opened with what its stages need, a skipped one with None -- and a
        pack is finished when plans.pack_plan says that the file just opened starts the next one."""
        records, waiting, sizes, opened = [], [], [], 0

        def finish(upto):
            held = [w for w in waiting[:upto] if w[1] is not None]
            if held:
                fronts = [self._front_clip(read, is_lr_input, channels, encoding, mine, "enhance_file") for _, (read, _, mine) in held]
                lrs = [lr for lr, _, _ in fronts]
                clips = self.enhance_lr_many(lrs, None if seed is None else self._pack_noise(seed, lrs))
                norms, crossovers = self.last_norm, self.last_crossovers
            i = 0
            for rec, entry in waiting[:upto]:
                if entry is not None:
                    (lr, hr, meta), (_, path_out, mine) = fronts[i], entry
                    f = _File(clips[i], lr, hr, meta, norms[i], crossovers[i])
                    self._fill_record(rec, self._finish(f, path_out, encoding, extended_metrics, mine))
                    i += 1
                if report is not None:
                    report(rec)
            del waiting[:upto]
            del sizes[:len(held)]

        for k, (rel, path_in, path_out) in enumerate(plan):
            rec = self._blank_record(rel, path_out, written_from, extended_metrics, o)
            # pack_files + 1 buffers: the file that turns out to start the next pack is read while the pack before it still holds its own
            read = self._open(path_in, channels, verify_input, o, rec, 'pack%d' % (opened % (pack_files + 1)))
            records.append(rec)
            if read is None:
                waiting.append((rec, None))
                continue
            opened += 1
            mine = o._replace(stage=o.stage and dict(o.stage, seed=dither_seed + k),
                              spec=o.spec and dict(o.spec, path=os.path.join(o.spec['path'], rel + '.png')))
            sizes.append(self._clip_bytes(read[1], channels))
            if len(pack_plan(sizes, pack_files)) > 1:                       # this file starts the next pack: finish the one before it
                finish(len(waiting))
            waiting.append((rec, (read, path_out, mine)))
        finish(len(waiting))
        return records


# The options both entry points share (and enhance_folder's album_cache_bytes): the keyword-only parameters of _options.
_OPTION_NAMES = tuple(name for name, p in inspect.signature(SuperResolver._options).parameters.items() if p.kind is p.KEYWORD_ONLY)
