"""Whole-file super-resolution: wav in, wav out, on the device from the waveform to the waveform.

The command line of whole-file generation (python -m pix2pixhdaudiosr_amd.generate; the first line above is its --help
description) and the options dump it starts from."""
import argparse
import ast
import os
import sys
from types import SimpleNamespace

import torch

from .ops import shaper_coefficients
from .plans import (check_container, check_input_formats, CLIP_MODES, CROSSOVER_AUTO, DITHER_CURVES, check_dither, dither_line, LOUDNESS_MODES, LOUDNESS_SCOPES, LOWBANDS, PCM_ENCODINGS, ClipError, check_crossover, check_limiter, check_loudness, check_loudness_scope, check_speech_level, check_speech_level_rate, SPEECH_LEVEL_MODES, check_lowband,
                    check_output_options, check_output_rate, check_paths, check_spectrogram, check_bandwidth, check_segment_norm, check_pack_files, check_stereo_report, check_stream, select_channels, stream_plan, output_rate_line, spectro_bins)
from .report import _print_album, _print_bandwidth, _print_crossover, _print_limiter, _print_loudness, _print_loudness_range, _print_speech_level, _print_metrics, _print_metrics_ext, _print_peaks, _print_stereo, _print_unwritten, metrics_rows, write_metrics_csv
from .resolver import SuperResolver, per_channel_metrics


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


def _size_arg(text):
    w, sep, h = text.lower().partition('x')
    try:
        return int(w), int(h)
    except ValueError:
        raise argparse.ArgumentTypeError("expected WIDTHxHEIGHT in pixels, such as 1600x512, got %r" % text)


def _loudness_arg(text):
    if text in LOUDNESS_MODES:
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected report, input or a target in LUFS such as -23, got %r" % text)


def _speech_level_arg(text):
    if text in SPEECH_LEVEL_MODES:
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected report, input or a target in dBov such as -26, got %r" % text)


def _crossover_hz_arg(text):
    if text == CROSSOVER_AUTO:
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError("expected a frequency in Hz or auto, got %r" % text)


def _bandwidth_args(a):
    """The bandwidth options of the command line -> the keyword arguments of enhance_file / enhance_folder ({} without
    --bandwidth); ValueError for a bad one."""
    opts = {k: v for k, v in (('threshold_db', a.bandwidth_threshold_db), ('n_fft', a.bandwidth_n_fft), ('band_bins', a.bandwidth_band_bins))
            if v is not None}
    if not a.bandwidth:
        if opts:
            raise ValueError("--bandwidth_%s is an option of --bandwidth" % sorted(opts)[0])
        return {}
    check_bandwidth(True, opts or None, a.loudness_scope, "generate")
    return dict(bandwidth=True, bandwidth_opts=opts or None)


def _stereo_args(a):
    """The stereo report options of the command line -> the keyword arguments of enhance_file / enhance_folder ({} without
    --stereo_report); ValueError for a bad one."""
    opts = {k: v for k, v in (('n_fft', a.stereo_n_fft), ('hop', a.stereo_hop)) if v is not None}
    if not a.stereo_report:
        if opts:
            raise ValueError("--stereo_%s is an option of --stereo_report" % sorted(opts)[0])
        return {}
    check_stereo_report(True, opts or None, a.loudness_scope, "generate")
    return dict(stereo_report=True, stereo_report_opts=opts or None)


def _loudness_args(a, hr_rate=None, folder_mode=False):
    """The loudness options of the command line -> the keyword arguments of enhance_file / enhance_folder ({} without --loudness);
    ValueError for a bad one.  `hr_rate`: None as long as the options file has not been read (the rate is then checked later).
    `folder_mode`: whether --input is a folder, which --loudness_scope folder needs."""
    if a.loudness is None:
        if a.loudness_scope != 'file':
            raise ValueError("--loudness_scope folder is an option of --loudness")
        if a.loudness_max_gain_db is not None:
            raise ValueError("--loudness_max_gain_db is an option of --loudness")
        if a.loudness_range:
            raise ValueError("--loudness_range is an option of --loudness")
        return {}
    loud = check_loudness(a.loudness, 48000 if hr_rate is None else hr_rate, "generate", a.loudness_max_gain_db, a.loudness_range)
    kw = dict(loudness=a.loudness, loudness_max_gain_db=a.loudness_max_gain_db)
    if a.loudness_range:
        kw['loudness_range'] = True
    if a.loudness_scope != 'file':
        check_loudness_scope(a.loudness_scope, loud, "generate", folder_mode, a.limiter, a.spectrogram)
        kw['loudness_scope'] = a.loudness_scope
    return kw


def _speech_level_args(a, rates=()):
    """The speech-level options of the command line -> the keyword arguments of enhance_file / enhance_folder ({} without
    --speech_level); ValueError for a bad one.  `rates`: the rates the clips are measured at, as far as they are known."""
    sl = check_speech_level(a.speech_level, "generate", a.speech_level_max_gain_db, a.loudness)
    if sl is None:
        return {}
    for rate in rates:
        check_speech_level_rate(rate, "generate")
    return dict(speech_level=a.speech_level, speech_level_max_gain_db=a.speech_level_max_gain_db)


def _spectrogram_args(a, folder_mode):
    """The spectrogram options of the command line -> the three keyword arguments of enhance_file / enhance_folder ({} without
    --spectrogram); ValueError for a bad one."""
    given = [n for n in ('channel', 'n_fft', 'hop', 'size', 'range_db', 'top_db') if getattr(a, 'spectrogram_' + n) is not None]
    if a.spectrogram is None:
        if given:
            raise ValueError("--spectrogram_%s is an option of --spectrogram PATH" % given[0])
        return {}
    if folder_mode and os.path.isfile(a.spectrogram):
        raise ValueError("--input is a directory, so --spectrogram must be a directory too, and %s is a file" % a.spectrogram)
    if not folder_mode and os.path.isdir(a.spectrogram):
        raise ValueError("--input is a file, so --spectrogram must be a file too, and %s is a directory" % a.spectrogram)
    opts = {k: v for k, v in (('n_fft', a.spectrogram_n_fft), ('hop', a.spectrogram_hop), ('range_db', a.spectrogram_range_db),
                              ('top_db', a.spectrogram_top_db)) if v is not None}
    if a.spectrogram_size is not None:
        opts['width'], opts['height'] = a.spectrogram_size
    channel = 0 if a.spectrogram_channel is None else a.spectrogram_channel
    check_spectrogram(channel=channel, who="generate", **opts)
    return dict(spectrogram=a.spectrogram, spectrogram_channel=channel, spectrogram_opts=opts or None)


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
    ap.add_argument("--crossover_hz", type=_crossover_hz_arg, default=None, metavar="F|auto",
                    help="--crossover input: the crossover frequency (default: 0.95 of the low rate's Nyquist frequency); auto: measure "
                         "where each input's band ends and keep of the input only that band -- the crossover at 0.95 of the band edge, "
                         "never above the default; one `crossover:` line more per file")
    ap.add_argument("--crossover_taps", type=int, default=None, metavar="N",
                    help="--crossover input: length of the filter, odd, <= 4095 (default: the shortest whose transition band ends "
                         "under the low rate's Nyquist frequency)")
    ap.add_argument("--clip", default="clamp", choices=CLIP_MODES,
                    help="samples beyond the range of --encoding: clamp them, silently (default); guard: scale the whole file down, "
                         "all channels alike, so that its peak sits at --ceiling_dbfs; error: write nothing and stop")
    ap.add_argument("--ceiling_dbfs", type=float, default=None, metavar="DB",
                    help="--clip guard: the level the peak is brought down to, <= 0 (default: the limit of --encoding)")
    ap.add_argument("--dither", default=None, choices=("tpdf", "shaped"),
                    help="pcm16 only: +-1 LSB of triangular noise in front of the rounding, so that the quantisation error of quiet "
                         "passages is noise and not distortion; shaped (files written at 44100 or 48000 Hz): the same noise in front "
                         "of an error-feedback quantiser that moves the 16-bit floor out of 2-5 kHz, where the ear hears best, and "
                         "up above 15 kHz; one `dither:` line more at the start")
    ap.add_argument("--dither_curve", default=None, choices=tuple(DITHER_CURVES),
                    help="--dither shaped: the noise-shaping curve (default lipshitz9, 9 taps; e5 and light3 shape less and add less "
                         "noise in total)")
    ap.add_argument("--dither_chunk", type=int, default=None, metavar="N",
                    help="--dither shaped: samples after which the quantiser's error history starts again at zero, a multiple of 64 in "
                         "256 .. 1048576 (default 4096); chunks run in parallel, longer ones shape a little deeper, one at least as "
                         "long as the file is the plain sequential recursion")
    ap.add_argument("--dither_seed", type=int, default=0, help="seed of --dither (file k of a folder uses seed + k)")
    ap.add_argument("--report_peaks", action="store_true",
                    help="print peak (dBFS), clipped and non-finite samples and the gain of every file; three more columns "
                         "(peak_dbfs, clipped, gain) of --metrics_csv")
    ap.add_argument("--spectrogram", default=None, metavar="PATH",
                    help="also write a PNG with the spectrograms of the input the generator was given, of the written clip and, for "
                         "a full-band input, of the original, top to bottom on one time, frequency and dB scale (a folder in folder "
                         "mode: one picture per file, at the file's relative path + .png; default: off)")
    ap.add_argument("--spectrogram_channel", type=int, default=None, metavar="N", help="--spectrogram: the written channel to show (default 0)")
    ap.add_argument("--spectrogram_n_fft", type=int, default=None, metavar="N",
                    help="--spectrogram: STFT length, a power of two in 64 .. 2048 (default 1024)")
    ap.add_argument("--spectrogram_hop", type=int, default=None, metavar="N", help="--spectrogram: STFT hop in samples (default 256)")
    ap.add_argument("--spectrogram_size", type=_size_arg, default=None, metavar="WxH",
                    help="--spectrogram: pixels of one panel (default 1600x512)")
    ap.add_argument("--spectrogram_range_db", type=float, default=None, metavar="DB",
                    help="--spectrogram: dB below the top that reach the palette's first colour (default 90)")
    ap.add_argument("--spectrogram_top_db", type=float, default=None, metavar="DB",
                    help="--spectrogram: level of the palette's last colour, 0 = a full-scale sine (default: the picture's own maximum)")
    ap.add_argument("--loudness", type=_loudness_arg, default=None, metavar="report|input|LUFS",
                    help="measure the integrated loudness (ITU-R BS.1770-4 / EBU R 128) of the input the generator was given and of "
                         "the generated clip, and print both per file (report); also scale the written clip to the input's loudness "
                         "(input) or to a target in LUFS, -70 .. 0, such as -23; three more columns (lufs_in, lufs_out, "
                         "loudness_gain_db) of --metrics_csv (default: off)")
    ap.add_argument("--speech_level", type=_speech_level_arg, default=None, metavar="report|input|DBOV",
                    help="measure the active speech level (ITU-T P.56 method B: the level while somebody is speaking, in dBov, and the "
                         "activity factor) of the input the generator was given and of the generated clip, and print both per file "
                         "(report); also bring the written clip to the input's active level (input) or to a level such as -26, with one "
                         "gain for all channels in front of the output stage; three more columns (asl_in, asl_out, activity_out) of "
                         "--metrics_csv; not with --loudness (default: off)")
    ap.add_argument("--speech_level_max_gain_db", type=float, default=None, metavar="DB",
                    help="--speech_level input|DBOV: the largest gain applied, either way, 0 .. 120 (default 40)")
    ap.add_argument("--loudness_max_gain_db", type=float, default=None, metavar="DB",
                    help="--loudness input|LUFS: the largest gain applied, either way (default 40)")
    ap.add_argument("--loudness_range", action="store_true",
                    help="--loudness: also measure the loudness range (EBU Tech 3342: 3 s blocks, the 10th to the 95th percentile behind "
                         "gates at -70 LUFS and 20 LU under the mean) of both clips and the maximum short-term loudness of the generated "
                         "one, as the loudness stage leaves it; one more line per file and three more columns (lra_in, lra_out, "
                         "short_term_max) of --metrics_csv (default: off)")
    ap.add_argument("--loudness_scope", default="file", choices=LOUDNESS_SCOPES,
                    help="--loudness with a folder as --input: file (default) measures and normalises every file on its own; folder "
                         "treats the folder as one programme, as EBU R 128 normalises an album -- one loudness over the blocks of all "
                         "files, one gain (and with --clip guard one guard gain) for all of them, so the level differences between the "
                         "files survive; one `album:` line more and one `album` row of --metrics_csv; not with --limiter, "
                         "--loudness_range or --spectrogram")
    ap.add_argument("--true_peak", action="store_true",
                    help="also measure the true peak (ITU-R BS.1770-4 Annex 2: the written clip oversampled to at least 192 kHz) and "
                         "print it in dBTP with the peak line of every file; --clip guard then brings the true peak, not the sample "
                         "peak, down to --ceiling_dbfs (read as dBTP) and --clip error also refuses a file whose true peak exceeds the "
                         "limit of --encoding; one more column (true_peak_dbtp) of --metrics_csv (default: off)")
    ap.add_argument("--limiter", action="store_true",
                    help="with --clip guard: a look-ahead true-peak limiter in front of the guard -- only the crests over --ceiling_dbfs "
                         "are turned down, by one gain curve for all channels, so the loudness --loudness reached stays where the guard "
                         "alone would scale the whole file down; measures the true peak as --true_peak does; one more line per file "
                         "and two more columns (limiter_reduction_db, limited_samples) of --metrics_csv (default: off)")
    ap.add_argument("--limiter_lookahead_ms", type=float, default=None, metavar="MS",
                    help="--limiter: how far the gain curve looks ahead of a crest, which is also its attack time (default 5)")
    ap.add_argument("--limiter_hold_ms", type=float, default=None, metavar="MS",
                    help="--limiter: how long the curve holds a reduction behind a crest (default 20)")
    ap.add_argument("--bandwidth", action="store_true",
                    help="report where the band of the input the generator was given, of the generated clip and, for a full-band input, "
                         "of the original actually ends: the highest bin of the long-term average spectrum within "
                         "--bandwidth_threshold_db of the strongest band; one more line per file, one per remark (an input that stops "
                         "short of the low rate's Nyquist frequency, an original with nothing above it) and three more columns (bw_in, "
                         "bw_out, bw_orig, in Hz) of --metrics_csv; not with --loudness_scope folder (default: off)")
    ap.add_argument("--bandwidth_threshold_db", type=float, default=None, metavar="DB",
                    help="--bandwidth: dB under the strongest band at which the band ends, in (0, 200] (default 60)")
    ap.add_argument("--bandwidth_n_fft", type=int, default=None, metavar="N",
                    help="--bandwidth: STFT length of the long-term average spectrum, a power of two in 64 .. 2048, hop N / 2 (default 2048)")
    ap.add_argument("--bandwidth_band_bins", type=int, default=None, metavar="N",
                    help="--bandwidth: bins per band whose mean level is compared with the threshold (default 8)")
    ap.add_argument("--stereo", default="lr", choices=("lr", "ms"),
                    help="how a two-channel file is generated: lr -- left and right each a clip of its own, so the band above the low "
                         "rate's Nyquist frequency is invented twice; ms -- mid and side: what the channels share is invented once, only "
                         "their difference on its own (one channel runs as with lr; more than two are refused) (default: lr)")
    ap.add_argument("--norm_scope", default="group", choices=("group", "clip"),
                    help="what the dB spectrogram is normalised by: group -- the minimum and maximum of each group of --batchSize "
                         "segments, the reference's chain: the output depends on the batch size, and a group of digital silence is "
                         "written as NaN; clip -- one range per channel of a file, found on the device in a pass in front of its first "
                         "group: the same file at every batch size, silence stays silence; one start-up line more (default: group)")
    ap.add_argument("--segment_norm", action="store_true",
                    help="normalise every segment by its own range, what --norm_scope group means at --batchSize 1, at any batch size: "
                         "the same file at every batch size, a silent segment stays silent, no pass in front of the first group; all "
                         "channels of a file share groups and the last group is filled up with silent segments, so every group "
                         "replays the one captured graph; one start-up line more; not with --norm_scope clip (default: off)")
    ap.add_argument("--pack_files", type=int, default=1, metavar="N",
                    help="a folder as --input, with --segment_norm: up to N consecutive files share the generator's groups -- their "
                         "segments are gathered and stitched in one launch each and walked as one clip's, so a folder of short "
                         "utterances runs full groups where file by file each one's last group is filled up with silent segments; "
                         "a file's own segments, ranges and (with a seed) mask noise stay those of N = 1; one start-up line more; not "
                         "with --loudness_scope folder (default: 1, every file on its own)")
    ap.add_argument("--stream_seconds", type=float, default=None, metavar="W",
                    help="with --segment_norm: send every file through in windows of about W seconds -- whole segments, whole groups -- "
                         "each read, generated, encoded and appended to the output while the next is read, so that memory is a "
                         "window's whatever the file's length; the written file is the same where the model draws no mask noise, "
                         "which is otherwise drawn in window order; PCM, float and G.711 inputs (not FLAC, not IMA ADPCM); not with "
                         "the crossover, --container flac, --dither shaped, --pack_files, --output_rate, --metrics_ext or any option "
                         "that measures the whole file; one start-up line more (default: off, a file is one unit)")
    ap.add_argument("--stereo_report", action="store_true",
                    help="report how the left and right channel of a file written with two channels correlate below and above the low "
                         "rate's Nyquist frequency -- for the input the generator was given, the generated clip and, for a full-band "
                         "input, the original; one more line per such file, one per remark, and four more columns (corr_lf_out, "
                         "corr_hf_out, corr_hf_orig, side_hf_out_db) of --metrics_csv; not with --loudness_scope folder (default: off)")
    ap.add_argument("--stereo_n_fft", type=int, default=None, metavar="N",
                    help="--stereo_report: STFT length of the cross-spectrum, a power of two in 64 .. 2048 (default 2048)")
    ap.add_argument("--stereo_hop", type=int, default=None, metavar="N",
                    help="--stereo_report: hop of the cross-spectrum, 1 .. N of --stereo_n_fft (default: half of it)")
    ap.add_argument("--output_rate", type=int, default=None, metavar="HZ",
                    help="write the file at this rate instead of the checkpoint's hr_sampling_rate, 44100 for instance: a polyphase rate "
                         "converter (flat to 0.907 of the lower Nyquist frequency, 120 dB down where anything folds) in front of the "
                         "loudness, true-peak and limiter stages, which then measure and hold what is written; one start-up line more; "
                         "not with --spectrogram or --loudness_scope folder (default: off)")
    ap.add_argument("--input_formats", default=None, metavar="LIST",
                    help="a folder as --input: the extensions to list, of wav, flac, aif, aiff, aifc, au, snd and sph, with commas (default: wav); "
                         "x.flac or x.aif is written as x.wav; a single --input file is read by what its first bytes say, whatever its name")
    ap.add_argument("--verify_input", action="store_true",
                    help="FLAC inputs: decode the file on the host first and refuse it where its samples do not have the MD5 its "
                         "STREAMINFO states; one start-up line more (default: off)")
    ap.add_argument("--container", default="wav", choices=("wav", "flac"),
                    help="what is written: wav, or a FLAC stream that decodes to the wav's data chunk byte for byte, encoded on the "
                         "device (fixed predictors, Rice partitions, stereo decorrelation); pcm16 or pcm24 only; a folder's outputs "
                         "are then named .flac; one line more per file (default: wav)")
    ap.add_argument("--flac_block", type=int, default=None, metavar="N",
                    help="--container flac: samples per FLAC frame, 16 .. 65535 (default 4096)")
    ap.add_argument("--flac_md5", action="store_true",
                    help="--container flac: write the MD5 of the samples into STREAMINFO; the payload is then copied back beside the "
                         "stream, a second copy of the payload's size (default: off, the MD5 field is zeros)")
    ap.add_argument("--flac_lpc", type=int, default=None, metavar="N",
                    help="--container flac: also try LPC subframes of every order 1 .. N, N in 0 .. 12 (a predictor fitted per block; "
                         "--flac_block at most 16384); the file is never longer than without (default: off)")
    ap.add_argument("--fp16", action="store_true", help="16-bit activation storage")
    ap.add_argument("--mdct_type", default=None, choices=("mdct2", "mdct4"),
                    help="transform of the checkpoint (default: the options file's, else $P2PHD_MDCT_TYPE, else mdct2 -- "
                         "the one the reference's train.py, which writes opt.txt, is hard-wired to)")
    return ap


def _print_flac(path, f, encoding):
    print('%s: FLAC %d bit, %d frames of %d, %d bytes (%.1f %% of the PCM)%s%s'
          % (path, 24 if encoding == 'pcm24' else 16, f['frames'], f['block'], f['bytes'], 100.0 * f['bytes'] / f['pcm_bytes'],
             '' if f['md5'] is None else ', MD5 ' + f['md5'], ', LPC up to order %d' % f['lpc'] if f.get('lpc') else ''))


def _print_spectrogram(p):
    print('spectrogram: %s (%d panels, %d frames x %d bins, %.1f dB down from %+.1f dB)'
          % (p['path'], p['panels'], p['frames'], p['bins'], p['range_db'], p['top_db']))


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    try:                                                                    # before anything is loaded
        folder_mode = check_paths(a.input, a.output)
        check_segment_norm(a.segment_norm, a.norm_scope, "generate")
        if check_pack_files(a.pack_files, a.segment_norm, a.loudness_scope, "generate") > 1 and not folder_mode:
            raise ValueError("--pack_files is an option of a folder as --input")
        out_stage = check_output_options(a.encoding, a.clip, a.ceiling_dbfs, a.dither, a.dither_seed, a.report_peaks, "generate", a.dither_curve,
                                         a.dither_chunk)
        if a.output_rate is not None:                                       # (the model's rate: once the options file has been read)
            check_dither(a.dither, a.encoding, "generate", a.output_rate, a.dither_curve, a.dither_chunk)
        picture = _spectrogram_args(a, folder_mode)
        picture.update(_loudness_args(a, None, folder_mode))
        picture.update(_bandwidth_args(a))
        picture.update(_stereo_args(a))
        picture.update(_speech_level_args(a, () if a.output_rate is None else (a.output_rate,)))
        if a.true_peak:
            picture['true_peak'] = True
        if a.output_rate is not None:                                       # (the rate pair itself: once the options file has been read)
            check_output_rate(a.output_rate, a.output_rate, "generate")
            picture['output_rate'] = a.output_rate
        if a.input_formats is not None:
            if not folder_mode:
                raise ValueError("--input_formats is an option of a folder as --input")
            picture['input_formats'] = check_input_formats(a.input_formats, "generate")
        if a.verify_input:
            picture['verify_input'] = True
        if a.pack_files > 1:
            picture['pack_files'] = a.pack_files
        if check_stream(a.stream_seconds, "generate", a.segment_norm, a.crossover, None, loudness=a.loudness, speech_level=a.speech_level, clip=a.clip,
                        true_peak=a.true_peak, limiter=a.limiter, report_peaks=a.report_peaks, spectrogram=a.spectrogram, bandwidth=a.bandwidth,
                        stereo_report=a.stereo_report, output_rate=a.output_rate, extended_metrics=a.metrics_ext, container=a.container,
                        dither=a.dither, pack_files=a.pack_files, loudness_scope=a.loudness_scope) is not None:
            picture['stream_seconds'] = a.stream_seconds
        if check_container(a.container, a.flac_block, a.flac_md5, a.encoding, a.output_rate or 48000, "generate",
                           **({} if a.flac_lpc is None else dict(flac_lpc=a.flac_lpc))) is not None:
            picture.update(container=a.container, **{k: v for k, v in (('flac_block', a.flac_block), ('flac_md5', a.flac_md5 or None), ('flac_lpc', a.flac_lpc))
                                                     if v is not None})
        if a.limiter or a.limiter_lookahead_ms is not None or a.limiter_hold_ms is not None:
            check_limiter(a.limiter, a.limiter_lookahead_ms, a.limiter_hold_ms, out_stage, a.encoding, 48000, "generate")
            picture.update(limiter=True, limiter_lookahead_ms=a.limiter_lookahead_ms, limiter_hold_ms=a.limiter_hold_ms)
    except ValueError as e:
        ap.error(str(e))
    stage = dict(clip=a.clip, ceiling_dbfs=a.ceiling_dbfs, dither=a.dither, dither_seed=a.dither_seed, report_peaks=a.report_peaks, **picture)
    if a.dither == 'shaped':
        stage.update(dither_curve=a.dither_curve, dither_chunk=a.dither_chunk)
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
        check_lowband(a.lowband, a.lowband_fade, spectro_bins(opt.n_fft, opt.mdct_type), opt.hr_sampling_rate / opt.lr_sampling_rate)
        check_crossover(a.crossover, a.crossover_hz, a.crossover_taps, opt.hr_sampling_rate, opt.lr_sampling_rate)
        _loudness_args(a, opt.hr_sampling_rate, folder_mode)
        rc = check_output_rate(a.output_rate, opt.hr_sampling_rate, "generate", a.loudness_scope, a.spectrogram)
        if rc is not None and a.loudness is not None:
            _loudness_args(a, rc['rate'], folder_mode)
        _speech_level_args(a, (opt.hr_sampling_rate,) if rc is None else (opt.hr_sampling_rate, rc['rate']))
        check_dither(a.dither, a.encoding, "generate", opt.hr_sampling_rate if rc is None else rc['rate'], a.dither_curve, a.dither_chunk)
        if a.limiter:
            check_limiter(True, a.limiter_lookahead_ms, a.limiter_hold_ms, out_stage, a.encoding, opt.hr_sampling_rate if rc is None else rc['rate'],
                          "generate")
    except ValueError as e:
        ap.error(str(e))
    from ..models.models import create_model
    model = create_model(opt)
    model.eval()
    seed = getattr(opt, 'seed', None)
    if seed is not None:
        torch.manual_seed(int(seed))                                        # the mask noise: one run, one result
    sr = SuperResolver(model, opt, overlap=a.overlap, graph=not a.no_graph,
                       reference_amplitude=None if a.reference_amplitude is None else bool(a.reference_amplitude),
                       lowband=a.lowband, lowband_fade=a.lowband_fade, crossover=a.crossover, crossover_hz=a.crossover_hz,
                       crossover_taps=a.crossover_taps, **({} if a.stereo == 'lr' else {'stereo': a.stereo}),
                       **({} if a.norm_scope == 'group' else {'norm_scope': a.norm_scope}),
                       **({'segment_norm': True} if a.segment_norm else {}))
    print('amplitude: %s; low band: %s' % ("the reference's (half of sqrt(up_ratio - 1) * x)" if sr.reference_amplitude else 'full',
                                           "the model's" if sr.lowband == 'model' else
                                           "the input's (fade over %d rows)" % sr.lowband_fade))
    if sr.crossover_auto:
        print("crossover: the input below 0.95 of where its own band ends, at most %g Hz (auto)" % (sr.crossover_plan[1] * opt.hr_sampling_rate))
    elif sr.crossover_plan is not None:                                     # (without the option: no line more than before)
        print('crossover: the input below %g Hz (%d taps)' % (sr.crossover_plan[1] * opt.hr_sampling_rate, sr.crossover_plan[0]))
    if sr.stereo == 'ms':                                                   # (without the option: no line more than before)
        print('stereo: mid / side')
    if sr.norm_scope == 'clip':                                             # (without the option: no line more than before)
        print('normalisation: one range per clip')
    if sr.segment_norm:                                                     # (without the option: no line more than before)
        print('normalisation: one range per segment')
    if a.pack_files > 1:                                                    # (without the option: no line more than before)
        print('packing: up to %d files share groups' % a.pack_files)
    if a.stream_seconds is not None:                                        # (without the option: no line more than before)
        print(_stream_line(a, sr, folder_mode))
    if rc is not None:                                                      # (without the option: no line more than before)
        print(output_rate_line(rc))
    if a.dither == 'shaped':                                                # (without the option: no line more than before)
        print(dither_line(out_stage, shaper_coefficients(out_stage['curve']).numel()))
    if a.verify_input:                                                      # (without the option: no line more than before)
        print("input: every FLAC file's MD5 is checked on the host before it is read")
    rate = int(opt.hr_sampling_rate) if rc is None else rc['rate']
    try:
        return _run(a, sr, stage, seed, rate, folder_mode)
    except ClipError as e:
        print('error: %s' % e, file=sys.stderr)                             # --clip error: the file that would clip
        return 1


def _stream_line(a, sr, folder_mode):
    """--stream_seconds: the start-up line.  The segments per window follow from the written channel count (plans.stream_plan): a
    single input's own, read from its header; a folder's files are counted as one channel each here and planned one by one."""
    channels = 1
    if not folder_mode:
        try:
            from ..data import audiofile
            channels = select_channels(a.channels, audiofile.info(a.input).num_channels)
        except (ValueError, OSError, EOFError):                             # (enhance_file says what is wrong with it)
            pass
    plan = stream_plan(0, sr.opt.hr_sampling_rate, sr.opt.lr_sampling_rate, sr.opt.hr_sampling_rate, True, sr.T, sr.overlap, channels, sr.batch,
                       a.stream_seconds)
    return 'streaming: windows of %d segments (%g s)' % (plan['K'], plan['K'] * plan['stride'] / float(sr.opt.hr_sampling_rate))


def _print_report(a, name, wrote, r):
    """The lines of one enhanced file behind its `wrote` line, an option's only where the option is on (without it: no line more
    than before).  `r`: a folder record, or enhance_file's result in that shape; `name`: what the lines call the file; `wrote`: the
    path that was written."""
    if r.get('flac') is not None:
        _print_flac(wrote, r['flac'], a.encoding)
    if a.report_peaks or a.true_peak or a.limiter:
        _print_peaks(name, r['output'])
    if a.limiter:
        _print_limiter(r['output']['limiter'], r['out_frames'])
    if r.get('spectrogram') is not None:
        _print_spectrogram(r['spectrogram'])
    if r.get('loudness') is not None:
        _print_loudness(name, r['loudness'])
        if 'range' in r['loudness']:
            _print_loudness_range(name, r['loudness']['range'])
    if r.get('speech_level') is not None:
        _print_speech_level(name, r['speech_level'])
    if r.get('crossover') is not None:
        _print_crossover(r['crossover'])
    if r.get('bandwidth') is not None:
        _print_bandwidth(name, r['bandwidth'])
    if r.get('stereo') is not None:
        _print_stereo(name, r['stereo'])


# --metrics_csv: the argument that brings columns -> write_metrics_csv's flag for them (on: neither None, False nor scope 'file')
_CSV_FLAGS = {'loudness': 'loudness', 'true_peak': 'true_peak', 'limiter': 'limiter', 'loudness_range': 'loudness_range', 'loudness_scope': 'album',
              'bandwidth': 'bandwidth', 'stereo_report': 'stereo', 'speech_level': 'speech_level'}


def _run(a, sr, stage, seed, rate, folder_mode):
    if folder_mode:
        def report(r):
            if r['error'] is not None:
                print('skipped %s: %s' % (r['path'], r['error']))
                return
            _print_unwritten(r['path'], r['channels'], r['written_channels'])
            wrote = os.path.join(a.output, r.get('written', r['path']))
            print('wrote %s (%d samples at %d Hz, %d channel%s)' % (wrote, r['out_frames'], rate, r['written_channels'],
                                                                   '' if r['written_channels'] == 1 else 's'))
            _print_report(a, r['path'], wrote, r)
        # every file starts from the seed, so it comes out as a run of its own would write it
        records = sr.enhance_folder(a.input, a.output, a.is_lr_input, a.channels, a.encoding, seed=seed, report=report,
                                    extended_metrics=a.metrics_ext, **stage)
        done = [r for r in records if r['error'] is None]
        if a.loudness_scope == 'folder' and done:                          # (without the option: no line more than before)
            _print_album(done[0]['album'])
        print('%d of %d files enhanced, %d skipped' % (len(done), len(records), len(records) - len(done)))
        rows = metrics_rows(records, a.metrics_ext)                       # (the printed means: no peak columns)
        if rows:
            print('mean over %d channels: MSE %.4f  SNR_SR %.4f  SNR_LR %.4f  LSD %.4f' % ((len(rows) - 1,) + rows[-1][3:7]))
            if a.metrics_ext:
                print('mean over %d channels: LSD_LF %.4f  LSD_HF %.4f  SSNR_SR %.4f  SSNR_LR %.4f' % ((len(rows) - 1,) + rows[-1][7:]))
    else:
        res = sr.enhance_file(a.input, a.output, a.is_lr_input, a.channels, a.encoding, extended_metrics=a.metrics_ext, **stage)
        streamed = res.get('stream')                                        # (--stream_seconds: no clip comes back)
        out_frames = res['sr'].shape[-1] if streamed is None else streamed['out_frames']
        m, written = per_channel_metrics(res['metrics'], a.channels), (res['sr'] if streamed is None else res['norm']).shape[0]
        ext = res.get('metrics_ext')
        _print_unwritten(a.input, res['info'].num_channels, written)
        for c, mc in enumerate(m or ()):
            prefix = '' if a.channels == 'first' else 'channel %d ' % c
            _print_metrics(mc, prefix)
            if ext is not None:
                _print_metrics_ext(ext[c], prefix)
        if written == 1:
            print('wrote %s (%d samples at %d Hz)' % (a.output, out_frames, rate))
        else:
            print('wrote %s (%d samples at %d Hz, %d channels)' % (a.output, out_frames, rate, written))
        # the result in a record's shape: every option's key as enhance_file returned it, a record's own five beside them
        records = [dict(res, path=os.path.basename(a.input), out_frames=out_frames, metrics=m, metrics_ext=ext, output=res.get('output'),
                        loudness=res.get('loudness'))]
        _print_report(a, a.output, a.output, records[0])
    if a.metrics_csv:
        on = lambda v: v is not None and v is not False and v != 'file'     # noqa: E731
        write_metrics_csv(a.metrics_csv, records, a.metrics_ext, a.report_peaks, **{flag: True for arg, flag in _CSV_FLAGS.items() if on(getattr(a, arg))})
        print('metrics: %s' % a.metrics_csv)
    return 0
