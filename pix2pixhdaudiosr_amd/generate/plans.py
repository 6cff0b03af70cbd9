"""Whole-file generation: the host arithmetic and the validation of every option -- no tensor, no library (check_output_rate alone
asks the library, for the converter's plan: the host entry point that can refuse it is the one that knows why)."""
import math
import os
from fractions import Fraction

# encoding of wavio.save / wavio.write_payload -> (P2PHD_PCM_* code of include/p2phd.h, bytes per sample)
PCM_ENCODINGS = {'pcm16': (1, 2), 'pcm24': (2, 3), 'float32': (4, 4)}
DITHERS = (None, 'tpdf', 'shaped')
# the noise-shaped dither (csrc/shaper.hip): curve name -> curve id of p2phd_shaper_taps_fill (the first is the default); samples of a
# chunk where none is given -- the error history starts at zero in every chunk, which is what makes the recursion parallel, and a
# multiple of 64 in [DITHER_MIN_CHUNK, DITHER_MAX_CHUNK]; the written rates the curves are for
DITHER_CURVES = {'lipshitz9': 0, 'e5': 1, 'light3': 2}
DITHER_CHUNK = 4096
DITHER_MIN_CHUNK, DITHER_MAX_CHUNK = 256, 1 << 20
SHAPED_RATES = (44100, 48000)
CLIP_MODES = ('clamp', 'guard', 'error')
LOWBANDS = ('model', 'input')
CROSSOVERS = (None, 'input')
CROSSOVER_BETA = 8.96                                                       # Kaiser window, 90 dB
CROSSOVER_ATTEN_DB = 90.0
CROSSOVER_MAX_TAPS = 4095
CROSSOVER_AUTO = 'auto'                                                     # crossover_hz: follow the band each input has
# the bandwidth report (csrc/bandwidth.hip): STFT length and hop of the long-term average spectrum, bins of a band, dB under the
# strongest band at which the band ends
BANDWIDTH_DEFAULTS = {'n_fft': 2048, 'hop': 1024, 'band_bins': 8, 'threshold_db': 60.0}
# the stereo image report and the mid/side mode (csrc/stereo.hip): how a two-channel clip is generated -- 'lr': every channel a clip of
# its own; 'ms': mid and side, so that what the channels share is invented once --, STFT length and hop of the cross-spectrum, and
# how far the generated clip's correlation above the split may fall under the one below it before the report remarks on it (a
# reporting threshold like the bandwidth notes' 0.9 / 1.05, not a measurement)
STEREO_MODES = ('lr', 'ms')
# what the dB spectrogram is normalised by (csrc/spectro.hip): 'group' -- the minimum and maximum of each group of batchSize
# segments, the reference's chain; 'clip' -- one range per clip, over all of its segments
NORM_SCOPES = ('group', 'clip')
STEREO_DEFAULTS = {'n_fft': 2048, 'hop': 1024}
STEREO_NOTE_DROP = 0.3
# the spectrogram picture (csrc/specimg.hip): STFT length and hop in samples, pixels of one panel, dB below the top that
# reach the palette's first colour, grey rows between panels
SPECTROGRAM_DEFAULTS = {'n_fft': 1024, 'hop': 256, 'width': 1600, 'height': 512, 'range_db': 90.0, 'gap': 2}
SPECTROGRAM_MAX_SIDE = 16384
SPECTROGRAM_MAX_GAP = 64
# the loudness option (csrc/loudness.hip): the largest gain, either way, that normalisation applies; the modes beside a target in LUFS;
# the rates the K-weighting entry takes (a hop is rate / 10 samples); channels the gate takes
LOUDNESS_MAX_GAIN_DB = 40.0
LOUDNESS_MODES = ('report', 'input')
LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE = 8000, 384000
LOUDNESS_MAX_CHANNELS = 64
# what one loudness gain is found for: every file on its own, or the folder as one programme (EBU R 128 album loudness); the bytes of
# generated clips the folder pipeline keeps on the device between measuring and writing, beyond which a clip waits on the host
LOUDNESS_SCOPES = ('file', 'folder')
ALBUM_CACHE_BYTES = 4 << 30
# the speech-level option (csrc/speechlevel.hip; ITU-T P.56 method B): the largest gain either way where none is given, the modes, the
# rates the envelope's constants are filled for and the channels the decision takes in the file pipeline
SPEECH_LEVEL_DEFAULTS = {'max_gain_db': 40.0}
SPEECH_LEVEL_MODES = ('report', 'input')
SPEECH_LEVEL_MIN_RATE, SPEECH_LEVEL_MAX_RATE = 8000, 192000
SPEECH_LEVEL_MAX_CHANNELS = 8
SPEECH_LEVEL_KERNEL_CHANNELS = 64
# the true-peak option (csrc/truepeak.hip): taps per phase and Kaiser beta of the interpolator; the oversampled rate it reaches
TRUEPEAK_TAPS_PER_PHASE = 24
TRUEPEAK_BETA = 9.0
TRUEPEAK_MIN_OVERSAMPLED_RATE = 192000
# the limiter option (csrc/limiter.hip): look-ahead and hold in ms where none is given -- a judgement about audibility (a short
# hold lets the gain ride the crests of low tones), not a measured optimum -- and the kernel's caps in samples
LIMITER_LOOKAHEAD_MS = 5.0
LIMITER_HOLD_MS = 20.0
LIMITER_MAX_LOOKAHEAD = 1024
LIMITER_MAX_HOLD = 4096
# the output-rate option (csrc/rateconv.hip): the converter's flat passband as a fraction of the lower rate's Nyquist frequency (0.907:
# 20 kHz at 44.1 kHz) and its stopband attenuation in dB; the lowest rate that is written
RATECONV_DEFAULTS = {'passband': 0.907, 'atten_db': 120.0}
OUTPUT_MIN_RATE = 8000
# (index, (r, g, b)) anchors of spectrogram_lut
SPECTROGRAM_LUT_ANCHORS = ((0, (0, 0, 4)), (64, (30, 20, 140)), (128, (180, 40, 150)), (192, (250, 140, 30)), (255, (255, 250, 190)))


class ClipError(ValueError):
    """clip='error': the file would clip; nothing was written."""


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


def check_encoding(encoding, who):
    """-> (P2PHD_PCM_* code, bytes per sample) of an output encoding."""
    if encoding not in PCM_ENCODINGS:
        raise ValueError("%s: encoding must be one of %s, got %r" % (who, sorted(PCM_ENCODINGS), encoding))
    return PCM_ENCODINGS[encoding]


def check_dither(dither, encoding, who, rate=None, curve=None, chunk=None):
    """Validates the dither option.  `curve` (a name of DITHER_CURVES) and `chunk` are options of dither='shaped'; `rate`: None, or
    the rate the file is written at, which 'shaped' takes only from SHAPED_RATES (the curves are published for 44.1 kHz)."""
    if dither not in DITHERS:
        raise ValueError("%s: dither must be None, 'tpdf' or 'shaped', got %r" % (who, dither))
    if dither is not None and encoding != 'pcm16':
        raise ValueError("%s: dither is for pcm16 (a 24-bit or float32 file carries the signal's own low bits), got encoding %r"
                         % (who, encoding))
    if dither != 'shaped':
        if curve is not None or chunk is not None:
            raise ValueError("%s: dither_curve / dither_chunk are options of dither='shaped'; dither is %r" % (who, dither))
        return
    if curve is not None and curve not in DITHER_CURVES:
        raise ValueError("%s: dither_curve must be one of %s, got %r" % (who, sorted(DITHER_CURVES), curve))
    if chunk is not None and (not _is_int(chunk) or not DITHER_MIN_CHUNK <= chunk <= DITHER_MAX_CHUNK or chunk % 64):
        raise ValueError("%s: dither_chunk must be a multiple of 64 in [%d, %d], got %r" % (who, DITHER_MIN_CHUNK, DITHER_MAX_CHUNK, chunk))
    if rate is not None and rate not in SHAPED_RATES:
        raise ValueError("%s: dither='shaped' is for files written at %s Hz (its curves are published for 44.1 kHz), got %r Hz"
                         % (who, ' or '.join(str(r) for r in SHAPED_RATES), rate))


def dither_line(stage, taps):
    """The start-up line of dither='shaped'; `taps`: how many the curve has."""
    return 'dither: shaped (%s, %d taps, chunks of %d)' % (stage['curve'], taps, stage['chunk'])


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


def check_output_options(encoding, clip='clamp', ceiling_dbfs=None, dither=None, dither_seed=0, report_peaks=False, who="enhance_file",
                         dither_curve=None, dither_chunk=None):
    """Validates the output-stage options; -> None when all of them are at their defaults (the encoder runs without gain
    and dither and nothing is reported), else a dict {'clip', 'ceiling' (linear, or None), 'dither', 'seed', 'report'}; with
    dither 'shaped' the dict also carries 'curve' and 'chunk' (`dither_curve`, `dither_chunk`, or the defaults)."""
    check_encoding(encoding, who)
    if clip not in CLIP_MODES:
        raise ValueError("%s: clip must be one of %s, got %r" % (who, CLIP_MODES, clip))
    check_dither(dither, encoding, who, None, dither_curve, dither_chunk)
    if ceiling_dbfs is not None:
        if isinstance(ceiling_dbfs, bool) or not isinstance(ceiling_dbfs, (int, float)) or not -1000.0 <= ceiling_dbfs <= 0.0:
            raise ValueError("%s: ceiling_dbfs must be a level <= 0 dBFS, got %r" % (who, ceiling_dbfs))
        if clip != 'guard':
            raise ValueError("%s: ceiling_dbfs is the level clip='guard' scales to; clip is %r" % (who, clip))
    if isinstance(dither_seed, bool) or not isinstance(dither_seed, int):
        raise ValueError("%s: dither_seed must be an int, got %r" % (who, dither_seed))
    if clip == 'clamp' and ceiling_dbfs is None and dither is None and dither_seed == 0 and not report_peaks:
        return None
    stage = {'clip': clip, 'ceiling': ceiling_from_dbfs(ceiling_dbfs, encoding), 'dither': dither, 'seed': dither_seed,
             'report': bool(report_peaks)}
    if dither == 'shaped':
        stage.update(curve=next(iter(DITHER_CURVES)) if dither_curve is None else dither_curve,
                     chunk=DITHER_CHUNK if dither_chunk is None else dither_chunk)
    return stage


def spectro_bins(n_fft, mdct_type):
    """Rows of the spectrogram: MDCT2 keeps n_fft of them, MDCT4 half."""
    return int(n_fft) if mdct_type == 'mdct2' else int(n_fft) // 2


def check_lowband(lowband, lowband_fade, bins, up_ratio):
    """Validates the low-band options of SuperResolver for a spectrogram of `bins` rows: `lowband` is 'model' or 'input' and
    `lowband_fade` a whole number of rows in [0, keep], keep = int(bins / up_ratio) -- the rows the low-rate input carried
    (all of them at up_ratio <= 1).  Returns (lowband, lowband_fade, keep)."""
    from ..util.util import check_lowband_fade, lowband_keep_rows
    if lowband not in LOWBANDS:
        raise ValueError("SuperResolver: lowband must be 'model' or 'input', got %r" % (lowband,))
    keep = lowband_keep_rows(bins, up_ratio)
    return lowband, check_lowband_fade(lowband_fade, keep, "SuperResolver"), keep


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


def check_crossover(crossover, crossover_hz, crossover_taps, hr_rate, lr_rate):
    """Validates the crossover options of SuperResolver -> None (off), or crossover_plan's (taps, cutoff, beta).  crossover_hz
    'auto' (the crossover follows each clip's own band, crossover_auto_plan): the plan of an input that reaches the low rate's
    Nyquist frequency, which is the default one."""
    if crossover not in CROSSOVERS:
        raise ValueError("SuperResolver: crossover must be None or 'input', got %r" % (crossover,))
    if crossover is None:
        if crossover_hz is not None or crossover_taps is not None:
            raise ValueError("SuperResolver: crossover_hz / crossover_taps are options of crossover='input'; crossover is None")
        return None
    if isinstance(crossover_hz, str):
        if crossover_hz != CROSSOVER_AUTO:
            raise ValueError("SuperResolver: crossover_hz must be None, a frequency in Hz or 'auto', got %r" % (crossover_hz,))
        return crossover_auto_plan(hr_rate, lr_rate, float(lr_rate) / 2.0, crossover_taps)[0]
    return crossover_plan(hr_rate, lr_rate, crossover_hz, crossover_taps)


def crossover_auto_floor_hz(hr_rate, taps=None):
    """The lowest band edge crossover_auto_plan serves at `hr_rate`: with the crossover at 0.95 of the edge the transition band has
    0.05 of the edge on its upper side, which must hold half the width of the longest filter (`taps`, None: CROSSOVER_MAX_TAPS) --
    10 crossover_width_hz, a few parts in 10^9 more so that the plan's own `fits` test agrees in floating point."""
    return 10.0 * crossover_width_hz(float(hr_rate), CROSSOVER_MAX_TAPS if taps is None else taps) * (1.0 + 1e-9)


def crossover_auto_plan(hr_rate, lr_rate, edge_hz, taps=None):
    """The crossover of crossover_hz='auto' for an input whose band ends at `edge_hz`, host arithmetic only -> ((taps, cutoff,
    beta), edge): edge = `edge_hz` held inside [crossover_auto_floor_hz, the low rate's Nyquist frequency], and the filter is
    crossover_plan(hr_rate, 2 * edge, None, taps) -- the plan of a low rate whose Nyquist frequency is the edge: the crossover at
    0.95 of the edge, the transition band ending at the edge.  An input that reaches the low rate's Nyquist frequency gets
    crossover_plan's default tuple, exactly."""
    hr_rate, lr_rate = float(hr_rate), float(lr_rate)
    if not 0.0 < lr_rate < hr_rate:
        raise ValueError("crossover_plan: nothing to cross over: the low rate %g must be above 0 and below the high rate %g" % (lr_rate, hr_rate))
    edge = float(edge_hz)
    if not edge == edge:
        raise ValueError("crossover_auto_plan: the band edge must be a number, got %r" % (edge_hz,))
    nyquist = lr_rate / 2.0
    edge = min(nyquist, max(edge, min(nyquist, crossover_auto_floor_hz(hr_rate, taps))))
    return crossover_plan(hr_rate, 2.0 * edge, None, taps), edge


def check_bandwidth(bandwidth=False, opts=None, loudness_scope='file', who="enhance_file"):
    """Validates the bandwidth option -> None (off), or the plan {'n_fft', 'hop', 'band_bins', 'threshold_db'} that ops.bandwidth
    takes.  `bandwidth`: a bool.  `opts`: None or a dict of those four, None or absent standing for BANDWIDTH_DEFAULTS' value (hop:
    half of a given n_fft): `n_fft` a power of two in [64, 2048]; `hop` 1 .. n_fft; `band_bins` 1 .. n_fft / 2 + 1; `threshold_db`
    in (0, 200].  They are options of the option.  The report is one file's: with loudness_scope 'folder' it is a ValueError, as
    the spectrogram is.  A ValueError names the argument."""
    if not isinstance(bandwidth, bool):
        raise ValueError("%s: bandwidth must be a bool, got %r" % (who, bandwidth))
    if opts is not None and not isinstance(opts, dict):
        raise ValueError("%s: bandwidth_opts must be None or a dict, got %r" % (who, opts))
    if not bandwidth:
        if opts is not None:
            raise ValueError("%s: bandwidth_opts are options of bandwidth=True; bandwidth is False" % who)
        return None
    if loudness_scope == 'folder':
        raise ValueError("%s: bandwidth is not built for loudness_scope='folder': the report is measured per file" % who)
    opts = {k: v for k, v in (opts or {}).items() if v is not None}
    unknown = sorted(set(opts) - set(BANDWIDTH_DEFAULTS))
    if unknown:
        raise ValueError("%s: unknown bandwidth_opts %s" % (who, unknown))
    d = BANDWIDTH_DEFAULTS
    n_fft = opts.get('n_fft', d['n_fft'])
    if not _is_int(n_fft) or not 64 <= n_fft <= 2048 or n_fft & (n_fft - 1):
        raise ValueError("%s: bandwidth n_fft must be a power of two in [64, 2048], got %r" % (who, n_fft))
    hop = opts.get('hop', d['hop'] if 'n_fft' not in opts else n_fft // 2)
    if not _is_int(hop) or not 1 <= hop <= n_fft:
        raise ValueError("%s: bandwidth hop must be an int in [1, n_fft = %d], got %r" % (who, n_fft, hop))
    band_bins = opts.get('band_bins', d['band_bins'])
    if not _is_int(band_bins) or not 1 <= band_bins <= n_fft // 2 + 1:
        raise ValueError("%s: bandwidth band_bins must be an int in [1, n_fft / 2 + 1 = %d], got %r" % (who, n_fft // 2 + 1, band_bins))
    threshold_db = opts.get('threshold_db', d['threshold_db'])
    if isinstance(threshold_db, bool) or not isinstance(threshold_db, (int, float)) or not 0.0 < threshold_db <= 200.0:
        raise ValueError("%s: bandwidth threshold_db must lie in (0, 200] dB, got %r" % (who, threshold_db))
    return {'n_fft': n_fft, 'hop': hop, 'band_bins': band_bins, 'threshold_db': float(threshold_db)}


def bandwidth_rel(threshold_db):
    """What p2phd_bandwidth takes as `rel`: 10^(-threshold_db / 10), computed once."""
    return 10.0 ** (-float(threshold_db) / 10.0)


def bandwidth_notes(input_hz, original_hz, lr_nyquist):
    """The two remarks of the bandwidth report, host logic: an input whose band ends under 0.9 of the low rate's Nyquist frequency,
    and an original (None: there is none) whose band ends at or under 1.05 times that frequency."""
    notes = []
    if input_hz < 0.9 * lr_nyquist:
        notes.append("the input's band ends at %.2f kHz, under the low rate's Nyquist frequency %.2f kHz: the generator was trained on "
                     "inputs that reach it" % (input_hz / 1000.0, lr_nyquist / 1000.0))
    if original_hz is not None and original_hz <= 1.05 * lr_nyquist:
        notes.append("the original's band ends at %.2f kHz, the low rate's Nyquist frequency is %.2f kHz: the original carries nothing above "
                     "it: LSD-HF compares against an empty band" % (original_hz / 1000.0, lr_nyquist / 1000.0))
    return notes


def stereo_split_bin(hr_rate, lr_rate, n_fft):
    """The bin at which the stereo report splits the spectrum: the first bin of an n_fft-point transform at `hr_rate` that lies at or
    above the low rate's Nyquist frequency, ceil(lr_rate n_fft / (2 hr_rate)) in exact arithmetic.  ValueError unless it lies in
    [1, K - 1], K = n_fft / 2 + 1: both bands need a bin."""
    for name, v in (('hr_rate', hr_rate), ('lr_rate', lr_rate)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < v < float('inf'):
            raise ValueError("stereo_split_bin: %s must be a number > 0, got %r" % (name, v))
    if not _is_int(n_fft) or n_fft < 2:
        raise ValueError("stereo_split_bin: n_fft must be an int >= 2, got %r" % (n_fft,))
    k = math.ceil(Fraction(lr_rate) * n_fft / (2 * Fraction(hr_rate)))
    K = n_fft // 2 + 1
    if not 1 <= k <= K - 1:
        raise ValueError("stereo_split_bin: the low rate's Nyquist frequency %g Hz falls on bin %d of %d at %g Hz: the split must lie in "
                         "[1, %d]" % (lr_rate / 2.0, k, K, hr_rate, K - 1))
    return k


def check_stereo(stereo='lr', who="SuperResolver"):
    """Validates the stereo mode -> the mode, one of STEREO_MODES."""
    if stereo not in STEREO_MODES:
        raise ValueError("%s: stereo must be 'lr' or 'ms', got %r" % (who, stereo))
    return stereo


def check_norm_scope(norm_scope='group', who="SuperResolver"):
    """Validates the normalisation scope -> the scope, one of NORM_SCOPES."""
    if norm_scope not in NORM_SCOPES:
        raise ValueError("%s: norm_scope must be 'group' or 'clip', got %r" % (who, norm_scope))
    return norm_scope


def check_segment_norm(segment_norm=False, norm_scope='group', who="SuperResolver"):
    """Validates the per-segment normalisation option -> the bool.  It is an option of its own beside `norm_scope`: with it every
    segment has its own range, so there is no scope to choose, and together with norm_scope 'clip' it is a ValueError."""
    if not isinstance(segment_norm, bool):
        raise ValueError("%s: segment_norm must be a bool, got %r" % (who, segment_norm))
    check_norm_scope(norm_scope, who)
    if segment_norm and norm_scope != 'group':
        raise ValueError("%s: segment_norm gives every segment its own range and norm_scope %r one per clip: choose one of the two"
                         % (who, norm_scope))
    return segment_norm


def group_rows_plan(rows, batch):
    """How segment_norm walks the `rows` = C * S channel-major rows of a clip in groups of `batch`, without regard to channel ->
    a list of (r0, n): group g holds the rows r0 .. r0 + n - 1 and batch - n filler rows of zeros behind them.  Every row is in
    exactly one group, n == batch in every group but the last, 1 <= n <= batch there; no rows, no groups."""
    for name, v in (('rows', rows), ('batch', batch)):
        if not _is_int(v):
            raise ValueError("group_rows_plan: %s must be an int, got %r" % (name, v))
    if rows < 0:
        raise ValueError("group_rows_plan: rows must be >= 0, got %d" % rows)
    if batch < 1:
        raise ValueError("group_rows_plan: batch must be >= 1, got %d" % batch)
    return [(r0, min(batch, rows - r0)) for r0 in range(0, rows, batch)]


PACK_MAX_BYTES = 1 << 30                                                    # the float32 clips one pack holds on the device at most


def check_pack_files(pack_files=1, segment_norm=True, loudness_scope='file', who="enhance_folder"):
    """Validates the folder option pack_files -> the int: how many consecutive files of a folder share generator groups, 1 (the
    default) for none.  More than one needs segment_norm -- only then is a row of a group independent of its neighbours -- and is
    not built for loudness_scope 'folder', whose phase A is not packed: a ValueError each."""
    if isinstance(pack_files, bool) or not _is_int(pack_files) or pack_files < 1:
        raise ValueError("%s: pack_files must be an int >= 1, got %r" % (who, pack_files))
    if pack_files > 1 and not segment_norm:
        raise ValueError("%s: pack_files %d lets the files of a folder share groups, which needs segment_norm: only there does a row "
                         "of a group not depend on its neighbours" % (who, pack_files))
    if pack_files > 1 and loudness_scope == 'folder':
        raise ValueError("%s: pack_files is not built for loudness_scope 'folder' (the album's first pass is not packed)" % who)
    return int(pack_files)


def pack_plan(sizes, pack_files, max_bytes=PACK_MAX_BYTES):
    """How a folder's accepted files form packs: `sizes` -- the bytes of every file's float32 clip, in plan order -> a list of packs,
    each a list of consecutive indices into `sizes`.  A pack closes at `pack_files` files, and before the file with which its
    clips would exceed `max_bytes`; a file larger than that is a pack of its own.  Every file is in exactly one pack, in order."""
    pack_files = check_pack_files(pack_files, who="pack_plan")
    if not _is_int(max_bytes) or max_bytes < 1:
        raise ValueError("pack_plan: max_bytes must be an int >= 1, got %r" % (max_bytes,))
    packs, held = [], 0
    for i, size in enumerate(sizes):
        if not _is_int(size) or size < 0:
            raise ValueError("pack_plan: sizes must be ints >= 0, got %r" % (size,))
        if not packs or len(packs[-1]) >= pack_files or held + size > max_bytes:
            packs.append([])
            held = 0
        packs[-1].append(i)
        held += size
    return packs


def resample_geometry(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """(o, n, width, klen) of data.resample between two rates -- p2phd_resample_geometry's arithmetic, restated for the host: o and
    n are the rates over their common divisor, an output block of n samples reads the klen = 2 * width + o inputs from j * o - width."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError("resample_geometry: sample rates must be positive, got %d -> %d" % (orig_freq, new_freq))
    gd = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // gd, new_freq // gd
    width = int(math.ceil(lowpass_filter_width * o / (min(o, n) * rolloff)))
    return o, n, width, 2 * width + o


def resample_out_len(T, orig_freq, new_freq):
    """p2phd_resample_out_len: ceil(T * new / orig)."""
    gd = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // gd, int(new_freq) // gd
    return (n * int(T) + o - 1) // o


def check_stream(stream_seconds, who="enhance_file", segment_norm=False, crossover=None, hr_rate=None, loudness=None, speech_level=None,
                 clip='clamp', true_peak=False, limiter=False, report_peaks=False, spectrogram=None, bandwidth=False, stereo_report=False,
                 output_rate=None, extended_metrics=False, container='wav', dither=None, pack_files=1, loudness_scope='file'):
    """Validates the option stream_seconds against everything it is not built with -> None (off), or the window's length in seconds.
    A streamed file is never on the device as a whole: what needs the whole clip, or a figure of the whole file, is a ValueError
    that names the option, before a file is opened."""
    if stream_seconds is None:
        return None
    w = stream_seconds
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or not w > 0:
        raise ValueError("%s: stream_seconds must be a finite number above 0, got %r" % (who, stream_seconds))
    if not segment_norm:
        raise ValueError("%s: stream_seconds sends a file through in windows, which needs segment_norm: only there does a segment's "
                         "range not depend on the rest of the file" % who)
    if crossover is not None:
        raise ValueError("%s: stream_seconds is not built with the crossover (its filter reads across the windows)" % who)
    whole = (('loudness', loudness is not None), ('speech_level', speech_level is not None), ('clip=%r' % (clip,), clip != 'clamp'),
             ('true_peak', bool(true_peak)), ('limiter', bool(limiter)), ('report_peaks', bool(report_peaks)),
             ('spectrogram', spectrogram is not None), ('bandwidth', bool(bandwidth)), ('stereo_report', bool(stereo_report)),
             ('output_rate', output_rate is not None and (hr_rate is None or int(output_rate) != int(hr_rate))),
             ('extended_metrics', bool(extended_metrics)), ("container='flac'", container == 'flac'), ("dither='shaped'", dither == 'shaped'),
             ('pack_files > 1', not isinstance(pack_files, int) or pack_files > 1), ("loudness_scope='folder'", loudness_scope == 'folder'))
    for name, on in whole:
        if on:
            raise ValueError("%s: stream_seconds is not built with %s: it needs the whole clip, or a figure of the whole file" % (who, name))
    return float(w)


def _stage_inputs(A, B, o, n, width, len_in):
    """The inputs a window must hold so that a resampler stage's outputs [A, B) come out as in a run over the whole row: the range
    widened outward to whole blocks, a halo of `width` in front -- rounded up to whole blocks, so that the window starts on one -- and
    of width + o behind, cut at the ends of the row."""
    j_a, j_b = A // n, -(-B // n)
    a = max(0, (j_a - -(-width // o)) * o)
    b = min(len_in, j_b * o + width + o)
    return a, max(a, b)


def stream_plan(frames, in_rate, lr_rate, hr_rate, is_lr_input, T, overlap, C, batch, stream_seconds):
    """How a file of `frames` frames at `in_rate` goes through the pipeline in windows of about `stream_seconds` -> {'L', 'S',
    'stride', 'V' (segment_plan's, of the whole clip: L follows from the header alone), 'K' (segments per channel and window),
    'stages' (the resamplers of the low-rate round trip that are not the identity, [(orig, new, o, n, width, rows in, rows out)]),
    'windows'}.  K = max(1, round(stream_seconds * hr_rate / stride)), rounded up to a multiple of batch / gcd(batch, C): the C * K
    rows of a window fill whole groups and only the last window has filler rows.  A window: {'s0', 's1' (its segments [s0, s1) of
    every channel), 'emit' (the output positions it writes, [s0 * stride, s1 * stride), the last window up to L: the windows'
    ranges partition [0, L) in order), 'need' (the round-tripped clip it gathers from, [s0 * stride, (s1 - 1) * stride + T) cut to
    [0, L)), 'read' (the frames of the file to read), 'cuts' (per stage, the slice of its output that is the next stage's input
    -- the last one's: the needed range -- as local indices (lo, hi)), 'inputs' (per stage, the range of its input row the window
    holds)}.  A stage's window starts on a multiple of its o, so output m of the whole row is the window's output m - (start / o) * n,
    computed from the same operands in the same order wherever every input the sum reads is inside the window or outside the row."""
    frames, C, batch, T = int(frames), int(C), int(batch), int(T)
    if frames < 0 or C < 1 or batch < 1:
        raise ValueError("stream_plan: need frames >= 0, C >= 1 and batch >= 1, got %d, %d and %d" % (frames, C, batch))
    if isinstance(stream_seconds, bool) or not isinstance(stream_seconds, (int, float)) or not math.isfinite(stream_seconds) or not stream_seconds > 0:
        raise ValueError("stream_plan: stream_seconds must be a finite number above 0, got %r" % (stream_seconds,))
    chain = [(in_rate, hr_rate)] if is_lr_input else [(in_rate, lr_rate), (lr_rate, hr_rate)]
    stages, n_in = [], frames
    for orig, new in chain:
        if int(orig) == int(new):
            continue
        o, n, width, _ = resample_geometry(orig, new)
        n_out = resample_out_len(n_in, orig, new)
        stages.append((int(orig), int(new), o, n, width, n_in, n_out))
        n_in = n_out
    L = frames if not is_lr_input and int(in_rate) == int(hr_rate) else n_in       # (the round trip rounds the length up: cut)
    S, stride, V = segment_plan(L, T, overlap)
    unit = batch // math.gcd(batch, C)
    K = max(1, int(math.floor(stream_seconds * hr_rate / stride + 0.5)))
    K = -(-K // unit) * unit
    windows = []
    for s0 in range(0, S, K):
        s1 = min(S, s0 + K)
        need = (min(s0 * stride, L), min((s1 - 1) * stride + T, L))
        inputs, cuts, (A, B) = [], [], need
        for _, _, o, n, width, rows_in, _ in reversed(stages):
            a, b = _stage_inputs(A, B, o, n, width, rows_in)
            cuts.append((A - a // o * n, B - a // o * n))
            inputs.append((a, b))
            A, B = a, b
        windows.append({'s0': s0, 's1': s1, 'emit': (s0 * stride, L if s1 == S else s1 * stride), 'need': need, 'read': (A, B),
                        'cuts': cuts[::-1], 'inputs': inputs[::-1]})
    return {'L': L, 'S': S, 'stride': stride, 'V': V, 'K': K, 'stages': stages, 'windows': windows}


def check_stereo_report(stereo_report=False, opts=None, loudness_scope='file', who="enhance_file"):
    """Validates the stereo report option -> None (off), or the plan {'n_fft', 'hop'} that ops.stereo_image takes.  `stereo_report`:
    a bool.  `opts`: None or a dict of those two, None or absent standing for STEREO_DEFAULTS' value (hop: half of a given n_fft):
    `n_fft` a power of two in [64, 2048]; `hop` 1 .. n_fft.  They are options of the option.  The report is one file's: with
    loudness_scope 'folder' it is a ValueError, as the bandwidth report is.  A ValueError names the argument."""
    if not isinstance(stereo_report, bool):
        raise ValueError("%s: stereo_report must be a bool, got %r" % (who, stereo_report))
    if opts is not None and not isinstance(opts, dict):
        raise ValueError("%s: stereo_report_opts must be None or a dict, got %r" % (who, opts))
    if not stereo_report:
        if opts is not None:
            raise ValueError("%s: stereo_report_opts are options of stereo_report=True; stereo_report is False" % who)
        return None
    if loudness_scope == 'folder':
        raise ValueError("%s: stereo_report is not built for loudness_scope='folder': the report is measured per file" % who)
    opts = {k: v for k, v in (opts or {}).items() if v is not None}
    unknown = sorted(set(opts) - set(STEREO_DEFAULTS))
    if unknown:
        raise ValueError("%s: unknown stereo_report_opts %s" % (who, unknown))
    n_fft = opts.get('n_fft', STEREO_DEFAULTS['n_fft'])
    if not _is_int(n_fft) or not 64 <= n_fft <= 2048 or n_fft & (n_fft - 1):
        raise ValueError("%s: stereo_report n_fft must be a power of two in [64, 2048], got %r" % (who, n_fft))
    hop = opts.get('hop', STEREO_DEFAULTS['hop'] if 'n_fft' not in opts else n_fft // 2)
    if not _is_int(hop) or not 1 <= hop <= n_fft:
        raise ValueError("%s: stereo_report hop must be an int in [1, n_fft = %d], got %r" % (who, n_fft, hop))
    return {'n_fft': n_fft, 'hop': hop}


def _ratio_db(num, den):
    """10 log10(num / den) of two sums that are powers up to rounding: None where both vanish, +inf where only the denominator does,
    -inf where only the numerator does (a sum a rounding error under zero counts as vanished); NaN stays NaN."""
    if num != num or den != den:
        return float('nan')
    if den <= 0.0:
        return None if num <= 0.0 else float('inf')
    if num <= 0.0:
        return float('-inf')
    if num == float('inf') or den == float('inf'):
        return float('nan') if num == den else (float('inf') if num > den else float('-inf'))
    return 10.0 * math.log10(num / den)


def stereo_figures(res8):
    """The eight fetched sums of p2phd_stereo_bands ({S_ll, S_rr, Re, Im} below the split, then above it) -> {'low': figures, 'high':
    figures}, host arithmetic in float64.  figures = {'corr': Re / sqrt(S_ll S_rr), the correlation of the band's two channels;
    'coherence': hypot(Re, Im) / sqrt(S_ll S_rr), which a delay between the channels does not lower; 'side_db': 10 log10((S_ll + S_rr
    - 2 Re) / (S_ll + S_rr + 2 Re)), the level of L - R against L + R; 'balance_db': 10 log10(S_ll / S_rr)}.  None where a
    denominator is zero (an empty band, a silent channel), +-inf where a ratio is."""
    v = [float(t) for t in res8]
    if len(v) != 8:
        raise ValueError("stereo_figures: expected the eight sums of two bands, got %d values" % len(v))
    out = {}
    for name, (ll, rr, re, im) in (('low', v[:4]), ('high', v[4:])):
        prod = ll * rr
        den = math.sqrt(prod) if prod > 0.0 else (float('nan') if prod != prod else 0.0)
        out[name] = {'corr': None if den == 0.0 else re / den,
                     'coherence': None if den == 0.0 else math.hypot(re, im) / den,
                     'side_db': _ratio_db(ll + rr - 2.0 * re, ll + rr + 2.0 * re),
                     'balance_db': _ratio_db(ll, rr)}
    return out


def stereo_notes(output, mode):
    """The one remark of the stereo report, host logic.  `output`: the generated clip's {'low', 'high'} figures; `mode`: the mode
    it was generated in.  With 'lr', a correlation above the split that is more than STEREO_NOTE_DROP under the one below it: the
    channels' new band was invented twice, which stereo='ms' avoids."""
    lo, hi = output['low']['corr'], output['high']['corr']
    if mode != 'lr' or lo is None or hi is None or not hi < lo - STEREO_NOTE_DROP:
        return []
    return ["the generated clip's channels correlate %+.2f above the split and %+.2f below it: left and right were generated "
            "independently; stereo='ms' (--stereo ms) generates what they share once" % (hi, lo)]


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def check_spectrogram(n_fft=None, hop=None, width=None, height=None, range_db=None, gap=None, top_db=None, channel=0,
                      who="enhance_file"):
    """Validates the options of the spectrogram picture, None standing for SPECTROGRAM_DEFAULTS' value -> the plan
    {'n_fft', 'hop', 'width', 'height', 'range_db', 'gap'} that ops.stft_db / ops.spectrogram_rgb take.  `n_fft`: a power of
    two in [64, 2048]; `hop`: 1 .. n_fft; `width`, `height` (of one panel): 1 .. 16384; `range_db`: finite and > 0; `gap`:
    0 .. 64; `top_db` (not part of the plan): None -- the picture's own maximum -- or a finite level; `channel`: an int >= 0.
    A ValueError names the argument."""
    d = SPECTROGRAM_DEFAULTS
    n_fft, hop = (d['n_fft'] if n_fft is None else n_fft), (d['hop'] if hop is None else hop)
    width, height = (d['width'] if width is None else width), (d['height'] if height is None else height)
    range_db, gap = (d['range_db'] if range_db is None else range_db), (d['gap'] if gap is None else gap)
    if not _is_int(n_fft) or not 64 <= n_fft <= 2048 or n_fft & (n_fft - 1):
        raise ValueError("%s: spectrogram n_fft must be a power of two in [64, 2048], got %r" % (who, n_fft))
    if not _is_int(hop) or not 1 <= hop <= n_fft:
        raise ValueError("%s: spectrogram hop must be an int in [1, n_fft = %d], got %r" % (who, n_fft, hop))
    for name, v in (('width', width), ('height', height)):
        if not _is_int(v) or not 1 <= v <= SPECTROGRAM_MAX_SIDE:
            raise ValueError("%s: spectrogram %s must be an int in [1, %d], got %r" % (who, name, SPECTROGRAM_MAX_SIDE, v))
    if isinstance(range_db, bool) or not isinstance(range_db, (int, float)) or not 0.0 < range_db < float('inf'):
        raise ValueError("%s: spectrogram range_db must be finite and > 0, got %r" % (who, range_db))
    if not _is_int(gap) or not 0 <= gap <= SPECTROGRAM_MAX_GAP:
        raise ValueError("%s: spectrogram gap must be an int in [0, %d], got %r" % (who, SPECTROGRAM_MAX_GAP, gap))
    if top_db is not None and (isinstance(top_db, bool) or not isinstance(top_db, (int, float)) or not math.isfinite(top_db)):
        raise ValueError("%s: spectrogram top_db must be None (the picture's own maximum) or a finite level in dB, got %r" % (who, top_db))
    if not _is_int(channel) or channel < 0:
        raise ValueError("%s: spectrogram channel must be an int >= 0, got %r" % (who, channel))
    return {'n_fft': n_fft, 'hop': hop, 'width': width, 'height': height, 'range_db': float(range_db), 'gap': gap}


def loudness_channel_weights(channels):
    """The BS.1770 channel weights of a clip of `channels` channels: all 1, except six channels in WAVE order (L R C LFE Ls Rs),
    where the LFE does not count and the surrounds count 1.41."""
    channels = int(channels)
    if channels < 1:
        raise ValueError("loudness_channel_weights: need at least one channel, got %d" % channels)
    return (1.0, 1.0, 1.0, 0.0, 1.41, 1.41) if channels == 6 else (1.0,) * channels


def check_loudness_rate(rate, who):
    """The rates p2phd_loudness_coeffs_fill takes: a multiple of 10 in [8000, 384000] Hz."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not LOUDNESS_MIN_RATE <= rate <= LOUDNESS_MAX_RATE \
            or rate != int(rate) or int(rate) % 10:
        raise ValueError("%s: loudness is measured in hops of rate / 10 samples: the rate must be a multiple of 10 in [%d, %d] Hz, got %r"
                         % (who, LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE, rate))
    return int(rate)


def check_loudness(loudness, hr_rate, who="enhance_file", max_gain_db=None, loudness_range=False):
    """Validates the loudness option for a file written at `hr_rate` -> None (off), or {'mode': 'report' | 'input' | 'target',
    'target': the level in LUFS (None unless a number was given), 'max_gain_db'}.  `loudness`: None, 'report' (measure only),
    'input' (the written clip as loud as the clip the generator was given) or a number in [-70, 0], the target in LUFS.
    `max_gain_db`: None (LOUDNESS_MAX_GAIN_DB) or a finite level >= 0, an option of the option.  `loudness_range`: a bool, an option
    of the option too (also measure the loudness range and the maximum short-term loudness); the dict then gains 'range': True."""
    if not isinstance(loudness_range, bool):
        raise ValueError("%s: loudness_range must be a bool, got %r" % (who, loudness_range))
    if loudness is None:
        if max_gain_db is not None:
            raise ValueError("%s: loudness_max_gain_db is an option of loudness; loudness is None" % who)
        if loudness_range:
            raise ValueError("%s: loudness_range is an option of loudness; loudness is None" % who)
        return None
    if max_gain_db is None:
        max_gain_db = LOUDNESS_MAX_GAIN_DB
    if isinstance(max_gain_db, bool) or not isinstance(max_gain_db, (int, float)) or not 0.0 <= max_gain_db < float('inf'):
        raise ValueError("%s: loudness_max_gain_db must be finite and >= 0, got %r" % (who, max_gain_db))
    if isinstance(loudness, str):
        if loudness not in LOUDNESS_MODES:
            raise ValueError("%s: loudness must be None, 'report', 'input' or a target in LUFS, got %r" % (who, loudness))
        mode, target = loudness, None
    else:
        if isinstance(loudness, bool) or not isinstance(loudness, (int, float)) or not -70.0 <= loudness <= 0.0:
            raise ValueError("%s: a loudness target must be a level in [-70, 0] LUFS, got %r" % (who, loudness))
        mode, target = 'target', float(loudness)
    check_loudness_rate(hr_rate, who)
    loud = {'mode': mode, 'target': target, 'max_gain_db': float(max_gain_db)}
    if loudness_range:
        loud['range'] = True
    return loud


def check_loudness_scope(loudness_scope, loud, who="enhance_folder", folder=True, limiter=False, spectrogram=None, album_cache_bytes=None):
    """Validates the scope of the loudness option -> None ('file': every file is measured and normalised on its own), or
    {'cache_bytes'} ('folder': the folder is one programme with one loudness gain and one guard gain).  `loud`: check_loudness'
    result; `folder`: whether a folder is being enhanced; `limiter` (a bool) and `spectrogram` (None or a path): the options that
    are not built for the folder scope, like loud['range'].  `album_cache_bytes`: None (ALBUM_CACHE_BYTES) or an int >= 0, an option
    of the folder scope: the bytes of generated clips kept on the device between measuring and writing."""
    if loudness_scope not in LOUDNESS_SCOPES:
        raise ValueError("%s: loudness_scope must be 'file' or 'folder', got %r" % (who, loudness_scope))
    if loudness_scope == 'file':
        if album_cache_bytes is not None:
            raise ValueError("%s: album_cache_bytes is an option of loudness_scope='folder'; loudness_scope is 'file'" % who)
        return None
    if not folder:
        raise ValueError("%s: loudness_scope='folder' is an option of folder mode (enhance_folder, --input DIR): one file is no album" % who)
    if loud is None:
        raise ValueError("%s: loudness_scope='folder' is an option of loudness; loudness is None" % who)
    if limiter:
        raise ValueError("%s: limiter is not built for loudness_scope='folder': the guard gain it leaves behind is one file's" % who)
    if loud.get('range', False):
        raise ValueError("%s: loudness_range is not built for loudness_scope='folder': the range is measured per file" % who)
    if spectrogram is not None:
        raise ValueError("%s: spectrogram is not built for loudness_scope='folder': the picture is rendered while its file's clips are "
                         "on the device" % who)
    if album_cache_bytes is None:
        album_cache_bytes = ALBUM_CACHE_BYTES
    if not _is_int(album_cache_bytes) or album_cache_bytes < 0:
        raise ValueError("%s: album_cache_bytes must be an int >= 0 (0: keep no generated clip on the device), got %r" % (who, album_cache_bytes))
    return {'cache_bytes': int(album_cache_bytes)}


def check_speech_level_rate(rate, who):
    """The rates p2phd_speechlevel_consts_fill takes: an int in [8000, 192000] Hz."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not SPEECH_LEVEL_MIN_RATE <= rate <= SPEECH_LEVEL_MAX_RATE or rate != int(rate):
        raise ValueError("%s: the active speech level is measured at a whole rate in [%d, %d] Hz, got %r"
                         % (who, SPEECH_LEVEL_MIN_RATE, SPEECH_LEVEL_MAX_RATE, rate))
    return int(rate)


def check_speech_level(value, who="enhance_file", max_gain_db=None, loudness=None):
    """Validates the speech-level option -> None (off), or {'mode': 'report' | 'input' | 'target', 'target': the level in dBov (None
    unless a number was given), 'max_gain_db'}.  `value`: None, 'report' (measure only), 'input' (the written clip at the active
    speech level of the clip the generator was given) or a finite number in [-70, 0], the target in dBov.  `max_gain_db`: None
    (SPEECH_LEVEL_DEFAULTS) or a level in [0, 120], an option of the option.  `loudness`: the loudness option, which claims the
    same gain: both at once are refused (and with it loudness_range and loudness_scope='folder', options of that option)."""
    if value is None:
        if max_gain_db is not None:
            raise ValueError("%s: speech_level_max_gain_db is an option of speech_level; speech_level is None" % who)
        return None
    if loudness is not None:
        raise ValueError("%s: speech_level and loudness are two claims on the one gain in front of the output stage; give one of them" % who)
    if max_gain_db is None:
        max_gain_db = SPEECH_LEVEL_DEFAULTS['max_gain_db']
    if isinstance(max_gain_db, bool) or not isinstance(max_gain_db, (int, float)) or not 0.0 <= max_gain_db <= 120.0:
        raise ValueError("%s: speech_level_max_gain_db must be in [0, 120], got %r" % (who, max_gain_db))
    if isinstance(value, str):
        if value not in SPEECH_LEVEL_MODES:
            raise ValueError("%s: speech_level must be None, 'report', 'input' or a target in dBov, got %r" % (who, value))
        mode, target = value, None
    else:
        if isinstance(value, bool) or not isinstance(value, (int, float)) or not -70.0 <= value <= 0.0:
            raise ValueError("%s: a speech_level target must be a finite level in [-70, 0] dBov, got %r" % (who, value))
        mode, target = 'target', float(value)
    return {'mode': mode, 'target': target, 'max_gain_db': float(max_gain_db)}


def truepeak_plan(rate):
    """The interpolator of the true-peak measurement for a clip at `rate`, host arithmetic only -> {'factor', 'taps_per_phase': 24,
    'beta': 9.0} for p2phd_truepeak_taps_fill: the factor is 4 below 96 kHz, 2 below 192 kHz and 1 from there on, so that the
    oversampled rate is at least 192 kHz, as ITU-R BS.1770-4 Annex 2 asks."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 < rate < float('inf'):
        raise ValueError("truepeak_plan: the rate must be a number > 0, got %r" % (rate,))
    factor = 1
    while factor < 4 and rate * factor < TRUEPEAK_MIN_OVERSAMPLED_RATE:
        factor *= 2
    return {'factor': factor, 'taps_per_phase': TRUEPEAK_TAPS_PER_PHASE, 'beta': TRUEPEAK_BETA}


def check_true_peak(true_peak, stage, encoding, hr_rate, who="enhance_file"):
    """Validates the true-peak option -> (stage, tp).  Off (False): the stage as it came and None.  On: the stage -- where every
    output option is at its default, the one of a plain report, so that the result has its 'output' -- and {'rate', 'ceiling': the
    linear level clip='guard' brings the true peak down to (the stage's ceiling, read as dBTP, else the encoding's limit), 'limit':
    the encoding's limit, above which clip='error' refuses}."""
    if not isinstance(true_peak, bool):
        raise ValueError("%s: true_peak must be a bool, got %r" % (who, true_peak))
    if not true_peak:
        return stage, None
    truepeak_plan(hr_rate)
    if stage is None:
        stage = {'clip': 'clamp', 'ceiling': None, 'dither': None, 'seed': 0, 'report': False}
    limit = encoding_limit(encoding)
    return stage, {'rate': hr_rate, 'ceiling': limit if stage['ceiling'] is None else stage['ceiling'], 'limit': limit}


def check_output_rate(output_rate, hr_rate, who="enhance_file", loudness_scope='file', spectrogram=None):
    """Validates the output-rate option for a model that generates at `hr_rate` -> None (off: `output_rate` is None or the model's
    rate, and nothing changes), or the option {'rate', 'model_rate', 'plan'}: `plan` is ops.rateconv_plan's dict for hr_rate ->
    output_rate with RATECONV_DEFAULTS.  `output_rate`: an int >= 8000 Hz.  Not built with `spectrogram` (the picture's panels share
    one frequency axis) or loudness_scope 'folder' (generate/album.py runs the per-file flow up to the metrics only); rates between which the
    converter is not built are refused with p2phd_rateconv_plan's text.  A ValueError each, before a file is opened."""
    if output_rate is None:
        return None
    if not _is_int(output_rate) or output_rate < OUTPUT_MIN_RATE:
        raise ValueError("%s: output_rate must be an int >= %d Hz, got %r" % (who, OUTPUT_MIN_RATE, output_rate))
    if hr_rate == output_rate:
        return None
    if hr_rate != int(hr_rate) or int(hr_rate) < 1:
        raise ValueError("%s: output_rate converts from the model's rate, which must be a whole number of Hz, got %r" % (who, hr_rate))
    if spectrogram is not None:
        raise ValueError("%s: spectrogram is not built with output_rate: its panels share one frequency axis and the written clip "
                         "would have another" % who)
    if loudness_scope == 'folder':
        raise ValueError("%s: output_rate is not built for loudness_scope='folder': the album flow writes at the model's rate" % who)
    from .ops import rateconv_plan
    try:
        plan = rateconv_plan(int(hr_rate), output_rate)
    except ValueError as e:
        raise ValueError("%s: output_rate %d: %s" % (who, output_rate, e))
    return {'rate': output_rate, 'model_rate': int(hr_rate), 'plan': plan}


def output_rate_line(rc):
    """The start-up line of the output-rate option."""
    p = rc['plan']
    return ('output rate: %d Hz (%d taps x %d phases, flat to %.2f kHz, -%g dB from %.2f kHz)'
            % (rc['rate'], p['taps_per_phase'], p['n'], p['passband_hz'] / 1000.0, p['atten_db'], p['stopband_hz'] / 1000.0))


def limiter_plan(rate, lookahead_ms=None, hold_ms=None):
    """The look-ahead and the hold of the limiter for a clip at `rate`, host arithmetic only -> {'lookahead': A, 'hold': H} in
    samples, round(ms * rate / 1000) each, A at least 1.  None: LIMITER_LOOKAHEAD_MS, LIMITER_HOLD_MS.  A value that needs more
    than LIMITER_MAX_LOOKAHEAD / LIMITER_MAX_HOLD samples is a ValueError that names the largest ms allowed at that rate."""
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 < rate < float('inf'):
        raise ValueError("limiter_plan: the rate must be a number > 0, got %r" % (rate,))
    plan = {}
    for key, name, ms, default, cap in (('lookahead', 'lookahead_ms', lookahead_ms, LIMITER_LOOKAHEAD_MS, LIMITER_MAX_LOOKAHEAD),
                                        ('hold', 'hold_ms', hold_ms, LIMITER_HOLD_MS, LIMITER_MAX_HOLD)):
        if ms is None:
            ms = default
        if isinstance(ms, bool) or not isinstance(ms, (int, float)) or not 0.0 <= ms < float('inf'):
            raise ValueError("limiter_plan: %s must be a finite number >= 0, got %r" % (name, ms))
        n = int(round(ms * rate / 1000.0))
        if n > cap:
            raise ValueError("limiter_plan: %s %g is %d samples at %g Hz, more than %d: at most %g ms at that rate"
                             % (name, ms, n, rate, cap, cap * 1000.0 / rate))
        plan[key] = max(n, 1) if key == 'lookahead' else n
    return plan


def check_limiter(limiter, lookahead_ms, hold_ms, stage, encoding, hr_rate, who="enhance_file"):
    """Validates the limiter option -> None (off), or {'lookahead', 'hold' (limiter_plan), 'lookahead_ms', 'hold_ms' (as given)}.
    `limiter`: a bool.  It is an option of clip='guard' (`stage`: check_output_options' result), whose ceiling it holds the crests
    under and whose one gain removes what is left; `lookahead_ms` and `hold_ms` are options of the option.  The caller switches the
    true-peak measurement on with it (check_true_peak(True, ...)): the limiter's envelope is the true-peak one."""
    if not isinstance(limiter, bool):
        raise ValueError("%s: limiter must be a bool, got %r" % (who, limiter))
    if not limiter:
        if lookahead_ms is not None or hold_ms is not None:
            raise ValueError("%s: limiter_lookahead_ms / limiter_hold_ms are options of limiter=True; limiter is False" % who)
        return None
    if stage is None or stage['clip'] != 'guard':
        raise ValueError("%s: limiter is an option of clip='guard' (it holds the crests under the guard's ceiling and the guard's one "
                         "gain removes what is left); clip is %r" % (who, 'clamp' if stage is None else stage['clip']))
    check_encoding(encoding, who)
    try:
        plan = limiter_plan(hr_rate, lookahead_ms, hold_ms)
    except ValueError as e:
        raise ValueError("%s: %s" % (who, e))
    return dict(plan, lookahead_ms=lookahead_ms, hold_ms=hold_ms)


def spectrogram_lut():
    """The palette of the spectrogram picture: a 256 x 3 uint8 numpy array, index 0 the quietest.  Anchors
    (SPECTROGRAM_LUT_ANCHORS): 0 (0, 0, 4) near-black, 64 (30, 20, 140) blue, 128 (180, 40, 150) magenta, 192 (250, 140, 30)
    orange, 255 (255, 250, 190) pale yellow; between two anchors (i0, a) and (i1, b) every channel is
    a + (b - a) * (i - i0) // (i1 - i0), integers throughout.  The integer Rec.601 luminance 299 r + 587 g + 114 b never
    falls as the index rises, so a grey-scale print keeps the order."""
    import numpy as np
    lut = np.zeros((256, 3), dtype=np.uint8)
    for (i0, a), (i1, b) in zip(SPECTROGRAM_LUT_ANCHORS[:-1], SPECTROGRAM_LUT_ANCHORS[1:]):
        for i in range(i0, i1 + 1):
            lut[i] = [a[c] + (b[c] - a[c]) * (i - i0) // (i1 - i0) for c in range(3)]
    return lut


# extensions a folder scan can list: RIFF/WAVE, FLAC, and the big-endian containers of data/containers.py (AIFF / AIFF-C, AU, SPHERE)
INPUT_FORMATS = ('wav', 'flac', 'aif', 'aiff', 'aifc', 'au', 'snd', 'sph')


def check_input_formats(formats, who="plan_folder"):
    """`formats`: a sequence of extensions, or one string with commas ('wav,flac') -> a tuple of INPUT_FORMATS' members, lower case,
    without duplicates; anything else is a ValueError."""
    names = formats.split(',') if isinstance(formats, str) else list(formats)
    out = []
    for f in names:
        f = f.strip().lower().lstrip('.') if isinstance(f, str) else f
        if f not in INPUT_FORMATS:
            raise ValueError("%s: input formats must be of %s, got %r" % (who, list(INPUT_FORMATS), formats))
        if f not in out:
            out.append(f)
    if not out:
        raise ValueError("%s: no input format given" % who)
    return tuple(out)


CONTAINERS = ('wav', 'flac')                                                # what the per-file flow can write
FLAC_BLOCK = 4096                                                           # samples per FLAC frame where none is asked for
FLAC_LPC_MAX = 12                                                           # the largest LPC order of the option flac_lpc
FLAC_LPC_BLOCK = 16384                                                      # the largest block with flac_lpc > 0


def check_container(container, flac_block, flac_md5, encoding, rate, who, flac_lpc=None):
    """The container option of enhance_file / enhance_folder -> None ('wav': nothing changes), or {'block', 'md5'} for 'flac'.
    `rate`: the rate that will be written.  A ValueError each: an unknown container; flac_block or flac_md5 without 'flac';
    'flac' with an encoding that is not integer PCM, a block outside 16 .. 65535, a rate above 1048575 (STREAMINFO has 20 bits).
    `flac_lpc`: None, or the largest LPC order M the encoder tries, an int in 0 .. 12; the dict gains 'lpc': M where M > 0.  A
    ValueError: without 'flac', outside the range, or M > 0 with a block above 16384."""
    if container not in CONTAINERS:
        raise ValueError("%s: container must be one of %s, got %r" % (who, list(CONTAINERS), container))
    if container == 'wav':
        if flac_lpc is not None:
            raise ValueError("%s: flac_lpc is an option of container='flac'; container is 'wav'" % who)
        if flac_block is not None or flac_md5:
            raise ValueError("%s: flac_block / flac_md5 are options of container='flac'; container is 'wav'" % who)
        return None
    if encoding not in ('pcm16', 'pcm24'):
        raise ValueError("%s: container='flac' holds integer samples: encoding must be 'pcm16' or 'pcm24', got %r" % (who, encoding))
    block = FLAC_BLOCK if flac_block is None else flac_block
    if isinstance(block, bool) or not isinstance(block, int) or not 16 <= block <= 65535:
        raise ValueError("%s: flac_block must be an int in 16 .. 65535, got %r" % (who, flac_block))
    if not 1 <= int(rate) <= 1048575:
        raise ValueError("%s: container='flac' states the rate in 20 bits: at most 1048575 Hz, got %r" % (who, rate))
    if flac_lpc is not None:
        if isinstance(flac_lpc, bool) or not isinstance(flac_lpc, int) or not 0 <= flac_lpc <= FLAC_LPC_MAX:
            raise ValueError("%s: flac_lpc must be an int in 0 .. %d, got %r" % (who, FLAC_LPC_MAX, flac_lpc))
        if flac_lpc > 0 and block > FLAC_LPC_BLOCK:
            raise ValueError("%s: with flac_lpc > 0 flac_block is at most %d, got %r" % (who, FLAC_LPC_BLOCK, block))
        if flac_lpc > 0:
            return {'block': block, 'md5': bool(flac_md5), 'lpc': flac_lpc}
    return {'block': block, 'md5': bool(flac_md5)}


def plan_folder(dir_in, dir_out, formats=('wav',), ext='.wav'):
    """[(relative path, input path, output path)] of every *.wav under dir_in, recursive, sorted by relative path; the
    output keeps the relative path under dir_out.  Other files are ignored.  `formats`: the extensions that are listed
    (check_input_formats; default: wav alone); `ext`: the extension every output gets ('.wav'; '.flac' with container='flac'), so
    with the default x.flac or x.aif is written as x.wav, and two inputs that would be written to the same path are a ValueError."""
    if ext not in ('.wav', '.flac'):
        raise ValueError("plan_folder: ext must be '.wav' or '.flac', got %r" % (ext,))
    formats = check_input_formats(formats)
    if not os.path.isdir(dir_in):
        raise NotADirectoryError("%s is not a directory" % dir_in)
    if os.path.exists(dir_out) and not os.path.isdir(dir_out):
        raise NotADirectoryError("--input is a directory, so --output must be one too: %s is a file" % dir_out)
    rel = []
    for root, _, files in os.walk(dir_in):
        for f in files:
            if f.lower().endswith(tuple('.' + x for x in formats)):
                rel.append(os.path.relpath(os.path.join(root, f), dir_in))
    plan, taken = [], {}
    for r in sorted(rel):
        out = r if r.lower().endswith(ext) else os.path.splitext(r)[0] + ext
        if out in taken:
            raise ValueError("%s and %s would both be written to %s" % (os.path.join(dir_in, taken[out]), os.path.join(dir_in, r), os.path.join(dir_out, out)))
        taken[out] = r
        plan.append((r, os.path.join(dir_in, r), os.path.join(dir_out, out)))
    return plan


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
