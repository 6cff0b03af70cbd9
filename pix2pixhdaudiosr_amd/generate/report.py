"""Whole-file generation: the metrics table of --metrics_csv and the lines the command line prints per file."""
import csv

METRICS_COLUMNS = ("file", "channel", "frames", "mse", "snr_sr", "snr_lr", "lsd")
METRICS_COLUMNS_EXT = METRICS_COLUMNS + ("lsd_lf", "lsd_hf", "ssnr_sr", "ssnr_lr")     # --metrics_ext
METRICS_COLUMNS_PEAKS = ("peak_dbfs", "clipped", "gain")                                # --report_peaks
METRICS_COLUMNS_LOUDNESS = ("lufs_in", "lufs_out", "loudness_gain_db")                  # --loudness
METRICS_COLUMNS_LOUDNESS_RANGE = ("lra_in", "lra_out", "short_term_max")               # --loudness_range (behind the loudness columns)
METRICS_COLUMNS_TRUE_PEAK = ("true_peak_dbtp",)                                         # --true_peak
METRICS_COLUMNS_LIMITER = ("limiter_reduction_db", "limited_samples")                   # --limiter
METRICS_COLUMNS_BANDWIDTH = ("bw_in", "bw_out", "bw_orig")                              # --bandwidth (behind every other column)
METRICS_COLUMNS_STEREO = ("corr_lf_out", "corr_hf_out", "corr_hf_orig", "side_hf_out_db")   # --stereo_report (behind those too)
METRICS_COLUMNS_SPEECH_LEVEL = ("asl_in", "asl_out", "activity_out")                    # --speech_level (behind every other column)


def _mean(values):
    return sum(values) / len(values)


def _nanmean(values):
    kept = [v for v in values if v == v]
    return sum(kept) / len(kept) if kept else float('nan')


def _columns(extended, peaks, loudness=False, true_peak=False, limiter=False, loudness_range=False, bandwidth=False, stereo=False, speech_level=False):
    """The columns behind file, channel and frames: [(value for (record, channel), mean over the rows)]."""
    if extended:
        cols = [(lambda r, c, n=n: r['metrics_ext'][c][n], _nanmean) for n in METRICS_COLUMNS_EXT[3:]]
    else:
        cols = [(lambda r, c, k=k: r['metrics'][c][k], _mean) for k in (0, 1, 2, 6)]
    if peaks:
        cols += [(lambda r, c: r['output']['peak_dbfs'][c], _mean), (lambda r, c: r['output']['clipped'][c], _mean),
                 (lambda r, c: r['output']['gain'], _mean)]
    if loudness:
        cols += [(lambda r, c: r['loudness']['input'], _mean), (lambda r, c: r['loudness']['output'], _mean),
                 (lambda r, c: r['loudness']['gain_db'], _mean)]
    if loudness_range:
        cols += [(lambda r, c: r['loudness']['range']['input'], _mean), (lambda r, c: r['loudness']['range']['output'], _mean),
                 (lambda r, c: r['loudness']['range']['short_term_max'], _mean)]
    if true_peak:
        cols += [(lambda r, c: r['output']['true_peak_dbtp'][c], _mean)]
    if limiter:
        cols += [(lambda r, c: r['output']['limiter']['max_reduction_db'], _mean), (lambda r, c: r['output']['limiter']['limited_samples'], _mean)]
    if bandwidth:
        cols += [(lambda r, c, n=n: float('nan') if r['bandwidth'][n] is None else r['bandwidth'][n], _nanmean) for n in ('input', 'output', 'original')]
    if stereo:
        def figure(r, clip, band, name):
            f = None if r.get('stereo') is None or r['stereo'][clip] is None else r['stereo'][clip][band][name]
            return float('nan') if f is None else f
        cols += [(lambda r, c, k=k: figure(r, *k), _nanmean) for k in (('output', 'low', 'corr'), ('output', 'high', 'corr'), ('original', 'high', 'corr'),
                                                                    ('output', 'high', 'side_db'))]
    if speech_level:
        cols += [(lambda r, c, n=n: r['speech_level'][n], _mean) for n in ('input', 'output', 'activity')]
    return cols


def metrics_rows(records, extended=False, peaks=False, loudness=False, true_peak=False, limiter=False, loudness_range=False, album=False, bandwidth=False,
                 stereo=False, speech_level=False):
    """records of enhance_folder -> the rows of --metrics_csv: one per written channel that has metrics, then the `mean` row
    (the plain mean of each column over the rows above, what the reference's eval_matric.py averages); no mean row when
    nothing was measured.  `extended`: the records carry 'metrics_ext' and a row has the columns of METRICS_COLUMNS_EXT; the
    mean of a column then runs over its entries that are not NaN (a clip too short for one segment has no segmental SNR).
    `peaks`: the records carry 'output' and a row ends with the columns of METRICS_COLUMNS_PEAKS -- the channel's peak in
    dBFS, its clipped samples and the file's gain; the mean row holds their plain means.  `loudness`: the records carry
    'loudness' and a row ends with the columns of METRICS_COLUMNS_LOUDNESS -- the file's integrated loudness going in and as
    written, in LUFS, and the gain between the generated and the written clip in dB; plain means again.  `true_peak`: the records' 'output'
    carries the true peak and a row ends with the column of METRICS_COLUMNS_TRUE_PEAK -- the channel's true peak in dBTP, like
    peak_dbfs measured on the clip in front of the guard's gain; its plain mean.  `limiter`: the records' 'output' carries 'limiter'
    and a row ends with the columns of METRICS_COLUMNS_LIMITER -- the file's largest reduction in dB and its number of reduced samples;
    plain means.  `loudness_range`: the records' 'loudness' carries 'range' and the columns of METRICS_COLUMNS_LOUDNESS_RANGE stand
    behind the loudness columns -- the file's loudness range going in and as the loudness stage leaves it, in LU, and its maximum
    short-term loudness in LUFS; plain means (a file under 3 s counts with 0.0 and -inf).  `album` (with `loudness`): the records
    carry 'album' (loudness_scope='folder') and one row `album` stands behind `mean`: the folder's loudness going in and as written
    and the one gain in the loudness columns, every other cell empty; the files' rows keep the tracks' own figures.  `bandwidth`:
    the records carry 'bandwidth' and a row ends, behind every other column, with the columns of METRICS_COLUMNS_BANDWIDTH -- where
    the band of the file's input, of its generated clip and of its original ends, in Hz (the file's figures, the same in each of its
    channels' rows); plain means.  `stereo`: the records carry 'stereo' and a row ends, behind those too, with the columns of
    METRICS_COLUMNS_STEREO -- the generated clip's correlation below and above the split, the original's above it and the generated
    clip's side level above it in dB (the file's figures; nan where the file has no stereo image or no such figure); means over
    the rows that have one.  `speech_level`: the records carry 'speech_level' and a row ends, behind every other column, with the
    columns of METRICS_COLUMNS_SPEECH_LEVEL -- the file's active speech level going in and as written, in dBov, and the written
    clip's activity factor; plain means (a file without activity counts with -inf and 0)."""
    if speech_level:
        cols = _columns(extended, peaks, loudness, true_peak, limiter, loudness_range, bandwidth, stereo, speech_level)
    elif stereo:
        cols = _columns(extended, peaks, loudness, true_peak, limiter, loudness_range, bandwidth, stereo)
    elif bandwidth:
        cols = _columns(extended, peaks, loudness, true_peak, limiter, loudness_range, bandwidth)
    elif loudness_range:
        cols = _columns(extended, peaks, loudness, true_peak, limiter, loudness_range)
    elif limiter:
        cols = _columns(extended, peaks, loudness, true_peak, limiter)
    else:
        cols = _columns(extended, peaks, loudness, true_peak) if true_peak else _columns(extended, peaks, loudness)
    rows = [(r['path'], c, r['out_frames']) + tuple(value(r, c) for value, _ in cols)
            for r in records for c in range(len(r['metrics_ext' if extended else 'metrics'] or ()))]
    if rows:
        rows.append(("mean", "", "") + tuple(mean([row[3 + k] for row in rows]) for k, (_, mean) in enumerate(cols)))
    whole = next((r['album'] for r in records if r.get('album') is not None), None) if album and loudness else None
    if whole is not None:
        first = len(_columns(extended, peaks))                             # the loudness columns stand behind these
        cells = [""] * len(cols)
        cells[first:first + 3] = [whole['input'], whole['output'], whole['gain_db']]
        rows.append(("album", "", "") + tuple(cells))
    return rows


def write_metrics_csv(path, records, extended=False, peaks=False, loudness=False, true_peak=False, limiter=False, loudness_range=False, album=False,
                      bandwidth=False, stereo=False, speech_level=False):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow((METRICS_COLUMNS_EXT if extended else METRICS_COLUMNS) + (METRICS_COLUMNS_PEAKS if peaks else ())
                   + (METRICS_COLUMNS_LOUDNESS if loudness else ()) + (METRICS_COLUMNS_LOUDNESS_RANGE if loudness_range else ())
                   + (METRICS_COLUMNS_TRUE_PEAK if true_peak else ())
                   + (METRICS_COLUMNS_LIMITER if limiter else ()) + (METRICS_COLUMNS_BANDWIDTH if bandwidth else ())
                   + (METRICS_COLUMNS_STEREO if stereo else ()) + (METRICS_COLUMNS_SPEECH_LEVEL if speech_level else ()))
        extra = dict({'loudness': True} if loudness else {}, **({'true_peak': True} if true_peak else {}))
        if limiter:
            extra['limiter'] = True
        if loudness_range:
            extra['loudness_range'] = True
        if album:
            extra['album'] = True
        if bandwidth:
            extra['bandwidth'] = True
        if stereo:
            extra['stereo'] = True
        if speech_level:
            extra['speech_level'] = True
        for row in metrics_rows(records, extended, peaks, **extra):
            w.writerow([repr(v) if isinstance(v, float) else v for v in row])


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
    true_peak = ', true peak %s dBTP' % ' '.join('%+.2f' % v for v in o['true_peak_dbtp']) if 'true_peak_dbtp' in o else ''
    print('%s: peak %s dBFS%s, %d clipped, %d non-finite, gain %.6f' % (name, ' '.join('%+.2f' % v for v in o['peak_dbfs']), true_peak,
                                                                      sum(o['clipped']), sum(o['nonfinite']), o['gain']))


def _print_loudness(name, l):
    print('%s: loudness input %+.2f LUFS, output %+.2f LUFS, gain %+.2f dB' % (name, l['input'], l['output'], l['gain_db']))


def _print_speech_level(name, s):
    print('%s: speech level input %+.2f dBov (activity %.1f %%), measured %+.2f dBov (activity %.1f %%), gain %+.2f dB -> %+.2f dBov'
          % (name, s['input'], 100.0 * s['activity_input'], s['measured'], 100.0 * s['activity'], s['gain_db'], s['output']))


def _print_album(a):
    print('album: loudness input %+.2f LUFS, measured %+.2f LUFS, gain %+.2f dB -> %+.2f LUFS (%d files, %d blocks)'
          % (a['input'], a['measured'], a['gain_db'], a['output'], a['files'], a['blocks_out']))


def _print_loudness_range(name, r):
    print('%s: loudness range input %.2f LU, output %.2f LU (%+.2f .. %+.2f LUFS), short-term max %+.2f LUFS'
          % (name, r['input'], r['output'], r['low'], r['high'], r['short_term_max']))


def _print_unwritten(name, available, written):
    if written < available:
        print('%s: %d of %d channels enhanced and written (--channels all writes every channel)' % (name, written, available))


def _print_limiter(l, frames):
    print('limiter: %+.2f dB at most, %.1f %% of the samples, true peak in %+.2f dBTP'
          % (l['max_reduction_db'], 100.0 * l['limited_samples'] / max(frames, 1), l['input_true_peak_dbtp']))


def _print_bandwidth(name, b):
    original = '' if b['original'] is None else ', original %.2f kHz' % (b['original'] / 1000.0)
    print("%s: bandwidth input %.2f kHz, output %.2f kHz%s (-%g dB, low rate's Nyquist %.2f kHz)"
          % (name, b['input'] / 1000.0, b['output'] / 1000.0, original, b['threshold_db'], b['lr_nyquist'] / 1000.0))
    for note in b['notes']:
        print('%s: note: %s' % (name, note))


def _print_crossover(x):
    print('crossover: %.2f kHz, %d taps (input band ends at %.2f kHz)' % (x['hz'] / 1000.0, x['taps'], x['edge_hz'] / 1000.0))


def _corr(f):
    return 'n/a' if f is None else '%+.2f' % f


def _print_stereo(name, s):
    clips = [(k, s[k]) for k in ('input', 'output', 'original') if s[k] is not None]
    print('%s: stereo correlation below / above %.2f kHz: %s'
          % (name, s['split_hz'] / 1000.0, ', '.join('%s %s / %s' % (k, _corr(f['low']['corr']), _corr(f['high']['corr'])) for k, f in clips)))
    for note in s['notes']:
        print('%s: note: %s' % (name, note))
