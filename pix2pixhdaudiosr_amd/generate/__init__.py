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

With the default `norm_scope='group'` a group is semantics: `to_spectro` normalises by the min / max of the whole batch tensor
(pix2pixHD_model.py:165-168 of the reference), so a group holds exactly the segments the reference's loader would put in it and a
last, smaller group runs at its own size -- padding it with silent segments would change its normalisation.  For the same reason
a channel of a file is a clip of its own: a group never mixes channels, and channel c of a [C, L] clip is grouped exactly as the
mono clip audio[c].

`--norm_scope clip` (opt-in, `SuperResolver(norm_scope='clip')`; csrc/spectro.hip) takes the semantics out of the group: a clip is
normalised by one range, the minimum and maximum of the dB spectrogram over all of its segments, found on the device in a pass in
front of its first group and read there by every group's encode (`model.clip_norm`, `model.inference(..., norm=)`).  The written
file then no longer depends on `--batchSize` beyond what the generator itself does with its batch, and a stretch of digital
silence one group long -- a lead-in, a gap, the side signal of a dual-mono file -- is written as silence where the group's own
range, max == min, writes NaN.  A channel is still a clip of its own, and a last, smaller group still runs at its own size.

`--segment_norm` (opt-in, `SuperResolver(segment_norm=True)`; csrc/spectro.hip, launch family "normrows") is the third way: one
range per segment, what 'group' means at batch 1, at any batch.  The encode takes every row's own statistics on the device
(`model.inference(..., norm='rows')`, `p2phd_spectro_encode_rows`) and `util.imdct` decodes every row under its own
(`p2phd_spectro_decode_signed_rows`, `_spliced_rows`), so the rows of a group no longer know of one another: the C * S rows of a
clip are walked in groups of `batch` without regard to channel (`group_rows_plan`), the last group is filled up with rows of
zeros -- a zero row has a range of zero, encodes as zeros, and its output is dropped -- and every group, of every clip, replays
the one captured graph.  No pre-pass, no held noise; a silent segment is written as silence.  Not with `norm_scope='clip'`.

`--pack_files N` (opt-in, an option of folder mode with `--segment_norm`; `enhance_folder(pack_files=N)`, `enhance_lr_many`) lets up to
N consecutive files of a folder share those groups: the rows of all their channels are gathered in one launch
(`segments_gather_ragged`, csrc/stitch.hip), walked as one clip's would be -- full groups, fillers in the last one only -- and stitched
back in one launch (`segments_stitch_ragged`), so sixteen utterances of 6 rows run 3 groups of 32 and not 16.  Everything in front of
and behind the rows stays per file; a file's rows, ranges and, with a seed, mask noise are those of a run of its own (`pack_plan`).

`--stream_seconds W` (opt-in, an option of `--segment_norm`; `enhance_file(stream_seconds=W)`, generate/stream.py) sends a file through
in windows of about W seconds -- whole segments, whole groups (`stream_plan`) -- each read, generated, stitched with the carry of the
window before (`segments_stitch_stream`, csrc/stitch.hip), encoded and appended to the output while the next one is read: memory is
a window's whatever the file's length, and the file is the unstreamed one byte for byte where the model draws no mask noise.  What
needs the whole clip or a figure of the whole file is refused with it (`check_stream`).

The two ends of the file path run on the device as well (csrc/pcm.hip): the data chunk of the input goes up as bytes and is
decoded there, the output is encoded there and comes back as the payload to write; the host only moves bytes.

The output stage is opt-in and on the device too: `--report_peaks` (peak, clipped and non-finite samples per channel),
`--clip guard [--ceiling_dbfs X]` (one gain for the whole file so that nothing clips), `--clip error` (refuse to write a
file that would clip) and `--dither tpdf` (PCM16).  Without them every byte written and every line printed is as before:
the integer encodings clamp, silently.  `--dither shaped` (csrc/shaper.hip; PCM16 written at 44100 or 48000 Hz) puts the same noise
in front of an error-feedback quantiser that moves the 16-bit floor out of 2-5 kHz and up above 15 kHz (`--dither_curve`,
`--dither_chunk`: the recursion starts again every chunk, which is what lets it run in parallel; `shaper_coefficients`).

`--crossover input` (opt-in, csrc/xover.hip) puts a time-domain crossover behind the stitch: a linear-phase complementary
filter pair, so that below `--crossover_hz` (default: 0.95 of the low rate's Nyquist frequency) the written clip is the input
and above it the generator's output.

`--spectrogram PATH` (opt-in, csrc/specimg.hip) also leaves a picture: the spectrograms of the input the generator was given,
of the written clip and -- for a full-band input -- of the original, stacked on one time, frequency and dB scale, rendered
on the device from the clips that are there at the end of enhance_file (`spectrogram_image`, `stft_db`, `spectrogram_rgb`).

`--loudness report|input|LUFS` (opt-in, csrc/loudness.hip) measures the integrated loudness after ITU-R BS.1770-4 / EBU R 128 of
the input the generator was given and of the generated clip on the device -- the level the pipeline writes depends on the
checkpoint's rates, the transform and the overlap -- and, with `input` or a target such as -23, multiplies the clip by the one
gain that brings it there, in front of the output stage (`loudness_hops`, `loudness_gate`, `loudness`).  `--loudness_range`, an
option of it, adds the other two programme descriptors of R 128 from the same hop energies: the loudness range after EBU Tech
3342 of both clips and the maximum short-term (3 s) loudness of the generated one, as the loudness stage leaves it
(`loudness_short_term`, `loudness_range`).  `--loudness_scope folder`, another option of it and of folder mode, treats the folder as
one programme, as EBU R 128 normalises an album: both gates over the 400 ms blocks of all files, one loudness gain and one guard
gain for all of them, every file measured before the first is written (generate/album.py; `loudness_blocks`, `loudness_gate_blocks`).

`--true_peak` (opt-in, csrc/truepeak.hip) measures the true peak after ITU-R BS.1770-4 Annex 2 on the device -- the clip the
encoder sees, oversampled to at least 192 kHz -- and reports it in dBTP; `--clip guard` then holds the true peak, not the sample
peak, at `--ceiling_dbfs`, and `--clip error` refuses a file whose true peak exceeds the encoding's limit (`true_peaks`,
`true_peak_coefficients`).

`--limiter` (opt-in, with `--clip guard`; csrc/limiter.hip) puts a look-ahead true-peak limiter in front of the guard: one gain
curve for all channels turns down the crests that stand over `--ceiling_dbfs` and nothing else, so a file brought to a loudness
target stays there where the guard's one gain would give the excess away (`limit`, `limiter_envelope`, `limiter_apply`,
`limiter_window`).

`--bandwidth` (opt-in, csrc/bandwidth.hip) reports where the band of each clip a file leaves actually ends -- of the input the
generator was given, of the generated clip and, for a full-band input, of the original: the highest bin of the long-term average
spectrum that still stands within `--bandwidth_threshold_db` (60) of the strongest band, found on the device, with a remark where
the input stops short of the low rate's Nyquist frequency or the original carries nothing above it (`ltas`, `bandwidth_detect`,
`bandwidth`).  `--crossover_hz auto` uses the same measurement per clip: the crossover keeps of the input only the band the input has.

`--stereo_report` (opt-in, csrc/stereo.hip) reports how the two channels of a file written with two channels correlate below and
above the low rate's Nyquist frequency -- for the input the generator was given, the generated clip and the original -- from the
long-term cross-spectrum of the pair, with a remark where the generated clip's new band has lost the correlation of its low band
(`cross_spectrum`, `stereo_bands`, `stereo_image`, `stereo_figures`).  `--stereo ms` (`SuperResolver(stereo='ms')`) is the remedy:
mid and side are generated instead of left and right, so what the channels share is invented once (`stereo_matrix`).

`--output_rate HZ` (opt-in, csrc/rateconv.hip) writes the file at another rate than the checkpoint's, 44100 for instance: a rational
polyphase converter (a Kaiser-windowed sinc, flat to 0.907 of the lower Nyquist frequency, 120 dB down where anything folds) sits in
front of the loudness, true-peak and limiter stages, which then measure and hold what is actually delivered (`rate_convert`,
`rateconv_plan`, `rateconv_coefficients`).

A FLAC input (told by its first bytes; csrc/flac.hip, data/flacio.py) is read as it stands: the file's bytes and its frame index, built
and CRC-checked on the host, are copied once and decoded on the device, one lane per FLAC frame (`flac_decode`, beside `pcm_decode`).
Folder mode lists *.flac only with `--input_formats wav,flac` (`plan_folder(..., formats=)`; x.flac is written as x.wav), and
`--verify_input` checks every FLAC file's MD5 on the host first.

A wav whose data chunk is coded -- G.711 mu-law or A-law, 4-bit IMA ADPCM: telephone archives -- is read as it stands too
(csrc/wavcodec.hip, data/wavio.py): the chunk's bytes are copied once and one launch of the family "wavcodec" decodes them to exactly
the samples of the file's PCM16 twin (`g711_decode`, `ima_decode`, beside `pcm_decode`); an IMA block header with a step index above
88 is refused on the host, naming file and block, before the copy.  No flag: a `.wav` is a `.wav`.

An AIFF / AIFF-C, Sun/NeXT AU or NIST SPHERE input (told by its first bytes -- 'FORM', '.snd', 'NIST' -- whatever its name: a TIMIT
`.WAV` is a SPHERE file; data/containers.py) is read as it stands as well: the sound data is copied once and one launch decodes it to
exactly the samples of the file's WAV twin -- `pcm_decode(..., big_endian=, signed8=)` for big-endian or signed 8-bit samples
(p2phd_pcm_decode_ex in csrc/pcm.hip), plain `pcm_decode` for little-endian ones (AIFF-C 'sowt', SPHERE byte format 01), `g711_decode`
for mu-law and A-law; the result's 'info' is a containers.AudioInfo, which leads with WavInfo's fields.  What is not read (AIFF-C ima4,
MACE, G.722, GSM; AU's G.72x codes; shorten-coded SPHERE; a non-integer sample rate) is a ValueError that names the file and the
coding before anything is launched, and a skipped file in folder mode.  Folder mode lists such files only with `--input_formats`
(aif, aiff, aifc, au, snd, sph; x.aif is written as x.wav).

`--container flac` (opt-in, csrc/flacenc.hip) writes a FLAC stream instead of a wav: the payload `pcm_encode` leaves on the device goes
through `flac_encode` there -- one workgroup per frame, fixed predictors, Rice partitions and the stereo assignments chosen on exact
bit counts -- and the file, decoded, is the wav's data chunk byte for byte.  `--flac_lpc N` also tries LPC subframes of every order
up to N (a predictor fitted per block, still chosen on exact bit counts; the file is never longer), `--flac_block N` sets the frame length, `--flac_md5`
brings the payload back as well and writes its MD5; a folder's outputs are then named .flac (`plan_folder(..., ext=)`).

`--speech_level report|input|DBOV` (opt-in, csrc/speechlevel.hip) measures the active speech level after ITU-T P.56 method B -- the
level while somebody is speaking, in dBov, with its activity factor -- of the same two clips, per channel, and brings the written
clip to the input's level or to a level such as -26 with one gain for all channels, where the loudness gain would sit
(`speech_level_envelope`, `speech_level_counts`, `speech_level_decide`, `speech_level`).  It excludes `--loudness`: one gain, one claim.
"""
from .cli import _parser, _run, main, opt_from_file, parse_opt_file                                        # noqa: F401
from .ops import (PCM_FORMATS, G711_LAWS, g711_decode, ima_decode, flac_decode, flac_encode, rate_convert, rateconv_coefficients, rateconv_out_len, rateconv_plan, bandwidth, bandwidth_detect, cross_spectrum, ltas, stereo_bands, stereo_image, stereo_matrix, crossover, crossover_coefficients, limit, limiter_apply, limiter_envelope, limiter_window, loudness, loudness_blocks, loudness_coefficients, loudness_gate,  # noqa: F401
                  loudness_gate_blocks, loudness_hops, loudness_range, loudness_short_term, pcm_decode, pcm_encode, pcm_peaks, shaper_coefficients, segments_gather, segments_gather_planar, segments_gather_ragged, segments_stitch,
                  segments_stitch_planar, segments_stitch_ragged, segments_stitch_stream, spectrogram_rgb, stft_db, true_peak_coefficients, true_peaks,
                  speech_level, speech_level_consts, speech_level_counts, speech_level_decide, speech_level_envelope)
from .plans import (check_stream, resample_geometry, resample_out_len, stream_plan, INPUT_FORMATS, check_input_formats, NORM_SCOPES, check_norm_scope, check_segment_norm, group_rows_plan, PACK_MAX_BYTES, check_pack_files, pack_plan, OUTPUT_MIN_RATE, RATECONV_DEFAULTS, check_output_rate, ALBUM_CACHE_BYTES, BANDWIDTH_DEFAULTS, STEREO_DEFAULTS, STEREO_MODES, STEREO_NOTE_DROP, check_stereo, check_stereo_report, stereo_figures, stereo_notes, stereo_split_bin, CROSSOVER_AUTO, bandwidth_notes, bandwidth_rel, check_bandwidth, crossover_auto_floor_hz, crossover_auto_plan, CLIP_MODES, CROSSOVER_ATTEN_DB, CROSSOVER_BETA, CROSSOVER_MAX_TAPS, CROSSOVERS, DITHERS, DITHER_CHUNK, DITHER_CURVES, SHAPED_RATES, dither_line,  # noqa: F401
                    LIMITER_HOLD_MS, LIMITER_LOOKAHEAD_MS, LIMITER_MAX_HOLD, LIMITER_MAX_LOOKAHEAD, LOUDNESS_MAX_CHANNELS, LOUDNESS_MAX_GAIN_DB, LOUDNESS_MODES, LOUDNESS_SCOPES, LOWBANDS,
                    PCM_ENCODINGS, SPECTROGRAM_DEFAULTS, SPECTROGRAM_LUT_ANCHORS, TRUEPEAK_BETA, TRUEPEAK_TAPS_PER_PHASE, ClipError, ceiling_from_dbfs, check_crossover,
                    check_dither, check_encoding, check_limiter, check_loudness, check_loudness_rate, check_loudness_scope, check_lowband, check_output_options, check_paths,
                    check_spectrogram, check_true_peak, crossover_plan, crossover_width_hz, encoding_limit, limiter_plan, loudness_channel_weights, plan_folder,
                    segment_plan, select_channels, spectro_bins, spectrogram_lut, truepeak_plan,
                    SPEECH_LEVEL_DEFAULTS, SPEECH_LEVEL_MODES, check_speech_level, check_speech_level_rate)
from .report import (METRICS_COLUMNS, METRICS_COLUMNS_BANDWIDTH, METRICS_COLUMNS_EXT, METRICS_COLUMNS_LIMITER, METRICS_COLUMNS_LOUDNESS, METRICS_COLUMNS_LOUDNESS_RANGE, METRICS_COLUMNS_PEAKS,  # noqa: F401
                     METRICS_COLUMNS_SPEECH_LEVEL, METRICS_COLUMNS_STEREO, METRICS_COLUMNS_TRUE_PEAK, metrics_rows, write_metrics_csv)
from .resolver import SuperResolver, spectrogram_image                                                                              # noqa: F401
