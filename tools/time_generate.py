#!/usr/bin/env python3
"""Whole-file generation at the published geometry, timed: G3L2, ngf 48, n_fft 512 (MDCT2), segments of 32 512 samples,
bf16, groups of 4, a 15 s synthetic 48 kHz clip, untrained weights.

  hand      the hand-composed loop (seg_pad_audio -> model.inference -> util.imdct per group -> cat)
  eager     generate.SuperResolver(graph=False), overlap 0 and 0.25
  graphed   generate.SuperResolver(graph=True), overlap 0 and 0.25
  seams     RMS of the first difference at the joins (the first sample of every segment but the first) relative to the
            first-difference RMS of the whole output, at overlap 0 and 0.25, same weights and noise seed

  flac      (only when asked for) the input side on one 15 s mono 16-bit clip, the same samples as FLAC (encoded by tests/_flac_ref.py:
            block size 4096, FIXED 2 and LPC 8 subframes in turn) and as wav: SuperResolver._read + _decode on the FLAC (index on the
            host, csrc/flac.hip on the device), on the wav (read_payload, copy, p2phd_pcm_decode) and the host decoder followed by a
            copy, interleaved, median and spread of --reps; then by events p2phd_flac_decode whole and each kernel alone beside
            p2phd_pcm_decode, on the clip and on an hour of it; the host index and host decoder alone; log in --flac_log
  flacout   (only when asked for) the output side: enhance_file with container wav / flac / flac with flac_md5 on one 15 s mono and one
            stereo clip, interleaved, median and spread of --reps; then by events p2phd_flac_encode beside p2phd_pcm_encode_ex on the
            written payloads, on the clip and on an hour of it; the host encoder alone; the streams' sizes; log in --flacout_log;
            with --flac_lpc N instead: container flac with flac_lpc=N against without, p2phd_flac_encode_lpc beside p2phd_flac_encode by
            events on the clip and on the hour, the frame kernel's two instantiations alone, the sizes at M = 0, 4, 8, 12; log in --flaclpc_log
  wavcodec  (only when asked for) coded WAV input: one 15 s mono 8 kHz clip as G.711 mu-law, A-law and IMA ADPCM (written by
            tests/_wavcodec_ref.py), each beside its PCM16 twin: enhance_file(is_lr_input) and _read + _decode alone, interleaved, median
            and spread of --reps; then by events the two kernels of csrc/wavcodec.hip beside p2phd_pcm_decode, on the clip and on an hour
            of it; the host entries on one thread; log in --wavcodec_log
  containers  (only when asked for) AIFF, AU and NIST SPHERE input: one 15 s mono clip as AIFF 16-bit and SPHERE pcm at 48 kHz and as AU
            mu-law at 8 kHz (written by tests/_containers_ref.py), each beside its WAV twin: enhance_file and _read + _decode alone,
            interleaved, median and range of --reps; then by events p2phd_pcm_decode_ex (big-endian) at S16 / S24 / F32 beside
            p2phd_pcm_decode on the byte-swapped twin, on the clip and on an hour of it; log in --containers_log

  folder    (only when asked for) a folder of identical 15 s stereo PCM16 clips, end to end from the files to the files, two
            ways in one process: the host-codec loop over channel-files (wavio.load -> enhance_lr -> wavio.save per mono
            file, what the package did before the device codec) and generate.SuperResolver.enhance_folder(channels='all')
            on the stereo files; --reps repeats each, best and spread; log in --folder_log

  lowband   (only when asked for) generate.SuperResolver(lowband='model') against lowband='input' (fade 0 and 8 rows), graphed,
            overlap 0.25: seconds of audio per second, best of --reps with the spread, and lsd_lf / lsd_hf of each output against
            a full-band original whose low-rate round trip is the input; log in --lowband_log

  crossover (only when asked for) generate.SuperResolver(crossover=None) against crossover='input' (the default plan), geometry, clip
            and repeats of `lowband`: seconds of audio per second, best of --reps with the spread, and lsd_lf / lsd_hf of each
            output against the full-band original, and the energy of the two outputs' difference below the transition band and
            above the low rate's Nyquist frequency; log in --crossover_log

  spectrogram (only when asked for) generate.SuperResolver.enhance_file on one 15 s mono PCM16 clip with a full-band original, file to
            file, without and with spectrogram=PATH (the default plan: three panels of 1600 x 512) in one process, the runs
            interleaved: milliseconds per file, median and spread of --reps, and how the option's share splits into the two
            kernels (timed alone, by events) and the rest (the copy back and the PNG encoder on the host); log in
            --spectrogram_log

  loudness  (only when asked for) generate.SuperResolver.enhance_file on that clip, file to file, without the option and with
            loudness='report' and loudness=-23 in one process, the runs interleaved: milliseconds per file, median and spread of
            --reps, and the two kernels alone (hop energies, gate) by events on the clips of the last run; log in --loudness_log.
            With --loudness_range the third variant is loudness='report', loudness_range=True, and the short-term and the range
            kernel are timed alone beside the gate, on the clip's hop energies and on an hour's worth; log in --loudness_range_log

  truepeak  (only when asked for) generate.SuperResolver.enhance_file on that clip, file to file, without the option and with
            true_peak=True, clip='guard' in one process, the runs interleaved: milliseconds per file, median and spread of --reps,
            and p2phd_truepeak beside p2phd_pcm_peak alone, by events, on the clip of the last run; log in --truepeak_log

  limiter   (only when asked for) generate.SuperResolver.enhance_file on that clip, file to file, brought to a loudness target that
            leaves its true peak 4 dB over a -1 dBTP ceiling: without any option, with the guard alone and with limiter=True in one
            process, the runs interleaved: milliseconds per file, median and spread of --reps; the loudness of the two written
            files, the residual overshoot (the limited clip's true peak over the ceiling in front of the guard's residual gain),
            and the two kernels beside p2phd_truepeak alone, by events, on the clip of the last run; log in --limiter_log

  album     (only when asked for) generate.SuperResolver.enhance_folder(channels='all') on a folder of --files stereo PCM16 clips of
            --seconds each at different levels, files to files, in one process, the runs interleaved (nine repeats unless --reps says
            otherwise): without loudness, loudness=-23 at loudness_scope 'file', at scope 'folder', and at scope 'folder' with
            album_cache_bytes=0 (every generated clip waits on the host): milliseconds per folder, median and spread, and what
            the scope costs over scope 'file'; then p2phd_loudness_blocks and p2phd_loudness_gate_blocks alone, by events, beside
            p2phd_loudness_gate on the same hop energies, at the folder's block count and at 36 000 blocks; log in --album_log

  bandwidth (only when asked for) generate.SuperResolver.enhance_file on that clip, file to file, without the option and with
            bandwidth=True in one process, the runs interleaved (nine repeats unless --reps says otherwise): milliseconds per file,
            median and spread; then crossover='input' with the fixed crossover against crossover_hz='auto' likewise (the wait for
            the measurement's event shows there); then p2phd_ltas and p2phd_bandwidth alone, by events, at the clip's frame count
            and at an hour's; with --off_only only the run without any option is timed (one process of an alternating comparison
            with another checkout); log in --bandwidth_log

  stereo    (only when asked for) enhance_file on a two-channel clip of that length (a shared part and a part of each channel's own),
            channels='all', file to file: without any option, with stereo_report=True and with SuperResolver(stereo='ms'), in one
            process, the runs interleaved (nine repeats unless --reps says otherwise): milliseconds per file, median and spread;
            then p2phd_xspec and p2phd_stereo_bands alone, by events, beside p2phd_ltas on the same two rows (the same number of
            transforms), at the clip's frame count and at an hour's, and p2phd_stereo_matrix on the clip; with --off_only only the
            run without any option is timed (one process of an alternating comparison with another checkout); log in --stereo_log

  normscope (only when asked for) enhance_file on a mono clip of that length, file to file: SuperResolver as ever (norm_scope 'group')
            against SuperResolver(norm_scope='clip'), in one process, the runs interleaved (nine repeats unless --reps says
            otherwise): milliseconds per file, median and spread; then p2phd_spectro_range, p2phd_range_fold and
            p2phd_spectro_encode_given alone, by events, on one group's spectrum and noise, beside p2phd_spectro_encode_ex on the same
            tensors; with --off_only only the run without the option is timed (one process of an alternating comparison with another
            checkout); log in --normscope_log

  segnorm   (only when asked for) file to file, SuperResolver as ever (norm_scope 'group'), SuperResolver(norm_scope='clip') and
            SuperResolver(segment_norm=True), in one process, the runs interleaved (nine repeats unless --reps says otherwise):
            enhance_file on a mono clip of that length, then enhance_folder on eight two-channel clips of 2 s, where the eager last
            groups of the first two would dominate, and of 1.5 s, where they do: milliseconds, median and spread; then p2phd_spectro_encode_rows beside
            p2phd_spectro_encode_ex and p2phd_spectro_encode_given, and p2phd_spectro_decode_signed_rows beside
            p2phd_spectro_decode_signed, alone, by events, on one group's spectrum and noise (the option-off path against another
            checkout: normscope --off_only in either); log in --segnorm_log

  pack      (only when asked for) files to files with SuperResolver(segment_norm=True) at groups of 32, graphed: enhance_folder on 32 mono
            clips of 3 s with pack_files 1, 4, 16 and 32, in one process, the runs interleaved (nine repeats unless --reps says
            otherwise): milliseconds per folder, median and spread, and the groups each walks; then the ragged gather and stitch
            alone, by events, beside the planar launches they replace on the same clips; with --off_only only pack_files 1 is timed
            (the option-off folder run against another checkout: segnorm in either, which both have); log in --pack_log

  dither    (only when asked for) enhance_file on a mono clip of that length, file to file: without any option, with dither='tpdf' and
            with dither='shaped' (lipshitz9, chunks of 4096), in one process, the runs interleaved (nine repeats unless --reps says
            otherwise): milliseconds per file, median and spread; then p2phd_pcm_encode_shaped alone, by events, at chunk 4096 and
            1024 beside p2phd_pcm_encode_ex with TPDF on the same row, at the clip's length and at an hour's, and once with one chunk
            for the whole clip -- the recursion as one sequential chain, the measured cost of not chunking; with --off_only only the
            run without any option is timed (one process of an alternating comparison with another checkout); log in --dither_log

Without a mode every one of the first four runs in a process of its own under its own time limit, in that order, and the run stops at
the first that fails; the lines are also written to --log.

Usage:  python tools/time_generate.py [hand|eager|graphed|seams] [--seconds 15] [--reps 5] [--log profiles/time_generate.log]
        python tools/time_generate.py folder [--files 8] [--folder_log profiles/time_generate_folder.log]
        python tools/time_generate.py lowband [--lowband_log profiles/time_generate_lowband.log]
        python tools/time_generate.py crossover [--crossover_log profiles/time_generate_crossover.log]
        python tools/time_generate.py spectrogram [--spectrogram_log profiles/time_generate_spectrogram.log]
        python tools/time_generate.py loudness [--loudness_log profiles/time_generate_loudness.log]
        python tools/time_generate.py loudness --loudness_range [--loudness_range_log profiles/time_generate_loudness_range.log]
        python tools/time_generate.py truepeak [--truepeak_log profiles/time_generate_truepeak.log]
        python tools/time_generate.py limiter [--limiter_log profiles/time_generate_limiter.log]
        python tools/time_generate.py album [--files 8] [--album_log profiles/time_generate_album.log]
        python tools/time_generate.py bandwidth [--off_only] [--bandwidth_log profiles/time_generate_bandwidth.log]
        python tools/time_generate.py stereo [--off_only] [--stereo_log profiles/time_generate_stereo.log]
        python tools/time_generate.py rateconv [--off_only] [--rateconv_log profiles/time_generate_rateconv.log]
        python tools/time_generate.py normscope [--off_only] [--normscope_log profiles/time_generate_norm_scope.log]
        python tools/time_generate.py segnorm [--segnorm_log profiles/time_generate_segment_norm.log]
        python tools/time_generate.py pack [--off_only] [--pack_log profiles/time_generate_pack.log]
        python tools/time_generate.py dither [--off_only] [--dither_log profiles/time_generate_dither.log]
        python tools/time_generate.py flacout [--flac_lpc 12] [--flacout_log profiles/time_generate_flacout.log] [--flaclpc_log profiles/time_generate_flaclpc.log]
        python tools/time_generate.py wavcodec [--wavcodec_log profiles/time_generate_wavcodec.log]
        python tools/time_generate.py containers [--containers_log profiles/time_generate_containers.log]
"""
import argparse
import os
import subprocess
import sys
import time
from math import sqrt
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"hand": 240, "eager": 300, "graphed": 300, "seams": 240}


def _opt():
    return SimpleNamespace(
        gpu_ids=[0], isTrain=False, checkpoints_dir=None, name="t", model="pix2pixHD", input_nc=2, output_nc=2,
        label_nc=0, hr_sampling_rate=48000, lr_sampling_rate=8000, n_fft=512, hop_length=256, win_length=512, center=True,
        no_instance=True, ngf=48, netG="local", n_downsample_global=4, n_blocks_global=3, n_local_enhancers=1, n_blocks_local=2,
        norm="instance", no_lsgan=False, ndf=64, n_layers_D=3, num_D=2, no_ganFeat_loss=False, use_hifigan_D=False, use_time_D=False,
        verbose=False, continue_train=False, load_pretrain="", which_epoch="latest", pool_size=0, lr=0.0002, beta1=0.5,
        no_vgg_loss=True, use_match_loss=False, niter_fix_global=0, explicit_encoding=True, alpha=0.6, min_value=1e-7, mask=True,
        mask_mode="mode2", phase_encoding_mode=None, lambda_feat=10.0, fp16=True, niter_decay=100, instance_feat=False,
        label_feat=False, mdct_type="mdct2", segment_length=32512, batchSize=4)


def _setup(seconds):
    import torch
    from pix2pixhdaudiosr_amd.models.models import create_model
    import copy
    import tempfile
    opt = _opt()
    torch.manual_seed(1234)
    with tempfile.TemporaryDirectory() as folder:                 # generation runs an inference model: it loads its generator
        opt.checkpoints_dir = folder
        seed_opt = copy.copy(opt)
        seed_opt.isTrain = True
        create_model(seed_opt).save('latest')                     # untrained weights, written once, outside every timed region
        torch.cuda.empty_cache()
        model = create_model(opt)
    model.eval()
    n = int(seconds * opt.hr_sampling_rate)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    g = torch.Generator().manual_seed(7)
    # a band-limited clip: a few partials below the low rate's 4 kHz with a slow envelope, and a little noise
    x = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.2, 220.0, 0.0), (0.1, 660.0, 1.0), (0.05, 1870.0, 2.0), (0.03, 3300.0, 0.5)))
    x = x * (0.6 + 0.4 * torch.sin(2 * torch.pi * 0.7 * t)) + 0.002 * torch.randn(n, generator=g, dtype=torch.float64)
    return torch, model, opt, x.float().cuda()[None]


def _hand(torch, model, opt, lr):
    from pix2pixhdaudiosr_amd.data.audio_dataset import AudioTestDataset
    from pix2pixhdaudiosr_amd.dct.dct import IDCT
    from pix2pixhdaudiosr_amd.models.mdct import IMDCT2
    from pix2pixhdaudiosr_amd.util import util as U
    ds = AudioTestDataset.__new__(AudioTestDataset)
    ds.segment_length = opt.segment_length
    _imdct = IMDCT2(window=U.kbdwin, win_length=opt.win_length, hop_length=opt.hop_length, n_fft=opt.n_fft, center=opt.center,
                    out_length=opt.segment_length, device='cuda', idct_op=IDCT())
    up = opt.hr_sampling_rate / opt.lr_sampling_rate

    def run():
        seg = ds.seg_pad_audio(lr)
        audio = []
        with torch.no_grad():
            for s0 in range(0, seg.shape[0], opt.batchSize):
                sr_spectro, lr_pha, norm_param, _ = model.inference(seg[s0:s0 + opt.batchSize], None)
                audio.append(U.imdct(spectro=sr_spectro.abs(), pha=lr_pha.squeeze(1), norm_param=norm_param, _imdct=_imdct,
                                     up_ratio=up, explicit_encoding=True))
        return sqrt(up - 1) * torch.cat(audio, dim=0).view(1, -1)
    return run


def _time(torch, fn, reps):
    fn(); fn()                                                     # warm-up (and capture, where there is one)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def run_folder(seconds, reps, files, log):
    """Seconds of audio per second, files to files.  Audio counted: files * 2 channels * seconds for either way."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.data.audio_dataset import lr_round_trip
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver(model, opt)
    rate = int(opt.hr_sampling_rate)
    stereo = torch.cat([x, -0.7 * x.flip(-1)]).cpu()
    audio = files * 2 * seconds
    lines = ["# tools/time_generate.py folder: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25; %d stereo "
             "PCM16 clips of %g s at 48 kHz (%g s of audio), files to files, %d repeats" % (files, seconds, audio, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        d_st, d_mono, d_out = (os.path.join(tmp, n) for n in ("stereo", "mono", "out"))
        for d in (d_st, d_mono, d_out):
            os.makedirs(d)
        for i in range(files):
            wavio.save(os.path.join(d_st, "clip%03d.wav" % i), stereo, rate)
            for c in range(2):
                wavio.save(os.path.join(d_mono, "clip%03d_%d.wav" % (i, c)), stereo[c:c + 1], rate)
        monos = sorted(os.listdir(d_mono))

        def host_loop():                                           # enhance_file as it was before the device codec, per channel-file
            for name in monos:
                raw, r = wavio.load(os.path.join(d_mono, name))
                raw = raw[:1].cuda()
                lr = lr_round_trip(raw, r, opt.lr_sampling_rate, opt.hr_sampling_rate)[..., :raw.shape[-1]]
                wavio.save(os.path.join(d_out, name), sr.enhance_lr(lr), rate)

        def folder():
            recs = sr.enhance_folder(d_st, d_out, channels='all')
            assert len(recs) == files and all(r['error'] is None and r['written_channels'] == 2 for r in recs)

        for name, fn in (("host-codec loop over %d channel-files" % (2 * files), host_loop), ("enhance_folder, %d stereo files      " % files, folder)):
            fn()                                                   # warm-up: capture, packed weights, pinned buffers, page cache
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            rates = sorted(audio / t for t in ts)
            lines.append("%s  best %8.1f s of audio / s   spread %6.1f (worst %8.1f)   runs: %s"
                         % (name, rates[-1], rates[-1] - rates[0], rates[0], " ".join("%.1f" % (audio / t) for t in ts)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write(text)


def run_lowband(seconds, reps, log):
    """Seconds of audio per second of the graphed pipeline at overlap 0.25 with the model's and with the input's low band, the
    runs of the variants interleaved so that a drift of the machine falls on all of them; and what each does to the two bands."""
    _run_variants(seconds, reps, log, "lowband",
                  [("lowband model          ", dict()), ("lowband input, fade 0  ", dict(lowband='input')),
                   ("lowband input, fade 8  ", dict(lowband='input', lowband_fade=8))])


def run_crossover(seconds, reps, log):
    """The same comparison for the time-domain crossover: off against 'input' with the default plan, interleaved."""
    _run_variants(seconds, reps, log, "crossover", [("crossover off         ", dict()), ("crossover input       ", dict(crossover='input'))])


def _median(v):
    v = sorted(v)
    return 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])


def run_spectrogram(seconds, reps, log):
    """enhance_file, file to file, without and with the spectrogram picture: the same object, the same input, interleaved."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SPECTROGRAM_DEFAULTS, SuperResolver, spectrogram_rgb, stft_db
    n = x.shape[-1]
    g = torch.Generator().manual_seed(8)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    hi = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.02, 5200.0, 0.3), (0.01, 9100.0, 1.1), (0.005, 15300.0, 2.2)))
    hr = x.cpu() + (hi + 0.001 * torch.randn(n, generator=g, dtype=torch.float64)).float()[None]      # as the low-band run's original
    sr = SuperResolver(model, opt, overlap=0.25)
    d = SPECTROGRAM_DEFAULTS
    lines = ["# tools/time_generate.py spectrogram: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz with a full-band original, file to file, untrained weights, %d interleaved repeats; "
             "picture: 3 panels of %d x %d, STFT %d / %d" % (seconds, reps, d['width'], d['height'], d['n_fft'], d['hop'])]
    with tempfile.TemporaryDirectory() as tmp:
        src, out, png = (os.path.join(tmp, f) for f in ("in.wav", "out.wav", "out.png"))
        wavio.save(src, hr, int(opt.hr_sampling_rate))
        variants = (("spectrogram off", {}), ("spectrogram on ", dict(spectrogram=png)))
        for _, kw in variants:                                     # warm-up: capture, tables, pinned buffers, page cache
            res = sr.enhance_file(src, out, **kw)
            sr.enhance_file(src, out, **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in variants]
        for _ in range(reps):
            for k, (_, kw) in enumerate(variants):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(variants, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        lines.append("the option costs %.3f ms per file (difference of the medians), %.2f %% of the file without it"
                     % (_median(ts[1]) - _median(ts[0]), 100.0 * (_median(ts[1]) - _median(ts[0])) / _median(ts[0])))
        # the two kernels alone, by events, on the clips of the last run
        rows = torch.stack([res['lr'][0], res['sr'][0], res['hr'][0]])
        db = stft_db(rows, d['n_fft'], d['hop'])
        top = db.amax().reshape(1)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        k_stft, k_render = [], []
        for _ in range(reps + 2):
            ev[0].record()
            db = stft_db(rows, d['n_fft'], d['hop'])
            ev[1].record()
            img = spectrogram_rgb(db, top, d['range_db'], d['width'], d['height'], d['gap'])
            ev[2].record()
            torch.cuda.synchronize()
            k_stft.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_render.append(ev[1].elapsed_time(ev[2]) * 1e3)
        plane, pixels = db.numel() * 4, img.numel()
        lines.append("kernels alone (events, median of %d): stft_db %.1f us (%d frames x %d bins x 3 rows: %.1f MB written, %.0f GB/s), "
                     "render %.1f us (%.1f MB read, %.1f MB of pixels)"
                     % (reps, _median(k_stft[2:]), db.shape[1], db.shape[2], plane / 1e6, plane / (_median(k_stft[2:]) * 1e-6) / 1e9,
                        _median(k_render[2:]), plane / 1e6, pixels / 1e6))
        from pix2pixhdaudiosr_amd.util import util as U
        host = img.cpu().numpy()
        enc = []
        for _ in range(3):
            t0 = time.perf_counter()
            U.save_image(host, png)
            enc.append((time.perf_counter() - t0) * 1e3)
        lines.append("util.save_image of the %d x %d picture on the host: %.3f ms (median of 3), %d bytes of PNG"
                     % (host.shape[1], host.shape[0], _median(enc), os.path.getsize(png)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write(text)


def _loudness_range_kernels(torch, z, rate, reps, what):
    """The short-term and the range kernel alone on hop energies z [C, J], and the gate kernel beside them, by events -> a line."""
    from pix2pixhdaudiosr_amd.generate import loudness_gate, loudness_range, loudness_short_term
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    k_short, k_range, k_gate = [], [], []
    for _ in range(reps + 2):
        ev[0].record()
        p = loudness_short_term(z, rate)
        ev[1].record()
        loudness_range(p)
        ev[2].record()
        loudness_gate(z, rate)
        ev[3].record()
        torch.cuda.synchronize()
        k_short.append(ev[0].elapsed_time(ev[1]) * 1e3)
        k_range.append(ev[1].elapsed_time(ev[2]) * 1e3)
        k_gate.append(ev[2].elapsed_time(ev[3]) * 1e3)
    return ("%s (events, median of %d): loudness_short_term %.1f us, loudness_range %.1f us (%d blocks: nine passes of one workgroup), "
            "loudness_gate beside them %.1f us (%d blocks: two passes); runs: short-term %s; range %s; gate %s"
            % (what, reps, _median(k_short[2:]), _median(k_range[2:]), p.numel(), _median(k_gate[2:]), max(z.shape[1] - 3, 0),
               " ".join("%.1f" % v for v in k_short[2:]), " ".join("%.1f" % v for v in k_range[2:]), " ".join("%.1f" % v for v in k_gate[2:])))


def run_loudness(seconds, reps, log, ranged=False):
    """enhance_file, file to file, without and with the loudness option: the same object, the same input, interleaved; then the two
    kernels alone.  `ranged`: the variants are off, loudness='report' and the same with loudness_range=True, and the kernels alone
    are the short-term and the range kernel, on the clip's hop energies and on an hour's worth (36 000 blocks)."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, loudness_gate, loudness_hops
    n = x.shape[-1]
    g = torch.Generator().manual_seed(8)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    hi = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.02, 5200.0, 0.3), (0.01, 9100.0, 1.1), (0.005, 15300.0, 2.2)))
    hr = x.cpu() + (hi + 0.001 * torch.randn(n, generator=g, dtype=torch.float64)).float()[None]      # as the spectrogram run's original
    sr = SuperResolver(model, opt, overlap=0.25)
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py loudness: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz with a full-band original, file to file, untrained weights, %d interleaved repeats" % (seconds, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, hr, rate)
        variants = (("loudness off   ", {}), ("loudness report", dict(loudness='report')), ("loudness -23   ", dict(loudness=-23.0)))
        if ranged:
            lines[0] = lines[0].replace("time_generate.py loudness:", "time_generate.py loudness --loudness_range:")
            variants = variants[:2] + (("report + range ", dict(loudness='report', loudness_range=True)),)
        for _, kw in variants:                                     # warm-up: capture, pinned buffers, page cache
            res = sr.enhance_file(src, out, **kw)
            sr.enhance_file(src, out, **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in variants]
        for _ in range(reps):
            for k, (_, kw) in enumerate(variants):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(variants, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        for k in (1, 2):
            lines.append("%s costs %.3f ms per file (difference of the medians), %.2f %% of the file without it"
                         % (variants[k][0].strip(), _median(ts[k]) - _median(ts[0]), 100.0 * (_median(ts[k]) - _median(ts[0])) / _median(ts[0])))
        lines.append("the last file: %s" % ", ".join("%s %s" % (k, ("%+.3f" % v) if v is not None else "none") for k, v in sorted(res['loudness'].items())
                                                     if k != 'range'))
        if ranged:
            lines.append("the range costs %.3f ms per file over loudness report (difference of the medians), %.2f %% of the file without either"
                         % (_median(ts[2]) - _median(ts[1]), 100.0 * (_median(ts[2]) - _median(ts[1])) / _median(ts[0])))
            lines.append("the last file's range: %s" % ", ".join("%s %+.3f" % kv for kv in sorted(res['loudness']['range'].items())))
        # the two kernels alone, by events, on the generated clip of the last run (one row of %d samples)
        clip = res['sr'].contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        k_hops, k_gate = [], []
        for _ in range(reps + 2):
            ev[0].record()
            z = loudness_hops(clip, rate)
            ev[1].record()
            loudness_gate(z, rate, target=-23.0)
            ev[2].record()
            torch.cuda.synchronize()
            k_hops.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_gate.append(ev[1].elapsed_time(ev[2]) * 1e3)
        hop = rate // 10
        steps = 3 * hop                                            # samples one work item walks: 200 ms of warm-up and its hop
        us = _median(k_hops[2:])
        lines.append("kernels alone (events, median of %d): loudness_hops %.1f us (%d hops of %d samples, %d workgroups of one wave, %d samples "
                     "walked per work item: %.1f ns per sample of the float64 recursion, %.2f ms of audio per us), loudness_gate %.1f us (%d blocks)"
                     % (reps, us, z.shape[1], hop, -(-z.shape[1] // 64), steps, us * 1e3 / steps, clip.shape[-1] / rate * 1e3 / us,
                        _median(k_gate[2:]), max(z.shape[1] - 3, 0)))
        lines.append("runs: loudness_hops %s; loudness_gate %s" % (" ".join("%.1f" % v for v in k_hops[2:]), " ".join("%.1f" % v for v in k_gate[2:])))
        if ranged:
            lines.append(_loudness_range_kernels(torch, z, rate, reps, "range kernels alone, the clip"))
            hour = torch.rand((1, 36029), dtype=torch.float64, device=z.device, generator=torch.Generator(z.device).manual_seed(9)) * hop
            lines.append(_loudness_range_kernels(torch, hour, rate, reps, "range kernels alone, an hour of hops"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write(text)


def _album_kernels(torch, NB, rate, reps, what):
    """loudness_blocks and loudness_gate_blocks alone on random hop energies of NB blocks, and loudness_gate on the same hop
    energies beside them, by events -> a line."""
    from pix2pixhdaudiosr_amd.generate import loudness_blocks, loudness_gate, loudness_gate_blocks
    z = torch.rand((1, NB + 3), dtype=torch.float64, device='cuda', generator=torch.Generator('cuda').manual_seed(9)) * (rate // 10)
    p = torch.empty((NB,), dtype=torch.float64, device='cuda')
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    k_blocks, k_album, k_gate = [], [], []
    for _ in range(reps + 2):
        ev[0].record()
        loudness_blocks(z, rate, out=p)
        ev[1].record()
        loudness_gate_blocks(p, target=-23.0)
        ev[2].record()
        loudness_gate(z, rate, target=-23.0)
        ev[3].record()
        torch.cuda.synchronize()
        k_blocks.append(ev[0].elapsed_time(ev[1]) * 1e3)
        k_album.append(ev[1].elapsed_time(ev[2]) * 1e3)
        k_gate.append(ev[2].elapsed_time(ev[3]) * 1e3)
    return ("%s, %d blocks (events, median of %d): loudness_blocks %.1f us (%d workgroups), loudness_gate_blocks %.1f us (one workgroup, "
            "two passes of %d steps per thread), loudness_gate on the same hops %.1f us; runs: blocks %s; gate_blocks %s; gate %s"
            % (what, NB, reps, _median(k_blocks[2:]), min(-(-NB // 256), 2048), _median(k_album[2:]), -(-NB // 256), _median(k_gate[2:]),
               " ".join("%.1f" % v for v in k_blocks[2:]), " ".join("%.1f" % v for v in k_album[2:]), " ".join("%.1f" % v for v in k_gate[2:])))


def run_album(seconds, reps, files, log):
    """enhance_folder, files to files, without loudness and with loudness=-23 at either scope: the same object, the same folder,
    interleaved; then the two album kernels alone."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver(model, opt, overlap=0.25)
    rate = int(opt.hr_sampling_rate)
    stereo = torch.cat([x, -0.7 * x.flip(-1)]).cpu()
    lines = ["# tools/time_generate.py album: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; a folder of "
             "%d stereo PCM16 clips of %g s at 48 kHz, file k at 0.85^k of the first, files to files, channels='all', untrained weights, %d "
             "interleaved repeats" % (files, seconds, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(src)
        for i in range(files):
            wavio.save(os.path.join(src, "clip%03d.wav" % i), stereo * 0.85 ** i, rate)
        variants = (("loudness off            ", {}), ("-23, scope file         ", dict(loudness=-23.0)),
                    ("-23, scope folder       ", dict(loudness=-23.0, loudness_scope='folder')),
                    ("-23, scope folder, no cache", dict(loudness=-23.0, loudness_scope='folder', album_cache_bytes=0)))
        last = {}
        for name, kw in variants:                                  # warm-up: capture, pinned buffers, page cache
            sr.enhance_folder(src, out, channels='all', **kw)
            last[name] = sr.enhance_folder(src, out, channels='all', **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in variants]
        for _ in range(reps):
            for k, (_, kw) in enumerate(variants):
                t0 = time.perf_counter()
                recs = sr.enhance_folder(src, out, channels='all', **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
                assert len(recs) == files and all(r['error'] is None and r['written_channels'] == 2 for r in recs)
        for (name, _), tk in zip(variants, ts):
            lines.append("%s  median %9.3f ms per folder   spread %7.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        lines.append("scope file costs %.3f ms per folder over no loudness (difference of the medians), %.2f %% of it"
                     % (_median(ts[1]) - _median(ts[0]), 100.0 * (_median(ts[1]) - _median(ts[0])) / _median(ts[0])))
        for k in (2, 3):
            lines.append("%s costs %.3f ms per folder over scope file (difference of the medians), %.2f %% of it"
                         % (variants[k][0].strip(), _median(ts[k]) - _median(ts[1]), 100.0 * (_median(ts[k]) - _median(ts[1])) / _median(ts[1])))
        album = last[variants[2][0]][0]['album']
        lines.append("the album: %s" % ", ".join("%s %s" % (k, ("%+.3f" % v) if isinstance(v, float) else v) for k, v in sorted(album.items())))
        lines.append("the per-file gains at scope file: %s dB" % " ".join("%+.2f" % r['loudness']['gain_db'] for r in last[variants[1][0]]))
        lines.append(_album_kernels(torch, album['blocks_out'], rate, reps, "kernels alone, the folder"))
        lines.append(_album_kernels(torch, 36000, rate, reps, "kernels alone, an hour of blocks"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write(text)


def run_truepeak(seconds, reps, log):
    """enhance_file, file to file, without the true-peak option and with it under clip='guard': the same object, the same input,
    interleaved; then the true-peak kernel and the sample-peak kernel alone on the same clip."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, pcm_peaks, true_peaks, truepeak_plan
    n = x.shape[-1]
    g = torch.Generator().manual_seed(8)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    hi = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.02, 5200.0, 0.3), (0.01, 9100.0, 1.1), (0.005, 15300.0, 2.2)))
    hr = x.cpu() + (hi + 0.001 * torch.randn(n, generator=g, dtype=torch.float64)).float()[None]      # as the spectrogram run's original
    sr = SuperResolver(model, opt, overlap=0.25)
    rate = int(opt.hr_sampling_rate)
    plan = truepeak_plan(rate)
    lines = ["# tools/time_generate.py truepeak: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz with a full-band original, file to file, untrained weights, %d interleaved repeats" % (seconds, reps),
             "# true-peak plan: factor %d, %d taps per phase, beta %g" % (plan['factor'], plan['taps_per_phase'], plan['beta'])]
    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, hr, rate)
        variants = (("true_peak off         ", {}), ("true_peak, clip guard ", dict(true_peak=True, clip='guard')))
        for _, kw in variants:                                     # warm-up: capture, pinned buffers, page cache
            res = sr.enhance_file(src, out, **kw)
            sr.enhance_file(src, out, **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in variants]
        for _ in range(reps):
            for k, (_, kw) in enumerate(variants):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(variants, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        lines.append("%s costs %.3f ms per file (difference of the medians), %.2f %% of the file without it; it holds the peak report and the "
                     "guard's gain in the encoder as well as the true-peak kernel"
                     % (variants[1][0].strip(), _median(ts[1]) - _median(ts[0]), 100.0 * (_median(ts[1]) - _median(ts[0])) / _median(ts[0])))
        o = res['output']
        lines.append("the last file: peak %+.3f dBFS, true peak %+.3f dBTP, gain %.6f" % (o['peak_dbfs'][0], o['true_peak_dbtp'][0], o['gain']))
        # the two kernels alone, by events, on the generated clip of the last run (one row)
        clip = res['sr'].contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        k_true, k_peak = [], []
        for _ in range(reps + 2):
            ev[0].record()
            true_peaks(clip, rate)
            ev[1].record()
            pcm_peaks(clip, 'pcm16')
            ev[2].record()
            torch.cuda.synchronize()
            k_true.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_peak.append(ev[1].elapsed_time(ev[2]) * 1e3)
        L = clip.shape[-1]
        us, us_peak = _median(k_true[2:]), _median(k_peak[2:])
        fmas = (plan['factor'] - 1) * plan['taps_per_phase']
        lines.append("kernels alone (events, median of %d, each with the allocation of its small result in front): p2phd_truepeak %.1f us (%d "
                     "samples, %d fma per sample: %.2f Gfma/s, %.2f GB/s of samples read), p2phd_pcm_peak %.1f us: %.1f times the sample-peak kernel"
                     % (reps, us, L, fmas, L * fmas / us * 1e-3, 4.0 * L / us * 1e-3, us_peak, us / us_peak))
        lines.append("runs: p2phd_truepeak %s; p2phd_pcm_peak %s" % (" ".join("%.1f" % v for v in k_true[2:]), " ".join("%.1f" % v for v in k_peak[2:])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write(text)


def run_bandwidth(seconds, reps, log, off_only=False):
    """enhance_file, file to file, without the bandwidth option and with it -- the same object, the same input, interleaved; the
    fixed crossover against crossover_hz='auto' likewise; then the two kernels alone at the clip's frame count and at an hour's."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    n = x.shape[-1]
    g = torch.Generator().manual_seed(8)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    hi = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.02, 5200.0, 0.3), (0.01, 9100.0, 1.1), (0.005, 15300.0, 2.2)))
    hr = x.cpu() + (hi + 0.001 * torch.randn(n, generator=g, dtype=torch.float64)).float()[None]      # as the spectrogram run's original
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py bandwidth: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz with a full-band original, file to file, untrained weights, %d interleaved repeats" % (seconds, reps)]

    def interleaved(runs, src, out):
        """runs: [(name, resolver, keyword arguments)] -> the milliseconds of every run, and the last result of each"""
        last = [None] * len(runs)
        for k, (_, sr, kw) in enumerate(runs):                      # warm-up: capture, pinned buffers, page cache
            sr.enhance_file(src, out, **kw)
            last[k] = sr.enhance_file(src, out, **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(reps):
            for k, (_, sr, kw) in enumerate(runs):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _, _), tk in zip(runs, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        return ts, last

    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, hr, rate)
        sr = SuperResolver(model, opt, overlap=0.25)
        if off_only:
            interleaved([("no option            ", sr, {})], src, out)
        else:
            ts, last = interleaved([("bandwidth off        ", sr, {}), ("bandwidth            ", sr, dict(bandwidth=True))], src, out)
            lines.append("bandwidth costs %.3f ms per file (difference of the medians), %.2f %% of the file without it: six launches and 96 bytes "
                         "more in the copy back" % (_median(ts[1]) - _median(ts[0]), 100.0 * (_median(ts[1]) - _median(ts[0])) / _median(ts[0])))
            b = last[1]['bandwidth']
            lines.append("the last file: input %.2f kHz, output %.2f kHz, original %.2f kHz, %d frames" % (b['input'] / 1e3, b['output'] / 1e3, b['original'] / 1e3, b['frames']))
            fixed, auto = SuperResolver(model, opt, overlap=0.25, crossover='input'), SuperResolver(model, opt, overlap=0.25, crossover='input', crossover_hz='auto')
            ts, last = interleaved([("crossover fixed      ", fixed, {}), ("crossover auto       ", auto, {})], src, out)
            lines.append("auto costs %.3f ms per file over the fixed crossover (difference of the medians): two launches, and the host waits for them "
                         "and a 32-byte copy before it can queue the crossover -- the groups are queued by then, so the device does not idle; the "
                         "last file: %r" % (_median(ts[1]) - _median(ts[0]), last[1]['crossover']))
    text = "\n".join(lines) + "\n"
    if not off_only:
        text += _bandwidth_kernels(torch, x, rate, reps)
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def _bandwidth_kernels(torch, x, rate, reps):
    """p2phd_ltas and p2phd_bandwidth alone, by events (each with the allocation of its result, the first also of its workspace, in
    front), on the 15 s clip and on an hour of it."""
    from pix2pixhdaudiosr_amd.generate import BANDWIDTH_DEFAULTS as P, bandwidth_detect, ltas
    lines = []
    hour = x.repeat(1, -(-3600 * rate // x.shape[-1]))[:, :3600 * rate].contiguous()
    for name, clip in (("the clip", x), ("an hour", hour)):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        k_ltas, k_dec = [], []
        for _ in range(reps + 2):
            ev[0].record()
            psd = ltas(clip, P['n_fft'], P['hop'])
            ev[1].record()
            bandwidth_detect(psd, 1, P['band_bins'], P['threshold_db'])
            ev[2].record()
            torch.cuda.synchronize()
            k_ltas.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_dec.append(ev[1].elapsed_time(ev[2]) * 1e3)
        L = clip.shape[-1]
        F = 1 + (L - P['n_fft']) // P['hop']
        us = _median(k_ltas[2:])
        lines.append("kernels alone on %s (events, median of %d): p2phd_ltas %.1f us (%d samples, %d frames of %d: %.2f M frames/s, %.2f GB/s of "
                     "samples read once), p2phd_bandwidth %.1f us" % (name, reps, us, L, F, P['n_fft'], F / us, 4.0 * L / us * 1e-3, _median(k_dec[2:])))
        lines.append("runs: p2phd_ltas %s; p2phd_bandwidth %s" % (" ".join("%.1f" % v for v in k_ltas[2:]), " ".join("%.1f" % v for v in k_dec[2:])))
    return "\n".join(lines) + "\n"


def run_stereo(seconds, reps, log, off_only=False):
    """enhance_file on a two-channel clip, file to file: without any option, with stereo_report=True (the same object) and with
    SuperResolver(stereo='ms'), interleaved; then p2phd_xspec and p2phd_stereo_bands alone, by events, beside p2phd_ltas on the same two
    rows, at the clip's frame count and at an hour's; and p2phd_stereo_matrix on the clip."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    n = x.shape[-1]
    g = torch.Generator().manual_seed(8)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    hi = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.02, 5200.0, 0.3), (0.01, 9100.0, 1.1), (0.005, 15300.0, 2.2)))
    mid = x.cpu()[:1] + hi.float()[None]
    own = 0.02 * torch.randn((2, n), generator=g)                   # what each channel has of its own, full band
    hr = mid + own
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py stereo: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s two-channel PCM16 clip at 48 kHz with a full-band original, file to file, channels='all', untrained weights, %d interleaved "
             "repeats" % (seconds, reps)]

    def interleaved(runs, src, out):
        last = [None] * len(runs)
        for k, (_, sr, kw) in enumerate(runs):                      # warm-up: capture, pinned buffers, page cache
            sr.enhance_file(src, out, channels='all', **kw)
            last[k] = sr.enhance_file(src, out, channels='all', **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(reps):
            for k, (_, sr, kw) in enumerate(runs):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, channels='all', **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _, _), tk in zip(runs, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        return ts, last

    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, hr, rate)
        sr = SuperResolver(model, opt, overlap=0.25)
        if off_only:
            interleaved([("no option            ", sr, {})], src, out)
        else:
            ms = SuperResolver(model, opt, overlap=0.25, stereo='ms')
            ts, last = interleaved([("stereo off           ", sr, {}), ("stereo_report        ", sr, dict(stereo_report=True)), ("stereo='ms'          ", ms, {})],
                                   src, out)
            base = _median(ts[0])
            lines.append("the report costs %.3f ms per file (difference of the medians), %.2f %% of the file without it: six launches and 192 bytes "
                         "more in the copy back" % (_median(ts[1]) - base, 100.0 * (_median(ts[1]) - base) / base))
            lines.append("the mode costs %.3f ms per file (difference of the medians), %.2f %%: two launches"
                         % (_median(ts[2]) - base, 100.0 * (_median(ts[2]) - base) / base))
            s = last[1]['stereo']
            lines.append("the last file ('lr'): correlation below / above %.2f kHz: %s; %d frames; %d note(s)"
                         % (s['split_hz'] / 1e3, ", ".join("%s %+.2f / %+.2f" % (k, s[k]['low']['corr'], s[k]['high']['corr']) for k in ('input', 'output', 'original')),
                            s['frames'], len(s['notes'])))
    text = "\n".join(lines) + "\n"
    if not off_only:
        text += _stereo_kernels(torch, hr.to(x.device), rate, reps)
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def _stereo_kernels(torch, x, rate, reps):
    """p2phd_xspec and p2phd_stereo_bands alone, by events (each with the allocation of its result, the first also of its workspace, in
    front), beside p2phd_ltas on the same two rows, on the clip and on an hour of it; p2phd_stereo_matrix on the clip."""
    from pix2pixhdaudiosr_amd.generate import STEREO_DEFAULTS as P, cross_spectrum, ltas, stereo_bands, stereo_matrix, stereo_split_bin
    lines = []
    k_split = stereo_split_bin(rate, 8000, P['n_fft'])
    hour = x.repeat(1, -(-3600 * rate // x.shape[-1]))[:, :3600 * rate].contiguous()
    for name, clip in (("the clip", x), ("an hour", hour)):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        k_x, k_b, k_l = [], [], []
        for _ in range(reps + 2):
            ev[0].record()
            xs = cross_spectrum(clip, P['n_fft'], P['hop'])
            ev[1].record()
            stereo_bands(xs, k_split)
            ev[2].record()
            ltas(clip, P['n_fft'], P['hop'])
            ev[3].record()
            torch.cuda.synchronize()
            k_x.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_b.append(ev[1].elapsed_time(ev[2]) * 1e3)
            k_l.append(ev[2].elapsed_time(ev[3]) * 1e3)
        L = clip.shape[-1]
        F = 1 + (L - P['n_fft']) // P['hop']
        lines.append("kernels alone on %s (events, median of %d; %d samples a row, %d frames of %d, %d transforms either way): p2phd_xspec %.1f us "
                     "(spread %.1f), p2phd_ltas on the same two rows %.1f us (spread %.1f), p2phd_stereo_bands %.1f us"
                     % (name, reps, L, F, P['n_fft'], F, _median(k_x[2:]), max(k_x[2:]) - min(k_x[2:]), _median(k_l[2:]), max(k_l[2:]) - min(k_l[2:]),
                        _median(k_b[2:])))
        lines.append("runs: p2phd_xspec %s; p2phd_ltas %s; p2phd_stereo_bands %s"
                     % tuple(" ".join("%.1f" % v for v in k[2:]) for k in (k_x, k_l, k_b)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    k_m = []
    for _ in range(reps + 2):
        ev[0].record()
        stereo_matrix(x, 0.5)
        ev[1].record()
        torch.cuda.synchronize()
        k_m.append(ev[0].elapsed_time(ev[1]) * 1e3)
    lines.append("p2phd_stereo_matrix on the clip (with the allocation of its result): %.1f us; runs: %s" % (_median(k_m[2:]), " ".join("%.1f" % v for v in k_m[2:])))
    return "\n".join(lines) + "\n"


def run_rateconv(seconds, reps, log, off_only=False):
    """enhance_file on a mono clip, file to file: without any option and with output_rate=44100 (the same object), interleaved; then
    p2phd_rateconv_fwd alone, by events, at the clip's length and at an hour's, beside the feeder's p2phd_resample_fwd at the same two
    rates on the same clip."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py rateconv: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz, file to file, untrained weights, %d interleaved repeats" % (seconds, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, x.cpu(), rate)
        sr = SuperResolver(model, opt, overlap=0.25)
        runs = [("no option            ", {})] if off_only else [("output_rate off      ", {}), ("output_rate 44100    ", dict(output_rate=44100))]
        last = None
        for _, kw in runs:                                          # warm-up: capture, pinned buffers, page cache, the table
            sr.enhance_file(src, out, **kw)
            last = sr.enhance_file(src, out, **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(reps):
            for k, (_, kw) in enumerate(runs):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(runs, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        if not off_only:
            base = _median(ts[0])
            r = last['output_rate']
            lines.append("the option costs %+.3f ms per file (difference of the medians), %+.2f %% of the file without it: one launch more, and the "
                         "stages behind it, the encoder and the copy back handle %d samples where they handled %d (%d taps x %d phases)"
                         % (_median(ts[1]) - base, 100.0 * (_median(ts[1]) - base) / base, last['sr'].shape[-1], x.shape[-1], r['taps_per_phase'], r['n']))
    text = "\n".join(lines) + "\n"
    if not off_only:
        text += _rateconv_kernels(torch, x, rate, reps)
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def _rateconv_kernels(torch, x, rate, reps):
    """p2phd_rateconv_fwd alone, by events (with the allocation of its result in front), on the clip and on an hour of it, beside the
    feeder's p2phd_resample_fwd (data.resample: the reference's 6-zero-crossing Hann sinc) at the same rates on the same rows."""
    from pix2pixhdaudiosr_amd.data.resample import resample
    from pix2pixhdaudiosr_amd.generate import rate_convert, rateconv_plan
    plan = rateconv_plan(rate, 44100)
    lines = []
    hour = x.repeat(1, -(-3600 * rate // x.shape[-1]))[:, :3600 * rate].contiguous()
    for name, clip in (("the clip", x), ("an hour", hour)):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        k_c, k_f = [], []
        for _ in range(reps + 2):
            ev[0].record()
            y = rate_convert(clip, rate, 44100, plan)
            ev[1].record()
            z = resample(clip, rate, 44100)
            ev[2].record()
            torch.cuda.synchronize()
            k_c.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_f.append(ev[1].elapsed_time(ev[2]) * 1e3)
        Lo = y.shape[-1]
        c, f = _median(k_c[2:]), _median(k_f[2:])
        lines.append("kernels alone on %s (events, median of %d; %d samples in, %d out): p2phd_rateconv_fwd %.1f us (spread %.1f) = %.3f ns per output, "
                     "%.1f Gfma/s over its %d taps; p2phd_resample_fwd on the same row %.1f us (spread %.1f) = %.3f ns per output (%d out)"
                     % (name, reps, clip.shape[-1], Lo, c, max(k_c[2:]) - min(k_c[2:]), c * 1e3 / Lo, Lo * plan['taps_per_phase'] / c * 1e-3,
                        plan['taps_per_phase'], f, max(k_f[2:]) - min(k_f[2:]), f * 1e3 / z.shape[-1], z.shape[-1]))
        lines.append("runs: p2phd_rateconv_fwd %s; p2phd_resample_fwd %s" % tuple(" ".join("%.1f" % v for v in k[2:]) for k in (k_c, k_f)))
        del y, z
    return "\n".join(lines) + "\n"


def run_speechlevel(seconds, reps, log, off_only=False):
    """enhance_file on a mono clip, file to file: without any option, with speech_level='report' and with speech_level=-26 (the same
    object), interleaved; then the three entries of csrc/speechlevel.hip alone, by events, at the clip's length and at an hour's."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py speechlevel: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz, file to file, untrained weights, %d interleaved repeats" % (seconds, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, x.cpu(), rate)
        sr = SuperResolver(model, opt, overlap=0.25)
        runs = [("no option            ", {})] if off_only else [("speech_level off     ", {}), ("speech_level report  ", dict(speech_level='report')),
                                                                  ("speech_level -26     ", dict(speech_level=-26.0))]
        last = None
        for _, kw in runs:                                          # warm-up: capture, pinned buffers, page cache
            sr.enhance_file(src, out, **kw)
            last = sr.enhance_file(src, out, **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(reps):
            for k, (_, kw) in enumerate(runs):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(runs, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        if not off_only:
            base = _median(ts[0])
            s = last['speech_level']
            for k in (1, 2):
                lines.append("%s costs %+.3f ms per file (difference of the medians), %+.2f %% of the file without it: six launches more"
                             % (runs[k][0].strip(), _median(ts[k]) - base, 100.0 * (_median(ts[k]) - base) / base))
            lines.append("the clip: input %+.2f dBov (activity %.1f %%), measured %+.2f dBov (activity %.1f %%), gain %+.2f dB"
                         % (s['input'], 100.0 * s['activity_input'], s['measured'], 100.0 * s['activity'], s['gain_db']))
    text = "\n".join(lines) + "\n"
    if not off_only:
        text += _speechlevel_kernels(torch, x, rate, reps)
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def _speechlevel_kernels(torch, x, rate, reps):
    """The three entries alone, by events (with the allocation of their results in front), on the clip and on an hour of it."""
    from pix2pixhdaudiosr_amd.generate import speech_level_counts, speech_level_decide, speech_level_envelope
    lines = []
    hour = x.repeat(1, -(-3600 * rate // x.shape[-1]))[:, :3600 * rate].contiguous()
    for name, clip in (("the clip", x), ("an hour", hour)):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        k_e, k_c, k_d = [], [], []
        for _ in range(reps + 2):
            ev[0].record()
            m, sq = speech_level_envelope(clip, rate)
            ev[1].record()
            a = speech_level_counts(m, rate)
            ev[2].record()
            speech_level_decide(sq, a, clip.shape[-1], target=-26.0)
            ev[3].record()
            torch.cuda.synchronize()
            k_e.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_c.append(ev[1].elapsed_time(ev[2]) * 1e3)
            k_d.append(ev[2].elapsed_time(ev[3]) * 1e3)
        n = clip.shape[-1]
        e, c, d = (_median(k[2:]) for k in (k_e, k_c, k_d))
        lines.append("kernels alone on %s (events, median of %d; %d samples): p2phd_speechlevel_envelope (three kernels) %.1f us (spread %.1f) = %.3f ns "
                     "per sample, %.1f GB/s of input read twice and m written once; p2phd_speechlevel_counts %.1f us (spread %.1f) = %.3f ns per sample; "
                     "p2phd_speechlevel_decide %.1f us (spread %.1f)"
                     % (name, reps, n, e, max(k_e[2:]) - min(k_e[2:]), e * 1e3 / n, 9.0 * n / e * 1e-3, c, max(k_c[2:]) - min(k_c[2:]), c * 1e3 / n,
                        d, max(k_d[2:]) - min(k_d[2:])))
        lines.append("runs: envelope %s; counts %s; decide %s" % tuple(" ".join("%.1f" % v for v in k[2:]) for k in (k_e, k_c, k_d)))
        del m, sq, a
    return "\n".join(lines) + "\n"


def run_dither(seconds, reps, log, off_only=False):
    """enhance_file on a mono clip, file to file: without any option, with dither='tpdf' and with dither='shaped' (the same object),
    interleaved; then p2phd_pcm_encode_shaped alone, by events, at chunk 4096, at chunk 1024 and at one chunk for the whole row (the
    plain sequential recursion), beside p2phd_pcm_encode_ex with TPDF, at the clip's length and at an hour's."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py dither: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz, file to file, untrained weights, %d interleaved repeats" % (seconds, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, x.cpu(), rate)
        sr = SuperResolver(model, opt, overlap=0.25)
        runs = [("no option            ", {})] if off_only else [("dither off           ", {}), ("dither tpdf          ", dict(dither='tpdf')),
                                                                  ("dither shaped        ", dict(dither='shaped'))]
        for _, kw in runs:                                          # warm-up: capture, pinned buffers, page cache, code objects
            sr.enhance_file(src, out, **kw)
            sr.enhance_file(src, out, **kw)
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(reps):
            for k, (_, kw) in enumerate(runs):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(runs, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        if not off_only:
            t, sh = _median(ts[1]), _median(ts[2])
            lines.append("shaped costs %+.3f ms per file over tpdf (difference of the medians), %+.2f %% of that file: the encoder's launch is "
                         "replaced by the shaper's" % (sh - t, 100.0 * (sh - t) / t))
    text = "\n".join(lines) + "\n"
    if not off_only:
        text += _dither_kernels(torch, x, rate, reps)
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def _dither_kernels(torch, x, rate, reps):
    """p2phd_pcm_encode_shaped alone, by events (with the allocation of its payload in front), on the clip and on an hour of it, at
    three chunk lengths, beside p2phd_pcm_encode_ex with TPDF on the same row.  One chunk for the whole row -- the recursion as one
    sequential chain -- is timed on the clip only, and once: it is the measured cost of not chunking."""
    from pix2pixhdaudiosr_amd.generate import pcm_encode
    lines = []
    x = (0.25 * x / x.abs().max().clamp_min(1e-9)).contiguous()
    hour = x.repeat(1, -(-3600 * rate // x.shape[-1]))[:, :3600 * rate].contiguous()
    for name, clip in (("the clip", x), ("an hour", hour)):
        kinds = [("p2phd_pcm_encode_ex tpdf", dict(dither='tpdf')), ("p2phd_pcm_encode_shaped chunk 4096", dict(dither='shaped', chunk=4096)),
                 ("p2phd_pcm_encode_shaped chunk 1024", dict(dither='shaped', chunk=1024))]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(kinds) + 1)]
        ks = [[] for _ in kinds]
        for _ in range(reps + 2):
            ev[0].record()
            for k, (_, kw) in enumerate(kinds):
                pcm_encode(clip, 'pcm16', seed=1, **kw)
                ev[k + 1].record()
            torch.cuda.synchronize()
            for k in range(len(kinds)):
                ks[k].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
        L = clip.shape[-1]
        lines.append("kernels alone on %s (events, median of %d; %d samples, lipshitz9): %s"
                     % (name, reps, L, "; ".join("%s %.1f us (spread %.1f) = %.3f ns per sample%s"
                                                 % (kn, _median(k[2:]), max(k[2:]) - min(k[2:]), _median(k[2:]) * 1e3 / L,
                                                    ", %d lanes" % -(-L // kw['chunk']) if 'chunk' in kw else "")
                                                 for (kn, kw), k in zip(kinds, ks))))
        lines.append("runs: " + "; ".join("%s %s" % (kn, " ".join("%.1f" % v for v in k[2:])) for (kn, _), k in zip(kinds, ks)))
    whole = 1 << 20                                                 # one chunk holds the clip: one lane walks it
    if x.shape[-1] <= whole:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        pcm_encode(x, 'pcm16', dither='shaped', chunk=whole, seed=1)
        ev[1].record()
        torch.cuda.synchronize()
        t = ev[0].elapsed_time(ev[1]) * 1e3
        lines.append("the recursion as one sequential chain on the clip (chunk %d >= %d samples, one lane, one run): %.1f us = %.1f ns per sample"
                     % (whole, x.shape[-1], t, t * 1e3 / x.shape[-1]))
    return "\n".join(lines) + "\n"


def run_flac(seconds, reps, log):
    """The input side on the same samples, three ways, interleaved: the FLAC path of SuperResolver (_read: file bytes into the pinned
    slot and the index on the host; _decode: one copy of bytes and table, the two kernels of the family "flac"), the WAV path
    (read_payload, copy, p2phd_pcm_decode) and the host decoder followed by a copy (flacio.load -> .cuda()).  Then, by events, the
    device decode whole and each kernel alone (p2phd_flac_decode_stage) beside p2phd_pcm_decode, on the clip and on an hour of it.  The
    clip is encoded by the restatement tests/_flac_ref.py: mono, 16 bit, block size 4096, FIXED order 2 and LPC order 8 subframes in
    turn.  The hour is the clip's bytes 240 times over with a table whose offsets and columns are shifted -- the device decoder reads
    the table, not the frames' numbers; the host index cannot be run on such an hour and is stated as 240 times the clip's; the host decoder is run on it, three times."""
    import tempfile
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _flac_ref as R
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.data import flacio, wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, flac_decode, pcm_decode
    rate = int(opt.hr_sampling_rate)
    q = torch.round(0.5 * x[0].cpu().double() * 32768.0).clamp(-32768, 32767).to(torch.int64)
    ints = q.tolist()
    lpc8 = dict(kind="lpc", coefs=[2048, -1024, 0, 0, 0, 0, 0, 0], precision=13, shift=10, porder=4, method=0)
    fixed = dict(kind="fixed", order=2, porder=4)
    last = len(ints) % 4096
    t0 = time.perf_counter()
    data, frames = R.make_stream([ints], 16, 4096, rate=rate, specs=lambda k, c: dict(fixed if k % 2 == 0 else lpc8, porder=4 if (k + 1) * 4096 <= len(ints) or last % 16 == 0 else 0))
    t_enc = time.perf_counter() - t0
    lines = ["# tools/time_generate.py flac: one %g s mono 16-bit clip at 48 kHz (%d samples), block size 4096, FIXED 2 / LPC 8 in turn, %d frames, %d bytes "
             "as FLAC (%.1f %% of the PCM16 payload; the restatement took %.1f s to encode it); %d interleaved repeats"
             % (seconds, len(ints), len(frames), len(data), 100.0 * len(data) / (2 * len(ints)), t_enc, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        pf, pw = os.path.join(tmp, "in.flac"), os.path.join(tmp, "in.wav")
        with open(pf, "wb") as f:
            f.write(data)
        wavio.save(pw, (q.float() / 32768.0)[None], rate)
        assert torch.equal(flacio.load(pf)[0], wavio.load(pw)[0])
        sr = SuperResolver(model, opt, overlap=0.25)

        def flac_path():
            return sr._decode(*sr._read(pf))

        def wav_path():
            return sr._decode(*sr._read(pw))

        def host_path():
            return flacio.load(pf)[0].cuda()

        def read_only():
            return sr._read(pf)
        runs = [("flac: _read + _decode (index on the host, device decode)", flac_path), ("flac: _read alone (file bytes, index)", read_only),
                ("wav:  _read + _decode (read_payload, copy, pcm_decode) ", wav_path), ("flac: host decoder + copy (flacio.load, .cuda())      ", host_path)]
        assert torch.equal(flac_path(), wav_path()) and torch.equal(host_path(), wav_path())
        for _, fn in runs:
            fn(); fn()
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(reps):
            for k, (_, fn) in enumerate(runs):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(runs, ts):
            lines.append("%s  median %8.3f ms   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
    meta, table = flacio.index_bytes(data)
    raw = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    pcm = torch.from_numpy(np.array(ints, dtype="<i2").view(np.uint8).copy()).cuda()
    copies = 3600 * rate // len(ints)
    big_table = np.concatenate([table + np.array([k * len(data), 0, k * len(ints), 0, 0, 0], dtype=np.int64) for k in range(copies)])
    big_meta = meta._replace(num_frames=copies * len(ints), num_flac_frames=len(big_table))
    def one_stage(stage, b, t, m):                                 # generate.flac_decode's allocations in front of one kernel alone
        out = torch.zeros((1, m.num_frames), dtype=torch.float32, device=b.device)
        status = torch.full((1,), -1, dtype=torch.int64, device=b.device)
        work = torch.empty((_lib.lib().p2phd_flac_workspace_bytes(1, m.num_frames),), dtype=torch.uint8, device=b.device)
        _lib.check(_lib.lib().p2phd_flac_decode_stage(stage, _lib.ptr(b), b.numel(), _lib.ptr(t), t.shape[0], 1, 16, _lib.ptr(out), m.num_frames,
                                                      _lib.ptr(work), _lib.ptr(status), _lib.stream_ptr()), "flac_decode_stage")
        return out

    for name, b, t, m, payload in (("the clip", raw, torch.from_numpy(table.copy()).cuda(), meta, pcm),
                                   ("an hour", raw.repeat(copies), torch.from_numpy(big_table).cuda(), big_meta, pcm.repeat(copies))):
        kinds = [("p2phd_flac_decode, both kernels", 0), ("flac_frames_kernel alone", 1), ("flac_pcm_kernel alone", 2), ("p2phd_pcm_decode", None)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(kinds) + 1)]
        ks = [[] for _ in kinds]
        for _ in range(reps + 2):
            outs = []
            ev[0].record()
            for k, (_, stage) in enumerate(kinds):
                if stage is None:
                    outs.append(pcm_decode(payload, m.num_frames, 1, 1, 16))
                elif stage == 0:
                    outs.append(flac_decode(b, t, m, check=False)[0])
                else:
                    outs.append(one_stage(stage, b, t, m))
                ev[k + 1].record()
            torch.cuda.synchronize()
            for k in range(len(kinds)):
                ks[k].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
            assert torch.equal(outs[0], outs[3])
            del outs
        L = m.num_frames
        lines.append("by events on %s (median of %d, each with the allocation and zeroing of its result in front; %d samples, %d frames = %d waves of the frame kernel): %s"
                     % (name, reps, L, m.num_flac_frames, -(-m.num_flac_frames // 64),
                        "; ".join("%s %.1f us (spread %.1f) = %.3f ns per sample" % (kn, _median(k[2:]), max(k[2:]) - min(k[2:]), _median(k[2:]) * 1e3 / L)
                                  for (kn, _), k in zip(kinds, ks))))
        lines.append("runs: " + "; ".join("%s %s" % (kn, " ".join("%.1f" % v for v in k[2:])) for (kn, _), k in zip(kinds, ks)))
    th, ti = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        flacio.index_bytes(data)
        ti.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        flacio.decode_frames(data, table, 0, len(table), 1)
        th.append((time.perf_counter() - t0) * 1e3)
    big = data * copies
    tb = []
    for _ in range(3):
        t0 = time.perf_counter()
        flacio.decode_frames(big, big_table, 0, len(big_table), 1)
        tb.append((time.perf_counter() - t0) * 1e3)
    lines.append("on the host, one thread, the clip: index (every CRC) median %.3f ms = %.2f ns per byte; p2phd_flac_decode_host median %.3f ms = %.2f ns per sample.  "
                 "The hour (the clip's bytes %d times over under a shifted table, as on the device): p2phd_flac_decode_host measured %s ms (3 runs, with the "
                 "allocation of its int32 rows); its index is not measured -- the repeated frames' numbers do not chain -- and would be %d times the clip's, %.0f ms"
                 % (_median(ti), _median(ti) * 1e6 / len(data), _median(th), _median(th) * 1e6 / len(ints), copies, " ".join("%.0f" % v for v in tb), copies,
                    _median(ti) * copies))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def run_wavcodec(seconds, reps, log):
    """Coded WAV input (G.711 mu-law, A-law, IMA ADPCM with 256-byte blocks; csrc/wavcodec.hip) against the PCM16 twin of the same
    samples: a mono telephone clip at 8 kHz, written by the restatement tests/_wavcodec_ref.py.  Interleaved: enhance_file
    (is_lr_input) per file, and the input side alone (_read + _decode).  Then, by events, each decoder's kernel alone beside
    p2phd_pcm_decode on the clip and on an hour of it (the clip's bytes 240 times over: G.711 is element-wise and IMA blocks are
    independent), and the host entries on one thread."""
    import ctypes
    import tempfile
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _wavcodec_ref as R
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, g711_decode, ima_decode, pcm_decode
    rate, align = 8000, 256
    n = int(seconds * rate)
    ints = torch.round(0.5 * x[0, ::6][:n].cpu().double() * 32768.0).clamp(-32768, 32767).to(torch.int64).numpy()[None]
    t0 = time.perf_counter()
    ima = R.ima_encode(ints, align, partial=False)
    t_enc = time.perf_counter() - t0
    payloads = {"ulaw": R.g711_encode(ints, R.ULAW), "alaw": R.g711_encode(ints, R.ALAW), "ima": ima}
    decoded = {"ulaw": R.g711_decode(payloads["ulaw"], n, 1, R.ULAW), "alaw": R.g711_decode(payloads["alaw"], n, 1, R.ALAW)}
    lines = ["# tools/time_generate.py wavcodec: one %g s mono clip at 8 kHz (%d samples) as mu-law, A-law (%d bytes each) and IMA ADPCM (block_align %d, "
             "505 samples a block, %d bytes; the restatement took %.1f s to encode it), each beside its PCM16 twin (%d bytes); %d interleaved repeats"
             % (seconds, n, n, align, len(ima), t_enc, 2 * n, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for kind, tag in (("ulaw", R.TAG_ULAW), ("alaw", R.TAG_ALAW), ("ima", R.TAG_IMA)):
            paths[kind] = os.path.join(tmp, kind + ".wav")
            if kind == "ima":
                R.write_coded_wav(paths[kind], tag, payloads[kind], rate, 1, block_align=align, fact=n)
                decoded[kind] = wavio.load(paths[kind])[0].numpy()
                R.write_pcm16_wav(os.path.join(tmp, "ima_pcm.wav"), np.rint(decoded[kind] * 32768.0).astype(np.int64), rate)
            else:
                R.write_coded_wav(paths[kind], tag, payloads[kind], rate, 1)
                R.write_pcm16_wav(os.path.join(tmp, kind + "_pcm.wav"), decoded[kind], rate)
            paths[kind + "_pcm"] = os.path.join(tmp, kind + "_pcm.wav")
            assert torch.equal(wavio.load(paths[kind])[0], wavio.load(paths[kind + "_pcm"])[0])
        sr = SuperResolver(model, opt, overlap=0.25)
        out = os.path.join(tmp, "out.wav")
        order = ["ulaw", "ulaw_pcm", "alaw", "alaw_pcm", "ima", "ima_pcm"]
        for what, fn in (("enhance_file(is_lr_input), file to file", lambda k: sr.enhance_file(paths[k], out, is_lr_input=True)),
                         ("_read + _decode alone", lambda k: sr._decode(*sr._read(paths[k])))):
            for k in order:
                fn(k); fn(k)
            torch.cuda.synchronize()
            ts = {k: [] for k in order}
            for _ in range(reps):
                for k in order:
                    t0 = time.perf_counter()
                    fn(k)
                    torch.cuda.synchronize()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            lines.append(what + ":")
            for k in order:
                tk = ts[k]
                lines.append("  %-9s median %8.3f ms   spread %6.3f (%.3f .. %.3f)   runs: %s"
                             % (k, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
            for k in ("ulaw", "alaw", "ima"):
                lines.append("  %s - its twin: %+.3f ms of medians; the twin's own spread %.3f ms"
                             % (k, _median(ts[k]) - _median(ts[k + "_pcm"]), max(ts[k + "_pcm"]) - min(ts[k + "_pcm"])))
    copies = 3600 * rate // n
    dev = {k: torch.frombuffer(bytearray(v), dtype=torch.uint8).cuda() for k, v in payloads.items()}
    dev["pcm"] = torch.from_numpy(ints[0].astype("<i2").view(np.uint8).copy()).cuda()
    for name, c in (("the clip", 1), ("an hour", copies)):
        b = {k: v.repeat(c) for k, v in dev.items()}
        L = n * c
        Lima = R.ima_frames(len(ima) * c, 1, align)
        kinds = [("g711_decode_kernel mu-law", lambda: g711_decode(b["ulaw"], L, 1, 'ulaw')), ("g711_decode_kernel A-law", lambda: g711_decode(b["alaw"], L, 1, 'alaw')),
                 ("ima_decode_kernel", lambda: ima_decode(b["ima"], Lima, 1, align)), ("p2phd_pcm_decode (PCM16)", lambda: pcm_decode(b["pcm"], L, 1, 1, 16))]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(kinds) + 1)]
        ks = [[] for _ in kinds]
        for _ in range(reps + 2):
            outs = []
            ev[0].record()
            for k, (_, fn) in enumerate(kinds):
                outs.append(fn())
                ev[k + 1].record()
            torch.cuda.synchronize()
            for k in range(len(kinds)):
                ks[k].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
            del outs
        lines.append("by events on %s (median of %d, each with the allocation of its result in front; %d samples, %d IMA blocks): %s"
                     % (name, reps, L, -(-Lima // 505), "; ".join("%s %.1f us (spread %.1f) = %.4f ns per sample" % (kn, _median(k[2:]), max(k[2:]) - min(k[2:]), _median(k[2:]) * 1e3 / L)
                                                                   for (kn, _), k in zip(kinds, ks))))
        lines.append("runs: " + "; ".join("%s %s" % (kn, " ".join("%.1f" % v for v in k[2:])) for (kn, _), k in zip(kinds, ks)))
    lib = _lib.lib()
    for name, c, r in (("the clip", 1, reps), ("an hour", copies, 3)):
        L = n * c
        res = []
        out_h = np.zeros(L + 505, dtype=np.float32)
        for kind in ("ulaw", "alaw", "ima"):
            src = np.frombuffer(payloads[kind] * c, dtype=np.uint8)
            tk = []
            for _ in range(r):
                t0 = time.perf_counter()
                if kind == "ima":
                    rc = lib.p2phd_ima_decode_host(ctypes.c_void_p(src.ctypes.data), src.size, 1, align, 0, L, ctypes.c_void_p(out_h.ctypes.data), L)
                else:
                    rc = lib.p2phd_g711_decode_host(ctypes.c_void_p(src.ctypes.data), L, 1, 1 if kind == "alaw" else 0, ctypes.c_void_p(out_h.ctypes.data), L)
                tk.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            res.append("%s median %.3f ms = %.2f ns per sample (%s)" % (kind, _median(tk), _median(tk) * 1e6 / L, " ".join("%.3f" % v for v in tk)))
        lines.append("on the host, one thread, %s (the host entry alone, into a buffer that exists): %s" % (name, "; ".join(res)))
    lines.append("not measured here: the option-off path (a PCM input) and the benchmark step against the parent commit in alternating processes")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def run_containers(seconds, reps, log):
    """AIFF, AU and NIST SPHERE input (data/containers.py, p2phd_pcm_decode_ex of csrc/pcm.hip) against the WAV twin of the same
    samples, written by the restatement tests/_containers_ref.py: a mono clip at 48 kHz as AIFF 16-bit and as SPHERE pcm (byte format
    10), and its 8 kHz decimation as AU mu-law (is_lr_input).  Interleaved: enhance_file per file, and the input side alone (_read +
    _decode).  Then, by events, p2phd_pcm_decode_ex with P2PHD_PCM_BIG_ENDIAN at S16 / S24 / F32 beside p2phd_pcm_decode on the
    byte-swapped twin -- the yardstick is the little-endian kernel of the same tree -- on the clip and on an hour of it (the clip's
    bytes 240 times over)."""
    import tempfile
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _containers_ref as R
    import _wavcodec_ref as W
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import audiofile, wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, pcm_decode
    rate = opt.hr_sampling_rate
    n = int(seconds * rate)
    ints = torch.round(0.5 * x[0, :n].cpu().double() * 32768.0).clamp(-32768, 32767).to(torch.int64).numpy()[None]
    low = ints[:, ::6]
    codes = W.g711_encode(low, W.ULAW)
    lines = ["# tools/time_generate.py containers: one %g s mono clip at %d Hz (%d samples) as AIFF 16-bit and SPHERE pcm (big-endian), and its 8 kHz "
             "decimation (%d samples) as AU mu-law, each beside its WAV twin; %d interleaved repeats" % (seconds, rate, n, low.shape[1], reps)]
    with tempfile.TemporaryDirectory() as tmp:
        paths = {k: os.path.join(tmp, k) for k in ("aiff.aif", "aiff_twin.wav", "sphere.sph", "sphere_twin.wav", "au_ulaw.au", "au_ulaw_twin.wav")}
        with open(paths["aiff.aif"], "wb") as f:
            f.write(R.aiff(R.int_bytes(ints, 2), 1, n, 16, rate=rate))
        with open(paths["sphere.sph"], "wb") as f:
            f.write(R.sphere(R.int_bytes(ints, 2), R.sphere_fields(1, rate, 2, n, "pcm", "10")))
        with open(paths["au_ulaw.au"], "wb") as f:
            f.write(R.au(codes, 1, 8000, 1))
        W.write_pcm16_wav(paths["aiff_twin.wav"], ints, rate)
        W.write_pcm16_wav(paths["sphere_twin.wav"], ints, rate)
        W.write_pcm16_wav(paths["au_ulaw_twin.wav"], W.g711_decode(codes, low.shape[1], 1, W.ULAW), 8000)
        order = list(paths)
        for a, b in zip(order[0::2], order[1::2]):
            assert torch.equal(audiofile.load(paths[a])[0].view(torch.int32), wavio.load(paths[b])[0].view(torch.int32))
        sr = SuperResolver(model, opt, overlap=0.25)
        out = os.path.join(tmp, "out.wav")
        for what, fn in (("enhance_file, file to file (the 8 kHz pair with is_lr_input)", lambda k: sr.enhance_file(paths[k], out, is_lr_input=k.startswith("au"))),
                         ("_read + _decode alone", lambda k: sr._decode(*sr._read(paths[k])))):
            for k in order:
                fn(k); fn(k)
            torch.cuda.synchronize()
            ts = {k: [] for k in order}
            for _ in range(reps):
                for k in order:
                    t0 = time.perf_counter()
                    fn(k)
                    torch.cuda.synchronize()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            lines.append(what + ":")
            for k in order:
                tk = ts[k]
                lines.append("  %-16s median %8.3f ms   range %.3f .. %.3f   runs: %s" % (k, _median(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
            for a, b in zip(order[0::2], order[1::2]):
                lines.append("  %s - its twin: %+.3f ms of medians; the twin's own spread %.3f ms" % (a, _median(ts[a]) - _median(ts[b]), max(ts[b]) - min(ts[b])))
    i24 = ints * 256 + 37
    f32 = (ints / 32768.0).astype(np.float32)
    pay = {("S16", True): R.int_bytes(ints, 2), ("S16", False): R.int_bytes(ints, 2, False), ("S24", True): R.int_bytes(i24, 3),
           ("S24", False): R.int_bytes(i24, 3, False), ("F32", True): R.float_bytes(f32, 4), ("F32", False): R.float_bytes(f32, 4, False)}
    dev = {k: torch.frombuffer(bytearray(v), dtype=torch.uint8).cuda() for k, v in pay.items()}
    fmt = {"S16": (1, 16), "S24": (1, 24), "F32": (3, 32)}
    for name, c in (("the clip", 1), ("an hour", 3600 * rate // n)):
        L = n * c
        kinds = []
        for f in ("S16", "S24", "F32"):
            be, le = dev[(f, True)].repeat(c), dev[(f, False)].repeat(c)
            kinds.append(("pcm_decode_ex %s big-endian" % f, lambda be=be, f=f: pcm_decode(be, L, 1, *fmt[f], big_endian=True)))
            kinds.append(("pcm_decode %s" % f, lambda le=le, f=f: pcm_decode(le, L, 1, *fmt[f])))
        assert all(torch.equal(kinds[i][1]().view(torch.int32), kinds[i + 1][1]().view(torch.int32)) for i in (0, 2, 4))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(kinds) + 1)]
        ks = [[] for _ in kinds]
        for _ in range(reps + 2):
            outs = []
            ev[0].record()
            for k, (_, fn) in enumerate(kinds):
                outs.append(fn())
                ev[k + 1].record()
            torch.cuda.synchronize()
            for k in range(len(kinds)):
                ks[k].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
            del outs
        lines.append("by events on %s (median of %d, each with the allocation of its result in front; %d samples):" % (name, reps, L))
        for (kn, _), k in zip(kinds, ks):
            lines.append("  %-28s %9.1f us (range %.1f .. %.1f) = %.4f ns per sample   runs: %s"
                         % (kn, _median(k[2:]), min(k[2:]), max(k[2:]), _median(k[2:]) * 1e3 / L, " ".join("%.1f" % v for v in k[2:])))
        for i in (0, 2, 4):
            lines.append("  %s - %s: %+.1f us of medians; the little-endian kernel's own spread %.1f us"
                         % (kinds[i][0], kinds[i + 1][0], _median(ks[i][2:]) - _median(ks[i + 1][2:]), max(ks[i + 1][2:]) - min(ks[i + 1][2:])))
    lines.append("not measured here: the WAV path and the benchmark step against the parent commit in alternating processes")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def run_flacout(seconds, reps, log):
    """The output side, file to file: enhance_file with container 'wav' and 'flac' on one mono and one stereo 16-bit clip, interleaved.
    Then, by events, p2phd_flac_encode (generate.flac_encode: its allocations in front) beside p2phd_pcm_encode_ex on the written
    payloads, on the clip and on an hour of it (the payload repeated); the host encoder, one thread, on the clip; and the streams'
    sizes.  The clips are the synthetic partials of the other modes through an untrained model: what they say about speech is
    little."""
    import tempfile
    import numpy as np
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.data import flacio, wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, flac_encode, pcm_encode
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py flacout: one %g s clip at %d Hz (%d samples per channel), mono and stereo, pcm16, block size 4096; %d interleaved repeats"
             % (seconds, rate, x.shape[-1], reps)]
    payloads = {}
    with tempfile.TemporaryDirectory() as tmp:
        sr = SuperResolver(model, opt, overlap=0.25)
        for tag, clip in (("mono", 0.5 * x), ("stereo", torch.cat([0.5 * x, 0.4 * x.flip(-1) + 0.1 * x]))):
            src = os.path.join(tmp, tag + "_in.wav")
            wavio.save(src, clip.cpu(), rate)
            pw, pf = os.path.join(tmp, tag + ".wav"), os.path.join(tmp, tag + ".flac")
            runs = [("%s: container wav " % tag, lambda: sr.enhance_file(src, pw, channels='all')),
                    ("%s: container flac" % tag, lambda: sr.enhance_file(src, pf, channels='all', container='flac')),
                    ("%s: flac, flac_md5" % tag, lambda: sr.enhance_file(src, pf, channels='all', container='flac', flac_md5=True))]
            for _, fn in runs:
                fn(); fn()
            torch.cuda.synchronize()
            ts = [[] for _ in runs]
            for _ in range(reps):
                for k, (_, fn) in enumerate(runs):
                    torch.manual_seed(3)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            for (name, _), tk in zip(runs, ts):
                lines.append("%s  median %8.3f ms   spread %6.3f (%.3f .. %.3f)   runs: %s"
                             % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
            torch.manual_seed(3)
            sr.enhance_file(src, pw, channels='all')
            torch.manual_seed(3)
            res = sr.enhance_file(src, pf, channels='all', container='flac')
            pay, _ = wavio.read_payload(pw)
            payloads[tag] = (bytes(pay), clip.shape[0])
            meta, table = flacio.index_bytes(open(pf, "rb").read())
            assert flacio.decode_frames(open(pf, "rb").read(), table, 0, len(table), clip.shape[0]).T.astype("<i2").tobytes() == payloads[tag][0]
            lines.append("%s: %d frames, %d bytes of FLAC for %d of PCM (%.1f %%); the worst-case stream that is copied back: %d bytes"
                         % (tag, res['flac']['frames'], res['flac']['bytes'], res['flac']['pcm_bytes'], 100.0 * res['flac']['bytes'] / res['flac']['pcm_bytes'],
                            flacio.encode_plan(clip.shape[0], 16, meta.num_frames, 4096)[1]))
    for tag, (pay, C) in payloads.items():
        dev = torch.frombuffer(bytearray(pay), dtype=torch.uint8).cuda()
        L = len(pay) // (2 * C)
        copies = 3600 * rate // L
        planar = torch.from_numpy(np.frombuffer(pay, dtype="<i2").reshape(-1, C).T.astype(np.float32) / 32768.0).cuda().contiguous()
        for name, b, w in (("the clip", dev, planar), ("an hour", dev.repeat(copies), planar.repeat(1, copies))):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ks = [[], []]
            for _ in range(reps + 2):
                ev[0].record()
                out = flac_encode(b, C, 16, rate)
                ev[1].record()
                enc = pcm_encode(w, 'pcm16')
                ev[2].record()
                torch.cuda.synchronize()
                ks[0].append(ev[0].elapsed_time(ev[1]) * 1e3)
                ks[1].append(ev[1].elapsed_time(ev[2]) * 1e3)
                total = int(out[1][-1].item())
                del out, enc
            n = b.numel() // (2 * C)
            lines.append("by events on %s, %s (median of %d, allocations in front; %d samples per channel, %d frames, %d bytes of FLAC): p2phd_flac_encode %.1f us "
                         "(spread %.1f) = %.3f ns per sample; p2phd_pcm_encode_ex %.1f us (spread %.1f) = %.3f ns per sample"
                         % (name, tag, reps, n, -(-n // 4096), total, _median(ks[0][2:]), max(ks[0][2:]) - min(ks[0][2:]), _median(ks[0][2:]) * 1e3 / (n * C),
                            _median(ks[1][2:]), max(ks[1][2:]) - min(ks[1][2:]), _median(ks[1][2:]) * 1e3 / (n * C)))
            lines.append("runs: flac_encode %s; pcm_encode %s" % (" ".join("%.1f" % v for v in ks[0][2:]), " ".join("%.1f" % v for v in ks[1][2:])))
            # the frame kernel alone with and without its CRC-16 (p2phd_flac_encode_stage, a measurement entry), flac_encode's allocations in front
            nf, worst, nwork = flacio.encode_plan(C, 16, n, 4096)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ks = [[], []]
            for _ in range(reps + 2):
                ev[0].record()
                for k, stage in enumerate((1, 2)):
                    stream = torch.empty((worst,), dtype=torch.uint8, device=b.device)
                    lens = torch.empty((nf + 1,), dtype=torch.int64, device=b.device)
                    work = torch.empty((nwork // 8,), dtype=torch.int64, device=b.device)
                    _lib.check(_lib.lib().p2phd_flac_encode_stage(stage, _lib.ptr(b), C, 16, n, rate, 4096, _lib.ptr(stream), worst, _lib.ptr(lens), _lib.ptr(work),
                                                                  nwork, _lib.stream_ptr()), "flac_encode_stage")
                    ev[k + 1].record()
                torch.cuda.synchronize()
                ks[0].append(ev[0].elapsed_time(ev[1]) * 1e3)
                ks[1].append(ev[1].elapsed_time(ev[2]) * 1e3)
                del stream, lens, work
            with_crc, without = _median(ks[0][2:]), _median(ks[1][2:])
            lines.append("by events on %s, %s: flacenc_frames_kernel alone %.1f us (spread %.1f), without its CRC-16 %.1f us (spread %.1f): the parallel CRC is %.1f us = %.1f %% "
                         "of the frame kernel" % (name, tag, with_crc, max(ks[0][2:]) - min(ks[0][2:]), without, max(ks[1][2:]) - min(ks[1][2:]), with_crc - without,
                                                  100.0 * (with_crc - without) / with_crc))
        th = []
        for _ in range(reps):
            t0 = time.perf_counter()
            flacio.encode(pay, C, 16, rate)
            th.append((time.perf_counter() - t0) * 1e3)
        lines.append("on the host, one thread, the clip, %s: p2phd_flac_encode_host median %.3f ms (spread %.3f) = %.1f ns per sample; an hour would be %d times that, %.0f ms"
                     % (tag, _median(th), max(th) - min(th), _median(th) * 1e6 / (L * C), copies, _median(th) * copies))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def run_flaclpc(seconds, reps, log, M):
    """flacout --flac_lpc M: the LPC option of the FLAC writer.  File to file: enhance_file with container 'flac' without the option and
    with flac_lpc=M on one mono and one stereo 16-bit clip, interleaved.  Then, by events, p2phd_flac_encode_lpc (generate.flac_encode
    with lpc_order=M: its allocations in front) beside p2phd_flac_encode on the written payloads, on the clip and on an hour of it,
    and the frame kernel alone (p2phd_flac_encode_lpc_stage beside p2phd_flac_encode_stage); the host encoder on the clip; and the
    streams' sizes at M = 0, 4, 8, 12.  The clips are the synthetic partials of the other modes through an untrained model."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.data import flacio, wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, flac_encode
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py flacout --flac_lpc %d: one %g s clip at %d Hz (%d samples per channel), mono and stereo, pcm16, block size 4096; %d "
             "interleaved repeats" % (M, seconds, rate, x.shape[-1], reps)]
    payloads = {}
    with tempfile.TemporaryDirectory() as tmp:
        sr = SuperResolver(model, opt, overlap=0.25)
        for tag, clip in (("mono", 0.5 * x), ("stereo", torch.cat([0.5 * x, 0.4 * x.flip(-1) + 0.1 * x]))):
            src = os.path.join(tmp, tag + "_in.wav")
            wavio.save(src, clip.cpu(), rate)
            pw, pf = os.path.join(tmp, tag + ".wav"), os.path.join(tmp, tag + ".flac")
            runs = [("%s: container flac          " % tag, lambda: sr.enhance_file(src, pf, channels='all', container='flac')),
                    ("%s: container flac, flac_lpc=%-2d" % (tag, M), lambda: sr.enhance_file(src, pf, channels='all', container='flac', flac_lpc=M))]
            for _, fn in runs:
                fn(); fn()
            torch.cuda.synchronize()
            ts = [[] for _ in runs]
            for _ in range(reps):
                for k, (_, fn) in enumerate(runs):
                    torch.manual_seed(3)
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            for (name, _), tk in zip(runs, ts):
                lines.append("%s  median %8.3f ms   spread %6.3f (%.3f .. %.3f)   runs: %s"
                             % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
            torch.manual_seed(3)
            sr.enhance_file(src, pw, channels='all')
            pay, _ = wavio.read_payload(pw)
            payloads[tag] = (bytes(pay), clip.shape[0])
            sizes = []
            for order in (0, 4, 8, 12):
                torch.manual_seed(3)
                res = sr.enhance_file(src, pf, channels='all', container='flac', flac_lpc=order)
                data = open(pf, "rb").read()
                meta, table = flacio.index_bytes(data)
                assert flacio.decode_frames(data, table, 0, len(table), clip.shape[0]).T.astype("<i2").tobytes() == payloads[tag][0]
                sizes.append("M = %d: %d bytes (%.1f %%)" % (order, res['flac']['bytes'], 100.0 * res['flac']['bytes'] / res['flac']['pcm_bytes']))
            lines.append("%s, the synthetic clip through the untrained model, %d bytes of PCM: %s" % (tag, len(pay), "; ".join(sizes)))
    for tag, (pay, C) in payloads.items():
        dev = torch.frombuffer(bytearray(pay), dtype=torch.uint8).cuda()
        L = len(pay) // (2 * C)
        copies = 3600 * rate // L
        for name, b in (("the clip", dev), ("an hour", dev.repeat(copies))):
            n = b.numel() // (2 * C)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ks = [[], []]
            for _ in range(reps + 2):
                ev[0].record()
                out0 = flac_encode(b, C, 16, rate)
                ev[1].record()
                out1 = flac_encode(b, C, 16, rate, lpc_order=M)
                ev[2].record()
                torch.cuda.synchronize()
                ks[0].append(ev[0].elapsed_time(ev[1]) * 1e3)
                ks[1].append(ev[1].elapsed_time(ev[2]) * 1e3)
                totals = (int(out0[1][-1].item()), int(out1[1][-1].item()))
                del out0, out1
            lines.append("by events on %s, %s (median of %d, allocations in front; %d samples per channel, %d frames): p2phd_flac_encode %.1f us (spread %.1f), %d bytes; "
                         "p2phd_flac_encode_lpc, lpc_order %d, %.1f us (spread %.1f), %d bytes: %.2f times the time, %.3f of the bytes"
                         % (name, tag, reps, n, -(-n // 4096), _median(ks[0][2:]), max(ks[0][2:]) - min(ks[0][2:]), totals[0], M, _median(ks[1][2:]),
                            max(ks[1][2:]) - min(ks[1][2:]), totals[1], _median(ks[1][2:]) / _median(ks[0][2:]), totals[1] / totals[0]))
            lines.append("runs: flac_encode %s; flac_encode lpc_order %d %s" % (" ".join("%.1f" % v for v in ks[0][2:]), M, " ".join("%.1f" % v for v in ks[1][2:])))
            nf, worst, nwork = flacio.encode_plan(C, 16, n, 4096)
            ks = [[], []]
            for _ in range(reps + 2):
                ev[0].record()
                for k in range(2):
                    stream = torch.empty((worst,), dtype=torch.uint8, device=b.device)
                    lens = torch.empty((nf + 1,), dtype=torch.int64, device=b.device)
                    work = torch.empty((nwork // 8,), dtype=torch.int64, device=b.device)
                    if k == 0:
                        _lib.check(_lib.lib().p2phd_flac_encode_stage(1, _lib.ptr(b), C, 16, n, rate, 4096, _lib.ptr(stream), worst, _lib.ptr(lens), _lib.ptr(work), nwork,
                                                                      _lib.stream_ptr()), "flac_encode_stage")
                    else:
                        _lib.check(_lib.lib().p2phd_flac_encode_lpc_stage(1, _lib.ptr(b), C, 16, n, rate, 4096, M, _lib.ptr(stream), worst, _lib.ptr(lens), _lib.ptr(work),
                                                                          nwork, _lib.stream_ptr()), "flac_encode_lpc_stage")
                    ev[k + 1].record()
                torch.cuda.synchronize()
                ks[0].append(ev[0].elapsed_time(ev[1]) * 1e3)
                ks[1].append(ev[1].elapsed_time(ev[2]) * 1e3)
                del stream, lens, work
            lines.append("by events on %s, %s: flacenc_frames_kernel alone %.1f us (spread %.1f), its LPC instantiation at lpc_order %d %.1f us (spread %.1f): %.2f times"
                         % (name, tag, _median(ks[0][2:]), max(ks[0][2:]) - min(ks[0][2:]), M, _median(ks[1][2:]), max(ks[1][2:]) - min(ks[1][2:]),
                            _median(ks[1][2:]) / _median(ks[0][2:])))
        th = [[], []]
        for _ in range(reps):
            for k, order in enumerate((0, M)):
                t0 = time.perf_counter()
                flacio.encode(pay, C, 16, rate, lpc_order=order)
                th[k].append((time.perf_counter() - t0) * 1e3)
        lines.append("on the host, one thread, the clip, %s: p2phd_flac_encode_host median %.3f ms (spread %.3f); p2phd_flac_encode_lpc_host, lpc_order %d, %.3f ms (spread %.3f)"
                     % (tag, _median(th[0]), max(th[0]) - min(th[0]), M, _median(th[1]), max(th[1]) - min(th[1])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def run_normscope(seconds, reps, log, off_only=False):
    """enhance_file on a mono clip, file to file: norm_scope 'group' (an object built without the option) and 'clip', interleaved;
    then p2phd_spectro_range, p2phd_range_fold and p2phd_spectro_encode_given alone, by events, on one group's spectrum beside
    p2phd_spectro_encode_ex on the same tensor."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    rate = int(opt.hr_sampling_rate)
    lines = ["# tools/time_generate.py normscope: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz, file to file, untrained weights, %d interleaved repeats" % (seconds, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, x.cpu(), rate)
        runs = [("no option            ", SuperResolver(model, opt, overlap=0.25))]
        if not off_only:
            runs = [("norm_scope group     ", runs[0][1]), ("norm_scope clip      ", SuperResolver(model, opt, overlap=0.25, norm_scope='clip'))]
        for _, sr in runs:                                          # warm-up: capture, pinned buffers, page cache
            sr.enhance_file(src, out)
            sr.enhance_file(src, out)
        torch.cuda.synchronize()
        ts = [[] for _ in runs]
        for _ in range(reps):
            for k, (_, sr) in enumerate(runs):
                t0 = time.perf_counter()
                sr.enhance_file(src, out)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(runs, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        if not off_only:
            base = _median(ts[0])
            sr = runs[1][1]
            S = -(-x.shape[-1] // int(sr.T * (1 - sr.overlap)))
            lines.append("the option costs %+.3f ms per file (difference of the medians), %+.2f %% of the file without it: about %d segments through "
                         "the transform once more in chunks of %d, one read of each spectrum, one noise fold and one draw of the clip's noise"
                         % (_median(ts[1]) - base, 100.0 * (_median(ts[1]) - base) / base, S, sr.batch))
    text = "\n".join(lines) + "\n"
    if not off_only:
        text += _normscope_kernels(torch, model, opt, x, reps)
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def _normscope_kernels(torch, model, opt, x, reps):
    """The three entries alone, by events, on the spectrum of one group of the clip (and its mask noise) and on 64 such groups in
    one tensor, beside the encode they extend."""
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    T, b = int(opt.segment_length), int(opt.batchSize)
    seg = x[0, :b * T].reshape(b, T).contiguous()
    with torch.no_grad():
        one = model._mdct(seg).contiguous()
    al, mv, st = float(opt.alpha), float(opt.min_value), _lib.stream_ptr()
    lines = []
    for what, k in (("one group", 1), ("64 groups", 64)):
        spec = one.repeat(k, 1, 1).contiguous()
        B, Fr, M = spec.shape
        shape = model.mask_noise_shape(b, T)
        noise = torch.randn((B,) + tuple(shape[1:]), device=spec.device)
        R = shape[2]
        part = torch.empty(L.p2phd_spectro_partials_floats(B, Fr, M), dtype=torch.float32, device=spec.device)
        log, pha = torch.empty((B, 2, M, Fr), device=spec.device), torch.empty((B, 1, M, Fr), device=spec.device)
        norm8 = torch.zeros(8, device=spec.device)
        acc = torch.tensor([float('inf'), float('-inf')] * 4).to(spec.device)
        calls = [("p2phd_spectro_encode_ex", lambda: L.p2phd_spectro_encode_ex(_lib.ptr(spec), B, Fr, M, 2, al, mv, R, 2, _lib.ptr(noise), None,
                                                                               _lib.ptr(log), _lib.ptr(pha), _lib.ptr(norm8), _lib.ptr(part), st)),
                 ("p2phd_spectro_range", lambda: L.p2phd_spectro_range(_lib.ptr(spec), B, Fr, M, 2, al, mv, _lib.ptr(acc), _lib.ptr(part), st)),
                 ("p2phd_range_fold", lambda: L.p2phd_range_fold(_lib.ptr(noise), noise.numel(), _lib.ptr(acc[4:]), _lib.ptr(part), st)),
                 ("p2phd_spectro_encode_given", lambda: L.p2phd_spectro_encode_given(_lib.ptr(spec), B, Fr, M, 2, al, mv, R, 2, _lib.ptr(noise), None,
                                                                                     _lib.ptr(norm8), _lib.ptr(log), _lib.ptr(pha), st))]
        lines.append("kernels alone on %s (events, median of %d): spectrum [%d, %d, %d] f32 = %.2f MB, noise %.2f MB, encoded %.2f MB"
                     % (what, reps, B, Fr, M, spec.numel() * 4e-6, noise.numel() * 4e-6, (log.numel() + pha.numel()) * 4e-6))
        # what each has to move at the least: the encode reads the spectrum and the noise twice and writes, reads and rewrites the planes
        moved = {"p2phd_spectro_encode_ex": spec.numel() + 3 * log.numel() + pha.numel() + 2 * noise.numel(), "p2phd_spectro_range": spec.numel(),
                 "p2phd_range_fold": noise.numel(), "p2phd_spectro_encode_given": spec.numel() + log.numel() + pha.numel() + noise.numel()}
        for name, fn in calls:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            us = []
            for _ in range(reps + 2):
                ev[0].record()
                _lib.check(fn(), name)
                ev[1].record()
                torch.cuda.synchronize()
                us.append(ev[0].elapsed_time(ev[1]) * 1e3)
            m = _median(us[2:])
            lines.append("%-28s %8.1f us (spread %.1f) = %.0f GB/s of the %.2f MB it has to move   runs: %s"
                         % (name, m, max(us[2:]) - min(us[2:]), moved[name] * 4e-3 / m, moved[name] * 4e-6, " ".join("%.1f" % v for v in us[2:])))
        del spec, noise, log, pha, part
    return "\n".join(lines) + "\n"


def run_segnorm(seconds, reps, log):
    """File to file, norm_scope 'group' (an object built without any option), 'clip' and segment_norm, interleaved: enhance_file on
    the mono clip, then enhance_folder on eight two-channel clips of 2 s (four segments a channel: one full group) and of 1.5 s (three:
    the one group of every channel of 'group' and 'clip' runs eagerly); then p2phd_spectro_encode_rows beside p2phd_spectro_encode_ex and p2phd_spectro_encode_given, and the row decode
    beside the plain one, alone, by events, on one group's spectrum."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    rate = int(opt.hr_sampling_rate)
    files, shorts = 8, (2.0, 1.5)
    lines = ["# tools/time_generate.py segnorm: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz, file to file, and folders of %d two-channel clips of %s s, files to files, channels='all'; "
             "untrained weights, %d interleaved repeats" % (seconds, files, " and ".join("%g" % v for v in shorts), reps)]
    runs = [("norm_scope group     ", SuperResolver(model, opt, overlap=0.25)),
            ("norm_scope clip      ", SuperResolver(model, opt, overlap=0.25, norm_scope='clip')),
            ("segment_norm         ", SuperResolver(model, opt, overlap=0.25, segment_norm=True))]
    with tempfile.TemporaryDirectory() as tmp:
        src, out, d_out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav", "out"))
        wavio.save(src, x.cpu(), rate)
        works = [("the %g s mono clip" % seconds, x.shape[-1], 1, lambda sr: sr.enhance_file(src, out))]
        for short in shorts:
            d_in = os.path.join(tmp, "in%g" % short)
            os.makedirs(d_in)
            n = int(short * rate)
            for i in range(files):
                a = x[:, i * 4000:i * 4000 + n]
                wavio.save(os.path.join(d_in, "clip%03d.wav" % i), torch.cat([a, -0.7 * a.flip(-1)]).cpu() * 0.9 ** i, rate)
            works.append(("the folder of %d two-channel clips of %g s" % (files, short), n, 2,
                          lambda sr, d_in=d_in: sr.enhance_folder(d_in, d_out, channels='all')))
        for what, length, C, work in works:
            for _, sr in runs:                                      # warm-up: capture, pinned buffers, page cache
                work(sr)
                work(sr)
            torch.cuda.synchronize()
            ts = [[] for _ in runs]
            for _ in range(reps):
                for k, (_, sr) in enumerate(runs):
                    t0 = time.perf_counter()
                    work(sr)
                    torch.cuda.synchronize()
                    ts[k].append((time.perf_counter() - t0) * 1e3)
            sr = runs[0][1]
            S = segment_plan(length, sr.T, sr.overlap)[0]
            lines.append("%s: %d segments per channel; 'group' and 'clip' walk each channel in %d replayed group%s of %d and %s; segment_norm walks a "
                         "file's %d rows in %d replayed groups, %d filler row%s"
                         % (what, S, S // sr.batch, '' if S // sr.batch == 1 else 's', sr.batch,
                            "one eager group of %d" % (S % sr.batch) if S % sr.batch else "no eager group", C * S, -(-C * S // sr.batch),
                            -C * S % sr.batch, '' if -C * S % sr.batch == 1 else 's'))
            for (name, _), tk in zip(runs, ts):
                lines.append("%s  median %8.3f ms   spread %6.3f (%.3f .. %.3f)   %+7.2f %% against group   runs: %s"
                             % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), 100.0 * (_median(tk) - _median(ts[0])) / _median(ts[0]),
                                " ".join("%.3f" % v for v in tk)))
    text = "\n".join(lines) + "\n" + _segnorm_kernels(torch, model, opt, x, reps)
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def run_stream(seconds, reps, log, long_seconds=600.0, windows=(1.0, 5.0, 30.0)):
    """File to file with SuperResolver(segment_norm=True): enhance_file on the `seconds` s mono clip and on one of `long_seconds` s,
    unstreamed and with stream_seconds of `windows`, interleaved in one process.  Per run: ms per file, the time until the first
    payload is on the host and about to be written (unstreamed: the whole file's, at _save; streamed: the first window's, behind its
    event), and the peak of torch.cuda.max_memory_allocated over the run."""
    import tempfile
    torch, model, opt, x = _setup(max(seconds, long_seconds))
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    rate = int(opt.hr_sampling_rate)
    sr = SuperResolver(model, opt, overlap=0.25, segment_norm=True)
    lines = ["# tools/time_generate.py stream: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed, segment_norm; "
             "mono PCM16 clips at 48 kHz, file to file; untrained weights, %d interleaved repeats" % reps]
    first = [None]
    save, event = sr._save, sr._stream_event

    def saving(*a, **k):
        first[0] = first[0] or time.perf_counter()
        return save(*a, **k)

    class Waited:
        def __init__(self, ev):
            self.ev = ev

        def synchronize(self):
            self.ev.synchronize()
            first[0] = first[0] or time.perf_counter()

    sr._save, sr._stream_event = saving, lambda: Waited(event())
    runs = [None] + list(windows)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.wav")
        for length in (seconds, long_seconds):
            src = os.path.join(tmp, "in%g.wav" % length)
            wavio.save(src, x[:, :int(length * rate)].cpu(), rate)
            work = lambda W: sr.enhance_file(src, out, **({} if W is None else {'stream_seconds': W}))     # noqa: E731
            for W in runs:                                          # warm-up: capture, pinned buffers, page cache
                work(W)
                work(W)
            torch.cuda.synchronize()
            ts, firsts, peaks, info = [[] for _ in runs], [[] for _ in runs], [0] * len(runs), [None] * len(runs)
            for _ in range(reps):
                for j, W in enumerate(runs):
                    torch.cuda.reset_peak_memory_stats()
                    first[0] = None
                    t0 = time.perf_counter()
                    res = work(W)
                    torch.cuda.synchronize()
                    ts[j].append((time.perf_counter() - t0) * 1e3)
                    firsts[j].append((first[0] - t0) * 1e3)
                    peaks[j] = max(peaks[j], torch.cuda.max_memory_allocated())
                    info[j] = res.get('stream')
                    del res
            lines.append("the %g s clip:" % length)
            for j, W in enumerate(runs):
                what = "unstreamed           " if W is None else "stream_seconds %-6g" % W
                shape = "" if info[j] is None else "   %d windows of %d segments, %d groups" % (info[j]['windows'], info[j]['segments_per_window'], info[j]['groups'])
                lines.append("%s  median %9.3f ms   spread %7.3f (%.3f .. %.3f)   %+7.2f %% against unstreamed   first payload after %9.3f ms   "
                             "peak allocated %7.1f MiB%s   runs: %s"
                             % (what, _median(ts[j]), max(ts[j]) - min(ts[j]), min(ts[j]), max(ts[j]), 100.0 * (_median(ts[j]) - _median(ts[0])) / _median(ts[0]),
                                _median(firsts[j]), peaks[j] / 2.0 ** 20, shape, " ".join("%.3f" % v for v in ts[j])))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def run_pack(seconds, reps, log, off_only=False, files=32, clip_seconds=3.0, batch=32):
    """Files to files with SuperResolver(segment_norm=True) at groups of `batch`: enhance_folder on `files` mono clips of
    `clip_seconds` s with pack_files 1, 4, 16 and 32, interleaved in one process; then the ragged gather and stitch alone, by events,
    beside the planar launches they replace on the same clips.  `off_only`: pack_files 1 alone (one process of an alternating
    comparison with another checkout, whose `segnorm` mode times the same path)."""
    import tempfile
    torch, model, opt, x = _setup(max(seconds, clip_seconds + files * 0.1 + 1.0))
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    rate = int(opt.hr_sampling_rate)
    sr = SuperResolver(model, opt, overlap=0.25, batch=batch, segment_norm=True)
    n = int(clip_seconds * rate)
    S = segment_plan(n, sr.T, sr.overlap)[0]
    packs = (1,) if off_only else (1, 4, 16, 32)
    lines = ["# tools/time_generate.py pack: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of %d, overlap 0.25, graphed, segment_norm; a "
             "folder of %d mono PCM16 clips of %g s at 48 kHz (%d rows each), files to files; untrained weights, %d interleaved repeats"
             % (batch, files, clip_seconds, S, reps)]
    with tempfile.TemporaryDirectory() as tmp:
        d_in, d_out = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        os.makedirs(d_in)
        clips = []
        for i in range(files):
            a = x[:, i * 4800:i * 4800 + n] * 0.97 ** i
            clips.append(a.contiguous())
            wavio.save(os.path.join(d_in, "clip%03d.wav" % i), a.cpu(), rate)
        work = lambda k: sr.enhance_folder(d_in, d_out, **({} if k == 1 else {'pack_files': k}))     # noqa: E731
        for k in packs:                                             # warm-up: capture, pinned buffers, page cache
            work(k)
            work(k)
        torch.cuda.synchronize()
        ts = [[] for _ in packs]
        for _ in range(reps):
            for j, k in enumerate(packs):
                t0 = time.perf_counter()
                work(k)
                torch.cuda.synchronize()
                ts[j].append((time.perf_counter() - t0) * 1e3)
    for k, tk in zip(packs, ts):
        groups = sum(-(-min(k, files - f0) * S // batch) for f0 in range(0, files, k))
        lines.append("pack_files %2d  %3d groups of %d for %d rows  median %9.3f ms   spread %7.3f (%.3f .. %.3f)   %+7.2f %% against pack_files 1   runs: %s"
                     % (k, groups, batch, files * S, _median(tk), max(tk) - min(tk), min(tk), max(tk), 100.0 * (_median(tk) - _median(ts[0])) / _median(ts[0]),
                        " ".join("%.3f" % v for v in tk)))
    text = "\n".join(lines) + "\n" + ("" if off_only else _pack_kernels(torch, sr, clips, reps))
    sys.stdout.write(text)
    if log:
        os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
        with open(log, "w") as f:
            f.write(text)


def _pack_kernels(torch, sr, clips, reps):
    """The ragged gather and stitch of all clips in one launch each beside the planar launches, one per clip, that they replace:
    by events around the whole of either, host work of the wrappers included -- what the stream sees."""
    from pix2pixhdaudiosr_amd.generate import segment_plan, segments_gather_planar, segments_gather_ragged, segments_stitch_planar, segments_stitch_ragged
    T = sr.T
    S, stride, _ = segment_plan(clips[0].shape[-1], T, sr.overlap)
    lengths, counts = [c.shape[-1] for c in clips], [c.shape[0] for c in clips]
    seg = segments_gather_ragged(clips, T, stride, [S] * len(clips))
    calls = [("gather, ragged: 1 launch", lambda: segments_gather_ragged(clips, T, stride, [S] * len(clips))),
             ("gather, planar: %d launches" % len(clips), lambda: [segments_gather_planar(c, T, stride, S) for c in clips]),
             ("stitch, ragged: 1 launch", lambda: segments_stitch_ragged(seg, lengths, counts, stride, sr.gain)),
             ("stitch, planar: %d launches" % len(clips), lambda: [segments_stitch_planar(seg[i * S:(i + 1) * S], 1, stride, sr.gain, lengths[i])
                                                                    for i in range(len(clips))])]
    moved = 4e-6 * (sum(lengths) + seg.numel())
    lines = ["the row ends alone on the %d clips (events, median of %d): %d rows of %d = %.2f MB of segments, %.2f MB of clips" % (len(clips), reps, seg.shape[0], T, seg.numel() * 4e-6, sum(lengths) * 4e-6)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for name, fn in calls:
        us = []
        for _ in range(reps + 2):
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            us.append(ev[0].elapsed_time(ev[1]) * 1e3)
        m = _median(us[2:])
        lines.append("%-28s %8.1f us (spread %.1f) = %.0f GB/s of the %.2f MB it has to move   runs: %s"
                     % (name, m, max(us[2:]) - min(us[2:]), moved * 1e3 / m, moved, " ".join("%.1f" % v for v in us[2:])))
    return "\n".join(lines) + "\n"


def _segnorm_kernels(torch, model, opt, x, reps):
    """The row encode beside the encodes it stands in for and the row decode beside the plain one, alone, by events, on the spectrum
    of one group of the clip (and its mask noise)."""
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    T, b = int(opt.segment_length), int(opt.batchSize)
    seg = x[0, :b * T].reshape(b, T).contiguous()
    with torch.no_grad():
        spec = model._mdct(seg).contiguous()
    al, mv, st = float(opt.alpha), float(opt.min_value), _lib.stream_ptr()
    B, Fr, M = spec.shape
    shape = model.mask_noise_shape(b, T)
    noise = torch.randn(shape, device=spec.device)
    R = shape[2]
    part = torch.empty(L.p2phd_spectro_partials_floats(B, Fr, M), dtype=torch.float32, device=spec.device)
    ws = torch.empty(L.p2phd_spectro_rows_partials_floats(B, Fr, M), dtype=torch.float32, device=spec.device)
    log, pha = torch.empty((B, 2, M, Fr), device=spec.device), torch.empty((B, 1, M, Fr), device=spec.device)
    back = torch.empty((B, Fr, M), device=spec.device)
    norm8, rows = torch.zeros(8, device=spec.device), torch.zeros((B, 8), device=spec.device)
    keep = M - R
    calls = [("p2phd_spectro_encode_ex", lambda: L.p2phd_spectro_encode_ex(_lib.ptr(spec), B, Fr, M, 2, al, mv, R, 2, _lib.ptr(noise), None,
                                                                           _lib.ptr(log), _lib.ptr(pha), _lib.ptr(norm8), _lib.ptr(part), st)),
             ("p2phd_spectro_encode_given", lambda: L.p2phd_spectro_encode_given(_lib.ptr(spec), B, Fr, M, 2, al, mv, R, 2, _lib.ptr(noise), None,
                                                                                 _lib.ptr(norm8), _lib.ptr(log), _lib.ptr(pha), st)),
             ("p2phd_spectro_encode_rows", lambda: L.p2phd_spectro_encode_rows(_lib.ptr(spec), B, Fr, M, 2, al, mv, R, 2, _lib.ptr(noise), None,
                                                                               _lib.ptr(rows), _lib.ptr(log), _lib.ptr(pha), _lib.ptr(ws), st)),
             ("p2phd_spectro_decode_signed", lambda: L.p2phd_spectro_decode_signed(_lib.ptr(log), _lib.ptr(pha), _lib.ptr(norm8), B, Fr, M, 2, keep, mv,
                                                                                   1.0, _lib.ptr(back), st)),
             ("p2phd_spectro_decode_signed_rows", lambda: L.p2phd_spectro_decode_signed_rows(_lib.ptr(log), _lib.ptr(pha), _lib.ptr(rows), B, Fr, M, 2,
                                                                                             keep, mv, 1.0, _lib.ptr(back), st))]
    lines = ["kernels alone on one group (events, median of %d): spectrum [%d, %d, %d] f32 = %.2f MB, noise %.2f MB, encoded %.2f MB; the row "
             "encode's workspace %d floats" % (reps, B, Fr, M, spec.numel() * 4e-6, noise.numel() * 4e-6, (log.numel() + pha.numel()) * 4e-6, ws.numel())]
    # what each has to move at the least: the encode reads the spectrum and the noise twice and writes, reads and rewrites the planes;
    # the row encode reads the spectrum and the noise twice and writes the planes once
    enc = spec.numel() + log.numel() + pha.numel() + noise.numel()
    dec = log.numel() + pha.numel() + back.numel()
    moved = {"p2phd_spectro_encode_ex": spec.numel() + 3 * log.numel() + pha.numel() + 2 * noise.numel(), "p2phd_spectro_encode_given": enc,
             "p2phd_spectro_encode_rows": enc + spec.numel() + noise.numel(), "p2phd_spectro_decode_signed": dec, "p2phd_spectro_decode_signed_rows": dec}
    for name, fn in calls:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        us = []
        for _ in range(reps + 2):
            ev[0].record()
            _lib.check(fn(), name)
            ev[1].record()
            torch.cuda.synchronize()
            us.append(ev[0].elapsed_time(ev[1]) * 1e3)
        m = _median(us[2:])
        lines.append("%-34s %8.1f us (spread %.1f) = %.0f GB/s of the %.2f MB it has to move   runs: %s"
                     % (name, m, max(us[2:]) - min(us[2:]), moved[name] * 4e-3 / m, moved[name] * 4e-6, " ".join("%.1f" % v for v in us[2:])))
    return "\n".join(lines) + "\n"


def run_limiter(seconds, reps, log):
    """enhance_file, file to file, at a loudness target that leaves the true peak 4 dB over a -1 dBTP ceiling: no output option, the
    guard alone, the limiter in front of the guard -- the same object, the same input, interleaved; what the two written files
    measure; then the limiter's two kernels and the true-peak kernel alone on the same clip."""
    import tempfile
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import (SuperResolver, limiter_apply, limiter_envelope, limiter_plan, loudness, loudness_channel_weights,
                                               true_peaks, truepeak_plan)
    n = x.shape[-1]
    g = torch.Generator().manual_seed(8)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    hi = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.02, 5200.0, 0.3), (0.01, 9100.0, 1.1), (0.005, 15300.0, 2.2)))
    hr = x.cpu() + (hi + 0.001 * torch.randn(n, generator=g, dtype=torch.float64)).float()[None]      # as the true-peak run's original
    sr = SuperResolver(model, opt, overlap=0.25)
    rate = int(opt.hr_sampling_rate)
    plan, lplan = truepeak_plan(rate), limiter_plan(rate)
    ceiling_db = -1.0
    lines = ["# tools/time_generate.py limiter: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; one "
             "%g s mono PCM16 clip at 48 kHz with a full-band original, file to file, untrained weights, %d interleaved repeats" % (seconds, reps),
             "# true-peak plan: factor %d, %d taps per phase, beta %g; limiter plan: look-ahead %d, hold %d samples; ceiling %+g dBTP"
             % (plan['factor'], plan['taps_per_phase'], plan['beta'], lplan['lookahead'], lplan['hold'], ceiling_db)]

    def written_loudness(path):
        y, _ = wavio.load(path)
        return float(loudness(y.cuda().contiguous(), rate, loudness_channel_weights(y.shape[0]))[0][0])

    with tempfile.TemporaryDirectory() as tmp:
        src, out = (os.path.join(tmp, f) for f in ("in.wav", "out.wav"))
        wavio.save(src, hr, rate)
        torch.manual_seed(99)
        first = sr.enhance_file(src, None, loudness='report', true_peak=True)
        target = min(0.0, first['loudness']['measured'] + (ceiling_db + 4.0) - max(first['output']['true_peak_dbtp']))
        lines.append("the generated clip: %.3f LUFS, true peak %+.3f dBTP; loudness target %.3f LUFS"
                     % (first['loudness']['measured'], max(first['output']['true_peak_dbtp']), target))
        stage = dict(loudness=target, clip='guard', ceiling_dbfs=ceiling_db)
        variants = (("no output option      ", {}), ("loudness, guard alone ", dict(stage, true_peak=True)), ("loudness, limiter     ", dict(stage, limiter=True)))
        results, levels = [], []
        for _, kw in variants:                                     # warm-up: capture, pinned buffers, page cache; one noise seed
            sr.enhance_file(src, out, **kw)
            torch.manual_seed(99)
            results.append(sr.enhance_file(src, out, **kw))
            levels.append(written_loudness(out))
        torch.cuda.synchronize()
        ts = [[] for _ in variants]
        for _ in range(reps):
            for k, (_, kw) in enumerate(variants):
                t0 = time.perf_counter()
                sr.enhance_file(src, out, **kw)
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        for (name, _), tk in zip(variants, ts):
            lines.append("%s  median %8.3f ms per file   spread %6.3f (%.3f .. %.3f)   runs: %s"
                         % (name, _median(tk), max(tk) - min(tk), min(tk), max(tk), " ".join("%.3f" % v for v in tk)))
        lines.append("the limiter costs %.3f ms per file over the guard alone (difference of the medians), %.2f %% of the file without an output option"
                     % (_median(ts[2]) - _median(ts[1]), 100.0 * (_median(ts[2]) - _median(ts[1])) / _median(ts[0])))
        og, ol = results[1]['output'], results[2]['output']
        lim = ol['limiter']
        lines.append("guard alone:  true peak %+.3f dBTP, gain %.6f; written %.3f LUFS (target %.3f)" % (og['true_peak_dbtp'][0], og['gain'], levels[1], target))
        lines.append("limiter:      true peak in %+.3f dBTP, %+.3f dB at most, %d of %d samples (%.1f %%); limited clip %+.5f dBTP: residual overshoot "
                     "%+.5f dB, residual gain %.7f; written %.3f LUFS: %.3f dB above the guard's"
                     % (lim['input_true_peak_dbtp'], lim['max_reduction_db'], lim['limited_samples'], n, 100.0 * lim['limited_samples'] / n,
                        ol['true_peak_dbtp'][0], ol['true_peak_dbtp'][0] - ceiling_db, ol['gain'], levels[2], levels[2] - levels[1]))
        # the kernels alone, by events, on the clip of the last run behind the loudness gain (one row)
        clip = results[2]['sr'].contiguous()
        ceiling = 10.0 ** (ceiling_db / 20.0)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        k_env, k_app, k_true = [], [], []
        for _ in range(reps + 2):
            ev[0].record()
            r, _ = limiter_envelope(clip, rate, ceiling)
            ev[1].record()
            limiter_apply(clip, r, lplan, want_g=False)
            ev[2].record()
            true_peaks(clip, rate)
            ev[3].record()
            torch.cuda.synchronize()
            k_env.append(ev[0].elapsed_time(ev[1]) * 1e3)
            k_app.append(ev[1].elapsed_time(ev[2]) * 1e3)
            k_true.append(ev[2].elapsed_time(ev[3]) * 1e3)
        L = clip.shape[-1]
        fmas = L * (lplan['lookahead'] + 1)
        lines.append("kernels alone (events, median of %d, each with the allocation of its results in front): p2phd_limiter_envelope %.1f us, "
                     "p2phd_limiter_apply %.1f us (%d samples, %.0f M fma in the curve where no tile is skipped: %.2f Gfma/s), p2phd_truepeak %.1f us"
                     % (reps, _median(k_env[2:]), _median(k_app[2:]), L, fmas * 1e-6, fmas / _median(k_app[2:]) * 1e-3, _median(k_true[2:])))
        lines.append("runs: envelope %s; apply %s; truepeak %s" % tuple(" ".join("%.1f" % v for v in k[2:]) for k in (k_env, k_app, k_true)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write(text)


def _run_variants(seconds, reps, log, mode, variants):
    torch, model, opt, x = _setup(seconds)
    from pix2pixhdaudiosr_amd.data.audio_dataset import lr_round_trip
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    from pix2pixhdaudiosr_amd.util import util as U
    n = x.shape[-1]
    g = torch.Generator().manual_seed(8)
    t = torch.arange(n, dtype=torch.float64) / opt.hr_sampling_rate
    # the full-band original: the band-limited clip plus partials and noise above the low rate's 4 kHz
    hi = sum(a * torch.sin(2 * torch.pi * f * t + p) for a, f, p in ((0.02, 5200.0, 0.3), (0.01, 9100.0, 1.1), (0.005, 15300.0, 2.2)))
    hr = x + (hi + 0.001 * torch.randn(n, generator=g, dtype=torch.float64)).float().cuda()[None]
    lr = lr_round_trip(hr, opt.hr_sampling_rate, opt.lr_sampling_rate, opt.hr_sampling_rate)[..., :n].contiguous()
    srs = [SuperResolver(model, opt, overlap=0.25, **kw) for _, kw in variants]
    lines = ["# tools/time_generate.py %s: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, overlap 0.25, graphed; "
             "%g s synthetic clip at 48 kHz, untrained weights, %d interleaved repeats" % (mode, seconds, reps)]
    for sr in srs:
        if sr.crossover_plan is not None:
            lines.append("# crossover plan: %d taps, the input below %g Hz" % (sr.crossover_plan[0], sr.crossover_plan[1] * opt.hr_sampling_rate))
    outs = []
    for sr in srs:                                                 # warm-up and capture; the same noise seed for every variant
        sr.enhance_lr(lr)
        torch.manual_seed(99)
        outs.append(sr.enhance_lr(lr))
    torch.cuda.synchronize()
    ts = [[] for _ in srs]
    for _ in range(reps):
        for k, sr in enumerate(srs):
            t0 = time.perf_counter()
            sr.enhance_lr(lr)
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    for (name, _), tk, y in zip(variants, ts, outs):
        rates = sorted(seconds / v for v in tk)
        e = U.compute_matrics_ext(hr, lr, y, opt)[0]
        lines.append("%s best %8.1f s of audio / s   spread %6.1f (worst %8.1f)   lsd_lf %.4f  lsd_hf %.4f  lsd %.4f   runs: %s"
                     % (name, rates[-1], rates[-1] - rates[0], rates[0], e['lsd_lf'], e['lsd_hf'], e['lsd'],
                        " ".join("%.1f" % (seconds / v) for v in tk)))
    if mode == "crossover":
        # both outputs come from one noise seed, so their difference is the crossover's work alone: where it sits in the spectrum
        plan = srs[1].crossover_plan
        rate, half = float(opt.hr_sampling_rate), opt.lr_sampling_rate / 2.0
        width = (90.0 - 7.95) * rate / (14.36 * (plan[0] - 1))
        c0 = (plan[0] - 1) // 2
        Y0, Y1 = (torch.fft.rfft(y[0, c0:n - c0].double()) for y in outs)
        f = torch.arange(Y0.numel(), device=Y0.device, dtype=torch.float64) * rate / (n - 2 * c0)
        for name, band in (("below %g Hz" % (plan[1] * rate - width / 2), f <= plan[1] * rate - width / 2), ("above %g Hz" % half, f >= half)):
            moved, was = (Y1 - Y0)[band].abs().pow(2).sum().item(), Y0[band].abs().pow(2).sum().item()
            lines.append("energy of (crossover input - crossover off) %-14s %8.2f dB of that band of crossover off" % (name + ":", 10.0 * torch.log10(torch.tensor(moved / was)).item()))
    e = U.compute_matrics_ext(hr, lr, lr, opt)[0]
    lines.append("the input itself as output                                                                lsd_lf %.4f  lsd_hf %.4f  lsd %.4f"
                 % (e['lsd_lf'], e['lsd_hf'], e['lsd']))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(log)), exist_ok=True)
    with open(log, "w") as f:
        f.write(text)


def run_mode(mode, seconds, reps):
    torch, model, opt, lr = _setup(seconds)
    from pix2pixhdaudiosr_amd.generate import SuperResolver, segment_plan
    if mode == "hand":
        dt = _time(torch, _hand(torch, model, opt, lr), reps)
        print(f"hand-composed loop    overlap 0     {seconds / dt:8.1f} s of audio / s   ({dt * 1e3:.3f} ms for {seconds:g} s, best of {reps})")
    elif mode in ("eager", "graphed"):
        for overlap in (0.0, 0.25):
            sr = SuperResolver(model, opt, overlap=overlap, graph=mode == "graphed")
            dt = _time(torch, lambda: sr.enhance_lr(lr), reps)
            S = segment_plan(lr.shape[-1], opt.segment_length, overlap)[0]
            print(f"pipeline {mode:8s}     overlap {overlap:<5g} {seconds / dt:8.1f} s of audio / s   ({dt * 1e3:.3f} ms, {S} segments, best of {reps})")
    elif mode == "seams":
        for overlap in (0.0, 0.25):
            S, stride, V = segment_plan(lr.shape[-1], opt.segment_length, overlap)
            torch.manual_seed(99)
            y = SuperResolver(model, opt, overlap=overlap).enhance_lr(lr)[0].double()
            d = y[1:] - y[:-1]                                      # d[n - 1] = y[n] - y[n - 1]
            joins = torch.arange(1, S, device=y.device) * stride
            joins = joins[joins < y.numel()]
            at = d[joins - 1].pow(2).mean().sqrt().item()
            allrms = d.pow(2).mean().sqrt().item()
            print(f"seams  overlap {overlap:<5g} {len(joins)} joins: first-difference RMS at the joins {at:.4e}, whole clip {allrms:.4e}, ratio {at / allrms:.3f}")
    else:
        raise SystemExit("unknown mode " + mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default=None, choices=list(LIMITS) + ["folder", "lowband", "crossover", "spectrogram", "loudness", "truepeak", "limiter", "album", "bandwidth", "stereo", "rateconv", "normscope", "segnorm", "pack", "stream", "dither", "flac", "flacout", "wavcodec", "containers", "speechlevel"])
    ap.add_argument("--files", type=int, default=8, help="folder and album mode: stereo clips in the folder")
    ap.add_argument("--album_log", default=os.path.join(ROOT, "profiles", "time_generate_album.log"))
    ap.add_argument("--folder_log", default=os.path.join(ROOT, "profiles", "time_generate_folder.log"))
    ap.add_argument("--lowband_log", default=os.path.join(ROOT, "profiles", "time_generate_lowband.log"))
    ap.add_argument("--crossover_log", default=os.path.join(ROOT, "profiles", "time_generate_crossover.log"))
    ap.add_argument("--spectrogram_log", default=os.path.join(ROOT, "profiles", "time_generate_spectrogram.log"))
    ap.add_argument("--loudness_log", default=os.path.join(ROOT, "profiles", "time_generate_loudness.log"))
    ap.add_argument("--loudness_range", action="store_true", help="loudness mode: time loudness_range=True against loudness='report' and off")
    ap.add_argument("--loudness_range_log", default=os.path.join(ROOT, "profiles", "time_generate_loudness_range.log"))
    ap.add_argument("--truepeak_log", default=os.path.join(ROOT, "profiles", "time_generate_truepeak.log"))
    ap.add_argument("--limiter_log", default=os.path.join(ROOT, "profiles", "time_generate_limiter.log"))
    ap.add_argument("--bandwidth_log", default=os.path.join(ROOT, "profiles", "time_generate_bandwidth.log"))
    ap.add_argument("--stereo_log", default=os.path.join(ROOT, "profiles", "time_generate_stereo.log"))
    ap.add_argument("--rateconv_log", default=os.path.join(ROOT, "profiles", "time_generate_rateconv.log"))
    ap.add_argument("--speechlevel_log", default=os.path.join(ROOT, "profiles", "time_generate_speechlevel.log"))
    ap.add_argument("--normscope_log", default=os.path.join(ROOT, "profiles", "time_generate_norm_scope.log"))
    ap.add_argument("--segnorm_log", default=os.path.join(ROOT, "profiles", "time_generate_segment_norm.log"))
    ap.add_argument("--pack_log", default=os.path.join(ROOT, "profiles", "time_generate_pack.log"))
    ap.add_argument("--stream_log", default=os.path.join(ROOT, "profiles", "time_generate_stream.log"))
    ap.add_argument("--dither_log", default=os.path.join(ROOT, "profiles", "time_generate_dither.log"))
    ap.add_argument("--flac_log", default=os.path.join(ROOT, "profiles", "time_generate_flac.log"))
    ap.add_argument("--wavcodec_log", default=os.path.join(ROOT, "profiles", "time_generate_wavcodec.log"))
    ap.add_argument("--containers_log", default=os.path.join(ROOT, "profiles", "time_generate_containers.log"))
    ap.add_argument("--flacout_log", default=os.path.join(ROOT, "profiles", "time_generate_flacout.log"))
    ap.add_argument("--flac_lpc", type=int, default=None, metavar="N", help="flacout mode: time the LPC option at order N against the writer without it (log in --flaclpc_log)")
    ap.add_argument("--flaclpc_log", default=os.path.join(ROOT, "profiles", "time_generate_flaclpc.log"))
    ap.add_argument("--off_only", action="store_true", help="bandwidth, dither, normscope, rateconv, speechlevel and stereo mode: time only the run without any option (no log unless the mode's log is given)")
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--reps", type=int, default=None, help="repeats (default 5; album, bandwidth, dither, normscope, rateconv, speechlevel and stereo mode: 9)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "time_generate.log"))
    a = ap.parse_args()
    if a.mode == "flacout" and a.flac_lpc is not None:
        return run_flaclpc(a.seconds, 9 if a.reps is None else a.reps, a.flaclpc_log, a.flac_lpc)
    if a.mode == "flacout":
        return run_flacout(a.seconds, 9 if a.reps is None else a.reps, a.flacout_log)
    if a.mode == "containers":
        return run_containers(a.seconds, 9 if a.reps is None else a.reps, a.containers_log)
    if a.mode == "wavcodec":
        return run_wavcodec(a.seconds, 9 if a.reps is None else a.reps, a.wavcodec_log)
    if a.mode == "flac":
        return run_flac(a.seconds, 9 if a.reps is None else a.reps, a.flac_log)
    if a.mode == "album":
        return run_album(a.seconds, 9 if a.reps is None else a.reps, a.files, a.album_log)
    if a.mode == "stereo":
        log = a.stereo_log if not a.off_only or "--stereo_log" in sys.argv else None
        return run_stereo(a.seconds, 9 if a.reps is None else a.reps, log, a.off_only)
    if a.mode == "rateconv":
        log = a.rateconv_log if not a.off_only or "--rateconv_log" in sys.argv else None
        return run_rateconv(a.seconds, 9 if a.reps is None else a.reps, log, a.off_only)
    if a.mode == "speechlevel":
        log = a.speechlevel_log if not a.off_only or "--speechlevel_log" in sys.argv else None
        return run_speechlevel(a.seconds, 9 if a.reps is None else a.reps, log, a.off_only)
    if a.mode == "dither":
        log = a.dither_log if not a.off_only or "--dither_log" in sys.argv else None
        return run_dither(a.seconds, 9 if a.reps is None else a.reps, log, a.off_only)
    if a.mode == "pack":
        log = a.pack_log if not a.off_only or "--pack_log" in sys.argv else None
        return run_pack(a.seconds, 9 if a.reps is None else a.reps, log, a.off_only)
    if a.mode == "stream":
        return run_stream(a.seconds, 9 if a.reps is None else a.reps, a.stream_log)
    if a.mode == "segnorm":
        return run_segnorm(a.seconds, 9 if a.reps is None else a.reps, a.segnorm_log)
    if a.mode == "normscope":
        log = a.normscope_log if not a.off_only or "--normscope_log" in sys.argv else None
        return run_normscope(a.seconds, 9 if a.reps is None else a.reps, log, a.off_only)
    if a.mode == "bandwidth":
        log = a.bandwidth_log if not a.off_only or "--bandwidth_log" in sys.argv else None
        return run_bandwidth(a.seconds, 9 if a.reps is None else a.reps, log, a.off_only)
    if a.reps is None:
        a.reps = 5
    if a.mode == "folder":
        return run_folder(a.seconds, a.reps, a.files, a.folder_log)
    if a.mode == "lowband":
        return run_lowband(a.seconds, a.reps, a.lowband_log)
    if a.mode == "crossover":
        return run_crossover(a.seconds, a.reps, a.crossover_log)
    if a.mode == "spectrogram":
        return run_spectrogram(a.seconds, a.reps, a.spectrogram_log)
    if a.mode == "loudness":
        if a.loudness_range:
            return run_loudness(a.seconds, a.reps, a.loudness_range_log, ranged=True)
        return run_loudness(a.seconds, a.reps, a.loudness_log)
    if a.mode == "truepeak":
        return run_truepeak(a.seconds, a.reps, a.truepeak_log)
    if a.mode == "limiter":
        return run_limiter(a.seconds, a.reps, a.limiter_log)
    if a.mode is not None:
        return run_mode(a.mode, a.seconds, a.reps)
    lines = ["# tools/time_generate.py: G3L2 ngf 48, n_fft 512 MDCT2, segment 32512, bf16, groups of 4, %g s synthetic clip at 48 kHz" % a.seconds]
    for mode, limit in LIMITS.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), mode, "--seconds", str(a.seconds), "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{mode}: no result within {limit} s")
            break
        out = [l for l in p.stdout.splitlines() if l.startswith(("hand", "pipeline", "seams"))]
        lines += out
        if p.returncode != 0:
            lines.append(f"{mode}: exit status {p.returncode}: {p.stderr.strip().splitlines()[-1] if p.stderr.strip() else ''}")
            break
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.log, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
