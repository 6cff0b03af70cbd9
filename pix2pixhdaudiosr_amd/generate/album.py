"""Whole-file generation: the folder pipeline of loudness_scope='folder' -- the folder is one programme (EBU R 128 album
normalisation): one integrated loudness over the 400 ms blocks of every file, one loudness gain and one guard gain for all of them,
so the level differences between the files survive.  Three phases: every file is generated and measured (A), the folder's figures
are found and brought back behind one synchronisation (B), every file is encoded with the folder's gains and written (C).
What a file goes through in phase A is the per-file flow's own front and metrics stage, and its record is built and filled by the
functions the per-file scope uses (generate/resolver.py), and it is written through the file path's own functions
(generate/fileio.py); only what the folder has to itself is written here."""
import math

import torch

from .ops import (_loudness_views, _pcm_peaks_packed, _true_peaks_packed, loudness_blocks, loudness_gate, loudness_gate_blocks, loudness_hops,
                  pcm_encode)
from .plans import loudness_channel_weights
from .resolver import _set


class _Blocks:
    """A grow-only float64 buffer on the device that takes the block powers of one file behind the other's."""

    def __init__(self, device):
        self.buf, self.used = torch.empty((4096,), dtype=torch.float64, device=device), 0

    def take(self, n):
        """-> the next `n` elements, to be written by the caller."""
        if self.used + n > self.buf.numel():
            grown = torch.empty((max(2 * self.buf.numel(), self.used + n),), dtype=torch.float64, device=self.buf.device)
            grown[:self.used].copy_(self.buf[:self.used])
            self.buf = grown
        self.used += n
        return self.buf[self.used - n:self.used]

    def filled(self):
        return self.buf[:self.used]


def enhance_album(sr, plan, written_from, is_lr_input, channels, encoding, seed, report, extended_metrics, o, dither_seed, verify_input=False):
    """enhance_folder with loudness_scope='folder' -> its records.  `sr`: the SuperResolver; `plan`: plan_folder's; `written_from`:
    None, or the output folder where a record gains 'written'; `o`: the validated options as enhance_folder holds them, o.album
    being check_loudness_scope's result; `verify_input`: enhance_file's, per FLAC file.  A file goes through the front and the
    metrics stage of the per-file flow (SuperResolver._front, ._metrics) and leaves the record the per-file scope leaves."""
    stage, tp, loud, album = o.stage, o.tp, o.loud, o.album
    rate = int(sr.opt.hr_sampling_rate)
    scaled = loud['mode'] != 'report'
    guard = stage is not None and stage['clip'] == 'guard'
    blocks_in, blocks_out = _Blocks(sr.device), _Blocks(sr.device)
    entries, kept_bytes = [], 0

    # -- A: generate and measure every file; keep its clip ---------------------------------------------
    for k, (rel, path_in, path_out) in enumerate(plan):
        rec = sr._blank_record(rel, path_out, written_from, extended_metrics, o)
        entry = {'rec': rec, 'k': k, 'path_out': path_out, 'clip': None}
        entries.append(entry)
        read = sr._open(path_in, channels, verify_input, o, rec)
        if read is None:
            continue
        if seed is not None:
            torch.manual_seed(int(seed))
        f = sr._front(read, is_lr_input, channels, encoding, o, "enhance_folder")
        sr._metrics(f, extended_metrics)
        lr, clip = f.lr, f.clip
        sr._fill_record(rec, {'info': f.meta, 'sr': clip, 'metrics': f.metrics, 'metrics_ext': f.ext, 'crossover': f.crossover, 'norm': f.norm})
        # the track's own figures, and its blocks into the folder's two buffers: six launches of the family "loudness"
        weights = loudness_channel_weights(clip.shape[0])
        track = entry['track'] = torch.empty((80,), dtype=torch.uint8, device=clip.device)
        z_in, z_out = loudness_hops(lr, rate), loudness_hops(clip, rate)
        loudness_gate(z_in, rate, weights, out=track[:40])
        loudness_gate(z_out, rate, weights, out=track[40:])
        loudness_blocks(z_in, rate, weights, out=blocks_in.take(max(z_in.shape[1] - 3, 0)))
        loudness_blocks(z_out, rate, weights, out=blocks_out.take(max(z_out.shape[1] - 3, 0)))
        nbytes = clip.numel() * clip.element_size()
        if kept_bytes + nbytes <= album['cache_bytes']:
            kept_bytes += nbytes
            entry['clip'] = clip.contiguous()
        else:
            entry['clip'] = clip.cpu()                                      # waits on the host until its turn comes
    done = [e for e in entries if e['rec']['error'] is None]

    # -- B: the folder's loudness, its one gain, every file's peaks, the one guard gain; one synchronisation ------------
    if done:
        total = torch.empty((80,), dtype=torch.uint8, device=sr.device)
        res_in, _ = loudness_gate_blocks(blocks_in.filled(), out=total[:40])
        wanted = {'report': {}, 'input': {'target_dev': res_in}, 'target': {'target': loud['target']}}[loud['mode']]
        _, gain = loudness_gate_blocks(blocks_out.filled(), max_gain_db=loud['max_gain_db'], out=total[40:], **wanted)
        pieces, guards = [total], []
        for e in done:
            w = _on_device(sr, e, gain if scaled else None)
            pieces.append(e.pop('track'))
            if stage is not None:
                (_, _, _, g), packed = _pcm_peaks_packed(w, encoding, stage['ceiling'], "enhance_folder")
                pieces.append(packed)
                if tp is not None:
                    (_, g), packed = _true_peaks_packed(w, tp['rate'], tp['ceiling'], "enhance_folder")
                    pieces.append(packed)
                guards.append(g)
            if e['clip'].is_cuda:
                e['clip'] = w                                               # (a clip that waits on the host is scaled again in phase C)
        # a file's guard gain is ceiling / peak where the peak is over the ceiling and 1 elsewhere (csrc/pcm.hip, csrc/truepeak.hip):
        # it does not grow with the peak, so the smallest of them is the gain of the folder's largest peak, bit for bit
        guard_gain = torch.cat(guards).min().reshape(1) if guards else None
        if guard_gain is not None:
            pieces.append(guard_gain.view(torch.uint8))
        flat = torch.cat(pieces)
        host = sr._pinned('album', flat.numel())[:flat.numel()]
        host.copy_(flat, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        _fill_records(done, host, loud, stage, tp, scaled, bool(guards), (blocks_in.used, blocks_out.used))

    # -- C: clip 'error' for the whole folder first, then encode and write ------------------------------------
    for e in done:
        if stage is not None:
            output = sr._output(e.pop('peaks'), e['rec']['written_channels'], stage, e['path_out'], encoding,
                                **_set(true_peak=tp and dict(tp, packed=e.pop('tpeaks'))))
            output['gain'] = e.pop('guard') if guard else 1.0
            e['rec']['output'] = output
    records = []
    for e in entries:
        rec = e['rec']
        if rec['error'] is None:
            w = _on_device(sr, e, gain if scaled and not e['clip'].is_cuda else None)
            if stage is None:
                dev = pcm_encode(w, encoding)
            else:
                dev = pcm_encode(w, encoding, gain=guard_gain if guard else None, dither=stage['dither'], seed=dither_seed + e['k'],
                                 curve=stage.get('curve'), chunk=stage.get('chunk'))
            flac = o.flac and dict(o.flac)                                  # (one file's, as in the per-file flow)
            extra = {}
            if flac is not None:
                dev, extra = sr._flac_stage(dev, w.shape[0], encoding, flac)
            payload, _ = sr._fetch(dev, None, **extra)
            sr._save(e['path_out'], payload, w.shape[0], encoding, **_set(flac=flac))
            if flac is not None:
                rec['flac'] = flac['result']
            e['clip'] = None
        records.append(rec)
        if report is not None:
            report(rec)
    return records


def _on_device(sr, entry, gain):
    """The kept clip of `entry` on the device, times `gain` (the file path's own expression) where one is given."""
    w = entry['clip'] if entry['clip'].is_cuda else entry['clip'].to(sr.device)
    return w if gain is None else (w * gain).contiguous()


def _fill_records(done, host, loud, stage, tp, scaled, guarded, blocks):
    """The fetched bytes of phase B -> every record's 'loudness' and 'album'; the peak buffers and the guard gain stay with the
    entries for phase C.  `blocks`: the block counts of the folder's two buffers."""
    at = [0]

    def cut(n):                                                             # (a copy: typed views need the alignment of a fresh tensor)
        at[0] += n
        return host[at[0] - n:at[0]].clone()

    (res_in, _), (res_out, gain) = _loudness_views(cut(40)), _loudness_views(cut(40))
    level_in, measured = float(res_in[0]), float(res_out[0])
    gain_db = 20.0 * math.log10(float(gain[0])) if scaled else 0.0
    target = {'report': None, 'input': level_in, 'target': loud['target']}[loud['mode']]
    album = {'input': level_in, 'measured': measured, 'gain_db': gain_db, 'output': measured + gain_db, 'target': target, 'files': len(done),
             'blocks_in': blocks[0], 'blocks_out': blocks[1], 'kept': int(res_out[3])}
    guard_gain = float(host[host.numel() - 4:].clone().view(torch.float32)[0]) if guarded else None
    for e in done:
        rec = e['rec']
        C = rec['written_channels']
        (t_in, _), (t_out, _) = _loudness_views(cut(40)), _loudness_views(cut(40))
        own = float(t_out[0])
        rec['loudness'] = {'input': float(t_in[0]), 'measured': own, 'gain_db': gain_db, 'output': own + gain_db,
                           'momentary_max': float(t_out[1]) + gain_db, 'target': target}
        rec['album'] = album
        if stage is not None:
            e['peaks'] = cut(20 * C + 4)
            e['tpeaks'] = None if tp is None else cut(4 * C + 4)
            e['guard'] = guard_gain
