"""Whole-file generation: FilePath -- the two ends of the file path: a file's bytes through pinned buffers onto the device and
decoded there, and a clip through the output stage and the encoder back into a file behind one synchronisation.  The second of the
two bases SuperResolver (generate/resolver.py) is assembled from; the folder pipeline of loudness_scope 'folder' (generate/album.py)
writes through the same functions."""
import hashlib
import math
import os

import torch

from .ops import (_limiter_stats_views, _pcm_peaks_packed, _peak_views, _true_peak_views, _true_peaks_packed, flac_decode, flac_encode, g711_decode,
                  ima_decode, limiter_apply, limiter_envelope, pcm_decode, pcm_encode, shaper_coefficients)
from .plans import ClipError


def _dbfs(level):
    return 20.0 * math.log10(level) if level > 0.0 else float('-inf')


def _set(**keywords):
    """Only what is set: the keywords that are not None, in the order given.  An option that is off never reaches a callee as a
    keyword, so a callee that knows nothing of it (the stubs of the host tests, an override of before the option) is called as
    it was before the option existed."""
    return {k: v for k, v in keywords.items() if v is not None}


class FilePath:
    """Needs of the object it is part of: `opt` (hr_sampling_rate), `device`, and `_pins`, the dict of its pinned buffers
    (slot -> (the buffer, the event behind the copy that last read it, or None))."""

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

    def _read(self, path, slot='in0', verify=False):
        """Host I/O only: the file's data chunk into pinned buffer `slot` -> (the bytes as a host tensor, WavInfo).  A file whose
        first bytes say FLAC (data/audiofile.py) goes through _read_flac instead; `verify` is its.  A coded data chunk (G.711, IMA
        ADPCM: wavio.CODED_TAGS) is read as it stands; an IMA block header with a step index above 88 is a ValueError here.  An
        AIFF, AU or SPHERE file (data/containers.py) brings its sound data as it stands and a containers.AudioInfo."""
        from ..data import audiofile, containers, wavio
        kind = audiofile.kind(path)
        if kind == 'flac':
            return self._read_flac(path, slot, verify)
        if kind != 'wav':                                                   # AIFF, AU, SPHERE: the sound data as it stands, an AudioInfo
            payload, meta = containers.read_payload(path, into=lambda n: self._pinned(slot, n).numpy())
            return self._pins[slot][0][:len(payload)], meta, slot
        payload, meta = wavio.read_payload(path, into=lambda n: self._pinned(slot, n).numpy())
        if meta.format_tag == 0x11:                                         # IMA ADPCM: the block headers, before the copy (names file and block)
            wavio.ima_scan(payload, meta.num_channels, meta.block_align, os.fspath(path))
        return self._pins[slot][0][:len(payload)], meta, slot

    def _read_flac(self, path, slot, verify=False):
        """Host work only: the whole FLAC file into pinned buffer `slot`, its frame index built on the host (every CRC verified;
        anything the reader does not hold is a ValueError here, before a launch) and laid behind the bytes at the next multiple of
        8 -> (bytes and table as one host tensor, FlacInfo): one copy takes both to the device.  `verify`: the file is first decoded
        on the host and its MD5 compared with STREAMINFO's.  The slot remembers the file's name for _decode's error text."""
        from ..data import flacio
        if verify and flacio.verify(path) is False:
            raise ValueError("%s: the decoded samples do not have the MD5 that STREAMINFO states" % path)
        # room for the table of a file whose frames average 768 bytes or more; a file of smaller frames moves to a larger buffer once
        payload, meta, table = flacio.read_file(path, into=lambda n: self._pinned(slot, n + n // 16 + 4096).numpy())
        n = len(payload)
        at = (n + 7) & ~7
        pinned = self._pins[slot][0]
        if pinned.numel() < at + table.nbytes:
            grown = torch.empty((at + table.nbytes,), dtype=torch.uint8, pin_memory=True)
            grown[:n].copy_(pinned[:n])
            self._pins[slot] = (grown, None)
            pinned = grown
        pinned[n:at].zero_()
        pinned[at:at + table.nbytes].copy_(torch.from_numpy(table).view(-1).view(torch.uint8))
        if not hasattr(self, '_pin_names'):
            self._pin_names = {}
        self._pin_names[slot] = os.fspath(path)
        return pinned[:at + table.nbytes], meta, slot

    def _decode(self, host, meta, slot):
        """The host bytes of a data chunk -> [channels, frames] f32 on the GPU: one copy, one kernel -- the PCM decoder's, or for a
        coded chunk (meta.format_tag 6, 7, 0x11) one of the family "wavcodec".  The bytes and table of a
        FLAC file (_read_flac): one copy, the two kernels of the family "flac", and one wait for their status word -- a frame that
        passed the index's CRCs and still does not decode is a ValueError that names it, before anything else is launched."""
        if host.numel() == 0:
            return torch.zeros((meta.num_channels, 0), dtype=torch.float32, device=self.device)
        dev = torch.empty((host.numel(),), dtype=torch.uint8, device=self.device)
        dev.copy_(host, non_blocking=True)
        busy = torch.cuda.Event()
        busy.record()
        self._pins[slot] = (self._pins[slot][0], busy)
        if hasattr(meta, 'num_flac_frames'):
            at = host.numel() - meta.num_flac_frames * 48
            try:
                return flac_decode(dev[:at], dev[at:].view(torch.int64).view(-1, 6), meta)
            except ValueError as e:                                         # (the decoder's refusal, with the file it is about)
                raise ValueError("%s: %s" % (getattr(self, '_pin_names', {}).get(slot, '<flac>'), e)) from None
        if meta.format_tag in (6, 7):                                       # G.711 A-law / mu-law (csrc/wavcodec.hip)
            return g711_decode(dev, meta.num_frames, meta.num_channels, 'alaw' if meta.format_tag == 6 else 'ulaw')
        if meta.format_tag == 0x11:                                         # IMA ADPCM; _read has scanned the block headers
            return ima_decode(dev, meta.num_frames, meta.num_channels, meta.block_align)
        if getattr(meta, 'big_endian', False) or getattr(meta, 'signed8', False):     # an AudioInfo (data/containers.py)
            return pcm_decode(dev, meta.num_frames, meta.num_channels, meta.format_tag, meta.bits_per_sample, big_endian=meta.big_endian,
                              signed8=meta.signed8)
        return pcm_decode(dev, meta.num_frames, meta.num_channels, meta.format_tag, meta.bits_per_sample)

    def _write(self, path_out, sr, encoding, stage=None, picture=None, loudness=None, speech_level=None, true_peak=None, limiter=None, bandwidth=None, stereo=None, rate=None,
               flac=None):
        """[C, L] on the GPU -> encoded on the device -> one copy back -> header + payload; -> the result's 'output', or None
        without a stage.  path_out None: the figures only.  `stage`: the output-stage options (check_output_options), or None for
        the encoder alone.  Every other keyword is None or what one option of enhance_file brings, and a caller passes only those
        that are set (_set):
          true_peak, limiter   the option's own dict, one file's (check_true_peak, _limiter_option; either comes with a stage):
                               _encode runs its kernels and leaves their packed figures in it, _output reads them
          loudness, speech_level, bandwidth, stereo   the measurement the per-file flow has already queued (_measure_*), a dict with 'packed'
          picture              the rendered spectrogram (_render_picture)
          rate                 the rate the header states where it is not the model's (the output-rate option: `sr` is converted)
          flac                 the container option's own dict, one file's (check_container): the payload goes through the FLAC
                               encoder on the device (_flac_stage) and the stream comes back in its place; it gains 'result'
        The first six come back with the payload and the peak figures behind _fetch's one synchronisation, copied in the order the
        hand-over to _fetch names them."""
        w = sr.contiguous()
        option = _set(true_peak=true_peak, limiter=limiter)
        dev, packed = (None, None) if path_out is None and stage is None else self._encode(w, path_out is not None, encoding, stage, **option)
        extra = {}
        if dev is not None and flac is not None:
            dev, extra = self._flac_stage(dev, w.shape[0], encoding, flac, **_set(rate=rate))
        host, stats = self._fetch(dev, packed, **_set(stereo=stereo, bandwidth=bandwidth, limiter=limiter, true_peak=true_peak, loudness=loudness, speech_level=speech_level,
                                                      picture=picture), **extra)
        output = None if stats is None else self._output(stats, w.shape[0], stage, path_out, encoding, **option)
        if host is not None:
            self._save(path_out, host, sr.shape[0], encoding, **_set(rate=rate, flac=flac))
        return output

    def _flac_stage(self, dev, channels, encoding, flac, rate=None):
        """The payload on the device -> (the FLAC frames on the device at their worst-case size, what _fetch brings back beside
        them): three launches of the family "flacenc".  `flac`: one file's container option, which gains what _save needs: the
        frame lengths ('lengths', a dict whose 'packed' _fetch replaces by its host copy), with md5 the payload itself ('pcm',
        likewise: a second copy of the payload's size), 'pcm_bytes', 'total' and 'rate'."""
        bits = {'pcm16': 16, 'pcm24': 24}[encoding]
        rate = int(self.opt.hr_sampling_rate if rate is None else rate)
        stream, lengths = flac_encode(dev, channels, bits, rate, flac['block'], **_set(lpc_order=flac.get('lpc')))
        flac.update(lengths={'packed': lengths.view(torch.uint8)}, pcm_bytes=dev.numel(), total=dev.numel() // (channels * bits // 8), rate=rate, bits=bits)
        extra = {'flac': flac['lengths']}
        if flac['md5']:
            flac['pcm'] = extra['flac_pcm'] = {'packed': dev}
        return stream, extra

    def _encode(self, w, wanted, encoding, stage, true_peak=None, limiter=None):
        """The device work of _write -> (the payload, or None when no file is `wanted`; the packed peak buffer, or None).
        `true_peak`: None, or the true-peak option, which gains 'packed' (the packed true-peak buffer on the device); the guard's
        gain is then the true-peak kernel's.  `limiter`: None, or the limiter option, which gains 'packed' (12 bytes on the device:
        the curve's statistics, then the true peak the clip came with); the two launches of the family "limiter" run first and the
        peak kernels, the guard's gain and the encoder see the limited clip."""
        if stage is None:
            return pcm_encode(w, encoding), None
        if limiter is not None:
            packed = limiter['packed'] = torch.empty((12,), dtype=torch.uint8, device=w.device)
            r, _ = limiter_envelope(w, limiter['rate'], limiter['ceiling'], peak_out=packed[8:].view(torch.float32))
            w, _, _ = limiter_apply(w, r, limiter, stats_out=packed[:8], want_g=False)
        (_, _, _, gain), packed = _pcm_peaks_packed(w, encoding, stage['ceiling'], "enhance_file")
        if true_peak is not None:
            (_, gain), true_peak['packed'] = _true_peaks_packed(w, true_peak['rate'], true_peak['ceiling'], "enhance_file")
        if not wanted:
            return None, packed
        return pcm_encode(w, encoding, gain=gain if stage['clip'] == 'guard' else None, dither=stage['dither'], seed=stage['seed'],
                          curve=stage.get('curve'), chunk=stage.get('chunk')), packed

    def _fetch(self, dev, packed, picture=None, **measured):
        """The payload and the packed peak buffer (either may be None) into their pinned buffers 'out' and 'peaks' behind one
        synchronisation -> (the payload, the peak buffer) on the host.  `measured`: name -> a dict whose 'packed' (a device tensor:
        the figures of 'stereo', 'bandwidth', 'limiter', 'true_peak', 'loudness', 'speech_level') is copied into the pinned buffer of that name in
        front of them, in the order given, and replaced by its host copy.  `picture`: None, or a dict whose 'image' and 'top' are
        copied and replaced likewise, into one buffer: the top's four bytes, then the pixels."""
        host = stats = None
        for name, m in measured.items():
            n = m['packed'].numel()
            pin = self._pinned(name, n)[:n]
            pin.copy_(m['packed'], non_blocking=True)
            m['packed'] = pin
        if picture is not None:
            img, top = picture['image'], picture['top']
            n = img.numel()
            pin = self._pinned('picture', 4 + n)
            pin[:4].copy_(top.view(torch.uint8), non_blocking=True)
            pin[4:4 + n].copy_(img.reshape(-1), non_blocking=True)
            picture['image'], picture['top'] = pin[4:4 + n].view(img.shape), pin[:4].view(torch.float32)
        if dev is not None:
            host = self._pinned('out', dev.numel())[:dev.numel()]
            host.copy_(dev, non_blocking=True)
        if packed is not None:
            stats = self._pinned('peaks', packed.numel())[:packed.numel()]
            stats.copy_(packed, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return host, stats

    @staticmethod
    def _output(stats, C, stage, path_out, encoding, true_peak=None, limiter=None):
        """The fetched peak buffer of a C-channel clip -> the result's 'output'; ClipError where clip 'error' finds a clipped sample.
        `true_peak`: None, or the true-peak option with its fetched 'packed': the output gains 'true_peak' and 'true_peak_dbtp', its
        'gain' is the true-peak kernel's, and clip 'error' also refuses a true peak above the encoding's limit.  `limiter`: None, or
        the limiter option with its fetched 'packed': the output gains 'limiter', and every other figure is the limited clip's."""
        peak, over, nonfinite, gain = (v.tolist() for v in _peak_views(stats, C))
        if true_peak is not None:
            tpeak, gain = (v.tolist() for v in _true_peak_views(true_peak['packed'], C))
        output = {'peak': peak, 'peak_dbfs': [_dbfs(v) for v in peak], 'clipped': over, 'nonfinite': nonfinite,
                  'gain': gain[0] if stage['clip'] == 'guard' else 1.0}
        if true_peak is not None:
            output.update(true_peak=tpeak, true_peak_dbtp=[_dbfs(v) for v in tpeak])
            if stage['clip'] == 'error' and max(tpeak) > true_peak['limit']:
                raise ClipError("%s: the true peak %+.2f dBTP is above the limit of %s (%d samples would clip); nothing was written -- "
                                "clip='guard' scales the file down" % (path_out, max(output['true_peak_dbtp']), encoding, sum(over)))
        if stage['clip'] == 'error' and any(over):
            raise ClipError("%s: %d samples would clip in %s (peak %+.2f dBFS); nothing was written -- clip='guard' scales "
                            "the file down, encoding='float32' keeps the samples"
                            % (path_out, sum(over), encoding, max(output['peak_dbfs'])))
        if limiter is not None:
            gmin, count = _limiter_stats_views(limiter['packed'][:8])
            output['limiter'] = {'lookahead': limiter['lookahead'], 'hold': limiter['hold'], 'max_reduction_db': _dbfs(float(gmin[0])),
                                 'limited_samples': int(count[0]) & 0xFFFFFFFF,
                                 'input_true_peak_dbtp': _dbfs(float(limiter['packed'][8:12].view(torch.float32)[0]))}
        if stage['dither'] == 'shaped':
            output['dither'] = {'kind': 'shaped', 'curve': stage['curve'], 'taps': shaper_coefficients(stage['curve']).numel(), 'chunk': stage['chunk']}
        return output

    def _save(self, path_out, host, channels, encoding, rate=None, flac=None):
        """The one place that turns what _fetch brought back into a file: header + payload, or with `flac` (the container option
        behind _flac_stage and _fetch) "fLaC", STREAMINFO and the frames' first lengths[-1] bytes; `flac` gains 'result'."""
        from ..data import flacio, wavio
        os.makedirs(os.path.dirname(os.path.abspath(path_out)), exist_ok=True)
        if flac is not None:
            lengths = flac['lengths']['packed'].clone().view(torch.int64).numpy()
            md5 = hashlib.md5(flac['pcm']['packed'].numpy()).digest() if flac['md5'] else None
            n = flacio.write_stream(path_out, host.numpy(), lengths, flac['rate'], channels, flac['bits'], flac['total'], flac['block'], md5)
            flac['result'] = {'block': flac['block'], 'frames': len(lengths) - 1, 'bytes': n, 'pcm_bytes': flac['pcm_bytes'],
                              'md5': None if md5 is None else md5.hex(), **_set(lpc=flac.get('lpc'))}
            return
        wavio.write_payload(path_out, host.numpy(), int(self.opt.hr_sampling_rate if rate is None else rate), channels, encoding)
