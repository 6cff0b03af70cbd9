"""Whole-file generation: StreamPath -- a file through the pipeline in windows (enhance_file / enhance_folder with stream_seconds,
--stream_seconds W).  A window of K consecutive segments of every channel (plans.stream_plan) is read, decoded, taken through the
low-rate round trip, gathered, generated, stitched, encoded and appended to the output while the next one is read: device memory
and pinned memory are a window's, whatever the file's length, and the first bytes are on disk when the second window is queued.
The third base SuperResolver (generate/resolver.py) is assembled from; it needs segment_norm, with which a row's encode, range and
decode see that row alone.

Why the written file is the unstreamed one byte for byte (given noise, or a model that draws none, and a generator whose rows do
not depend on their batch neighbours): the resampler's windows reproduce the whole row's sums operand by operand
(plans.stream_plan); the gather of a window's needed range is the whole clip's rows; the rows see themselves alone; the streamed
stitch fades a window's first segment with the carry of the window before through the one row body (csrc/stitch.hip); the mid/side
matrix is pointwise; and the encoder's dither is a function of the sample's index in the file (ops.pcm_encode's first_index).
Without given noise a group's mask noise is one torch.randn drawn in window order, which is the unstreamed order only where the
windows' groups are the clip's groups (one written channel)."""
import os
import struct

import torch

from .ops import pcm_encode, segments_gather_planar, segments_stitch_stream, stereo_matrix
from .plans import PCM_ENCODINGS, check_encoding, select_channels, stream_plan


def wav_header(payload_bytes, rate, channels, encoding):
    """The 44 bytes wavio.write_payload puts in front of a payload of this size."""
    from ..data import wavio
    tag, bits = wavio.ENCODINGS[encoding]
    align = int(channels) * bits // 8
    return (b"RIFF" + struct.pack("<I", 36 + payload_bytes + (payload_bytes & 1)) + b"WAVE"
            + b"fmt " + struct.pack("<IHHIIHH", 16, tag, int(channels), int(rate), int(rate) * align, align, bits)
            + b"data" + struct.pack("<I", payload_bytes))


class StreamPath:
    """Needs of the object it is part of: ClipPath's rows (_walk_rows, gain, T, overlap, batch, stereo) and FilePath's pinned
    buffers and decoder (_pinned, _decode)."""

    def _stream_info(self, path):
        """The header of a file that is to be streamed, read once -> its WavInfo / AudioInfo with num_frames the frames the file
        holds.  Only codings of a fixed size per frame stream: a FLAC or IMA ADPCM input is a ValueError naming file and coding."""
        from ..data import audiofile, containers, wavio
        kind = audiofile.kind(path)
        if kind == 'flac':
            raise ValueError("%s: a FLAC input is not streamed (its frames have no fixed size): stream_seconds takes PCM, float and G.711 "
                             "samples in WAV, AIFF, AU and SPHERE files" % path)
        if kind != 'wav':
            return containers.info(path)
        meta = wavio.frame_info(path)
        if meta.format_tag == 0x11:
            raise ValueError("%s: an IMA ADPCM input is not streamed (its frames share blocks): stream_seconds takes PCM, float and G.711 "
                             "samples in WAV, AIFF, AU and SPHERE files" % path)
        return meta

    def _stream_read(self, path, meta, window, slot):
        """Host I/O only: the window's frames -- one seek, one read -- into pinned buffer `slot` -> (the bytes as a host tensor, the
        info of these frames alone)."""
        from ..data import wavio
        f0, f1 = window['read']
        got = wavio.read_frames(path, meta, f0, f1, into=lambda n: self._pinned(slot, n).numpy())
        return self._pins[slot][0][:len(got)], meta._replace(num_frames=f1 - f0)

    def _stream_front(self, host, meta, slot, k, plan, window):
        """A window's bytes -> [k, needed samples] f32 on the device: the copy, the decoder, and every resampler of the round trip on
        the window with its halo, cut to what the next one reads and at last to the range the window's segments are gathered from."""
        from ..data import audio_dataset                                    # (looked up per call: the tests replace resample)
        x = self._decode(host, meta, slot)[:k]
        for (orig, new, *_), (lo, hi) in zip(plan['stages'], window['cuts']):
            x = audio_dataset.resample(x.contiguous(), orig, new)[..., lo:hi]
        return x

    def _stream_window(self, host, meta, slot, k, plan, window, index, noise, carries, norm, encoding, stage, out_slot):
        """The device work of one window, queued on the current stream -> (the payload's pinned host tensor, the event behind its
        copy).  Nothing is waited for."""
        stride, S = plan['stride'], plan['S']
        s0, s1 = window['s0'], window['s1']
        K = s1 - s0
        x = self._stream_front(host, meta, slot, k, plan, window)
        ms = self.stereo == 'ms' and k == 2
        if ms:
            x = stereo_matrix(x.contiguous(), 0.5)
        seg = segments_gather_planar(x, self.T, stride, K)
        out = torch.empty_like(seg)
        mine = None if noise is None else torch.cat([noise[c * S + s0:c * S + s1] for c in range(k)])
        self._walk_rows(seg, out, mine, k, K)
        norm[:, s0:s1].copy_(self.last_norm)
        a, b = window['emit']
        last = s1 == S
        if carries[0] is None:                                              # two buffers that take turns, a window's tails each
            carries[:] = [out.new_empty((k, plan['V'])) for _ in range(2)]
        sr = segments_stitch_stream(out, k, stride, self.gain, carry_in=carries[index % 2], carry_out=None if last else carries[(index + 1) % 2],
                                    first=s0 == 0, out_length=b - a)
        if ms:
            stereo_matrix(sr, 1.0, guard_side=True, out=sr)
        extra = {} if stage is None else dict(dither=stage['dither'], seed=stage['seed'])
        payload = pcm_encode(sr, encoding, first_index=a * k, **extra)
        pin = self._pinned(out_slot, payload.numel())[:payload.numel()]
        pin.copy_(payload, non_blocking=True)
        return pin, self._stream_event()

    @staticmethod
    def _stream_event():
        """An event recorded on the current stream: what the host waits for before it appends a window's payload."""
        done = torch.cuda.Event()
        done.record()
        return done

    def _enhance_stream(self, path_in, path_out, is_lr_input, channels, encoding, o, stream_seconds, noise=None):
        """One file through the pipeline in windows -> enhance_file's result: the five keys it always has with 'sr', 'lr', 'hr' and
        'metrics' None -- no clip is kept, nothing is compared --, 'norm' ([C, S, 2] on the GPU, copied from every window's table
        without a wait) and 'stream': {'windows', 'segments_per_window', 'groups', 'frames', 'out_frames', 'window_seconds'}.  `noise`:
        None, or the mask noise of all C * S rows in clip row order, sliced per window.  The host waits for the device on one event
        per window, one window late: while window k is queued it waits for window k - 1's payload and appends it, and window k + 1
        has been read into the other input slot by then (whose last copy, two windows back, _pinned makes sure of).  The output is
        written under a temporary name beside the target -- the header first, its sizes follow from the plan -- and renamed behind
        the last window; whatever goes wrong, the temporary file is removed and the error goes on."""
        check_encoding(encoding, "enhance_file")
        meta = self._stream_info(path_in)
        k = select_channels(channels, meta.num_channels)
        self._check_written_channels(o, channels, meta.num_channels)
        hr_rate = int(self.opt.hr_sampling_rate)
        plan = stream_plan(meta.num_frames, meta.sample_rate, self.opt.lr_sampling_rate, hr_rate, is_lr_input, self.T, self.overlap, k,
                           self.batch, stream_seconds)
        windows, L, S = plan['windows'], plan['L'], plan['S']
        if noise is not None and noise.shape[0] != k * S:
            raise ValueError("enhance_file: noise holds %d rows, the file's %d channels of %d segments take %d" % (noise.shape[0], k, S, k * S))
        nbytes = PCM_ENCODINGS[encoding][1]
        total = L * k * nbytes
        norm = torch.empty((k, S, 2), dtype=torch.float32, device=self.device)
        carries = [None, None]
        run = getattr(self.model, '_on_step_stream', None)
        run = run if callable(run) else (lambda fn, *a: fn(*a))
        tmp = f = None
        try:
            if path_out is not None:
                folder = os.path.dirname(os.path.abspath(path_out))
                os.makedirs(folder, exist_ok=True)
                tmp = os.path.join(folder, '.%s.%d.part' % (os.path.basename(path_out), os.getpid()))
                f = open(tmp, 'wb')
                f.write(wav_header(total, hr_rate, k, encoding))
            pending = None
            read = self._stream_read(path_in, meta, windows[0], 'stream0')
            with torch.no_grad():
                for i, window in enumerate(windows):
                    queued = run(self._stream_window, read[0], read[1], 'stream%d' % (i % 2), k, plan, window, i, noise, carries, norm, encoding,
                                 o.stage, 'streamout%d' % (i % 2))
                    if i + 1 < len(windows):
                        read = self._stream_read(path_in, meta, windows[i + 1], 'stream%d' % ((i + 1) % 2))
                    if pending is not None:
                        pending[1].synchronize()
                        if f is not None:
                            f.write(pending[0].numpy())
                    pending = queued
            pending[1].synchronize()
            if f is not None:
                f.write(pending[0].numpy())
                if total & 1:
                    f.write(b"\0")                                          # RIFF chunks are word-aligned
                f.close()
                f = None
                os.replace(tmp, path_out)
                tmp = None
        finally:
            if f is not None:
                f.close()
            if tmp is not None and os.path.exists(tmp):
                os.remove(tmp)
        self.last_norm = norm
        groups = sum(-(-k * (w['s1'] - w['s0']) // self.batch) for w in windows)
        return {'sr': None, 'lr': None, 'hr': None, 'metrics': None, 'info': meta, 'norm': norm,
                'stream': {'windows': len(windows), 'segments_per_window': plan['K'], 'groups': groups, 'frames': meta.num_frames, 'out_frames': L,
                           'window_seconds': plan['K'] * plan['stride'] / float(hr_rate)}}
