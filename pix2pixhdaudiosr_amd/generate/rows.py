"""Whole-file generation: ClipPath -- the rows of a clip: the model and its captured graph, a clip through the model group by
group, and the crossover and mid/side around the rows.  The first of the two bases SuperResolver (generate/resolver.py, which
documents the constructor's options) is assembled from."""
import math
from collections import namedtuple

import torch

from .ops import (bandwidth as _bandwidth, crossover, crossover_coefficients, segments_gather_planar, segments_gather_ragged, segments_stitch_planar,
                  segments_stitch_ragged, stereo_matrix)
from .plans import (BANDWIDTH_DEFAULTS, CROSSOVER_AUTO, check_crossover, check_lowband, check_norm_scope, check_segment_norm, check_stereo,
                    crossover_auto_plan, group_rows_plan, segment_plan, spectro_bins)

# One clip between the parts of enhance_lr / enhance_lr_many: `x` the [C, L] clip the rows are gathered from (mid and side with
# stereo 'ms'), its segment plan, and `measured` -- the auto crossover's measurement on the device and the event behind it, or None.
_Clip = namedtuple('_Clip', 'x C L S stride ms measured')


class ClipPath:
    """A clip on the device -> the generated clip (enhance_lr, enhance_lr_many).  What it needs of the file path is one pinned
    buffer for the auto crossover's measurement (_pinned: fileio.FilePath)."""

    # what an object built without __init__ (the stubs of the host tests) runs with: every option of the constructor off
    stereo, norm_scope, crossover_auto, last_norm, last_crossover = 'lr', 'group', False, None, None
    segment_norm = False

    def __init__(self, model, opt, overlap=0.25, batch=None, graph=True, reference_amplitude=None, lowband='model',
                 lowband_fade=0, crossover=None, crossover_hz=None, crossover_taps=None, stereo='lr', norm_scope='group',
                 segment_norm=False):
        from ..models.mdct import IMDCT2, IMDCT4
        from ..util import util as U
        self.model, self.opt = model, opt
        self.T = int(opt.segment_length)
        self.overlap = float(overlap)
        segment_plan(0, self.T, self.overlap)                               # validates both
        self.norm_scope = check_norm_scope(norm_scope)
        self.segment_norm = check_segment_norm(segment_norm, self.norm_scope)
        self.last_norm = None                             # 'clip': [C, 2] on the GPU, the latest call's ranges; segment_norm: [C, S, 2]
        self._rows = None                                                   # segment_norm: the [batch, 8] table of the latest eager group
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
            from ..dct.dct import IDCT
            self._imdct = IMDCT2(idct_op=IDCT(), **kw)                      # generate_audio.py:23-25
        elif self.mdct_type == 'mdct4':
            self._imdct = IMDCT4(**kw)
        else:
            raise ValueError("SuperResolver: mdct_type must be 'mdct2' or 'mdct4', got %r" % (self.mdct_type,))
        if self.up_ratio < 1:
            raise ValueError("SuperResolver: lr_sampling_rate above hr_sampling_rate")
        self.lowband, self.lowband_fade, _ = check_lowband(lowband, lowband_fade, spectro_bins(opt.n_fft, self.mdct_type), self.up_ratio)
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
        self.crossover_auto = crossover == 'input' and crossover_hz == CROSSOVER_AUTO
        self._xover_auto = {}                                               # k_top -> (plan, edge, the coefficients on the device)
        self._side = None                                                   # the stream the auto crossover's measurement comes back on
        self.last_crossover = None                                          # auto: {'hz', 'taps', 'edge_hz'} of the latest clip
        self.stereo = check_stereo(stereo)
        self._g = None                                                      # captured chain of a full group
        # the one constructor of the assembled object also makes what the file path (fileio.FilePath) keeps: an object built
        # without it has neither, as ever
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

    def _group(self, seg, noise, norm=None):
        """[b, T] low-rate segments -> [b, T] generated ones, before the sqrt(up_ratio - 1) gain (generate_audio.py:34-44).
        `norm`: None (norm_scope 'group': the model is called as ever), the clip's norm8, or 'rows' (segment_norm: every row
        its own range; the group's [b, 8] table is left in self._rows)."""
        from ..util import util as U
        if norm is None:
            sr_spectro, lr_pha, norm_param, lr_spectro = self.model.inference(seg, None, noise=noise)
        else:
            sr_spectro, lr_pha, norm_param, lr_spectro = self.model.inference(seg, None, noise=noise, norm=norm)
        if isinstance(norm, str):
            self._rows = norm_param['rows']
        splice = {} if self.lowband == 'model' else dict(lr_spectro=lr_spectro, lowband_fade=self.lowband_fade)
        audio = U.imdct(spectro=sr_spectro.abs(), pha=lr_pha.squeeze(1), norm_param=norm_param, _imdct=self._imdct,
                        up_ratio=self.up_ratio, explicit_encoding=bool(getattr(self.opt, 'explicit_encoding', False)), **splice)
        audio = audio.reshape(seg.shape[0], -1)
        if audio.shape[1] != self.T:
            raise ValueError("SuperResolver: segment_length %d does not come back from the transform (got %d samples): use "
                             "a multiple of hop_length" % (self.T, audio.shape[1]))
        return audio

    def _run_graphed(self, seg, noise, norm=None):
        """The chain of a full group through a graph over static buffers.  The first use runs the chain once eagerly on the
        buffers (packed weights, tables and workspaces exist before capture), then captures it; every use replays.  Weights
        that changed since (load_network, an optimiser step) make the capture stale: it is redone.  `norm` (norm_scope 'clip'):
        the clip's norm8, copied into a static buffer the captured encode and decode read; 'rows' (segment_norm) is handed on as
        it is, and the table the captured encode writes is kept as g['rows']."""
        from .. import _ops
        g = self._g
        by_rows = isinstance(norm, str)
        if g is None or g['epoch'] != _ops._WEIGHT_EPOCH[0]:
            shape = self.noise_shape(self.batch)
            g = self._g = {'epoch': _ops._WEIGHT_EPOCH[0], 'graph': None, 'out': None,
                           'seg': torch.empty((self.batch, self.T), dtype=torch.float32, device=self.device),
                           'noise': None if shape is None else torch.empty(shape, dtype=torch.float32, device=self.device),
                           'norm': norm if norm is None or by_rows else torch.empty((8,), dtype=torch.float32, device=self.device)}
        g['seg'].copy_(seg)
        if g['norm'] is not None and not by_rows:
            g['norm'].copy_(norm)
        if g['noise'] is not None:
            g['noise'].copy_(noise)
        if g['graph'] is None:
            self._group(g['seg'], g['noise'], g['norm'])
            torch.cuda.synchronize()
            # as _train_step_graphed captures: a side stream behind the current (step) stream, thread-local capture mode,
            # no flush of the caching allocator
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                graph.capture_begin(capture_error_mode="thread_local")
                g['out'] = self._group(g['seg'], g['noise'], g['norm'])
                graph.capture_end()
            torch.cuda.current_stream().wait_stream(side)
            g['graph'] = graph
            if by_rows:
                g['rows'] = self._rows
        g['graph'].replay()
        return g['out']

    def _group_rows(self, seg, noise):
        """segment_norm: one full group, [batch, T] -> (the generated [batch, T], the group's [batch, 8] table of ranges on the
        device), through the graph where the chain may be captured."""
        if self.graph and self._graph_ok():
            return self._run_graphed(seg, noise, 'rows'), self._g['rows']
        return self._group(seg, noise, 'rows'), self._rows

    def _walk_rows(self, seg, out, noise, C, S):
        """segment_norm: the C * S channel-major rows of `seg` through _group_rows in groups of `batch`, without regard to channel
        (plans.group_rows_plan); the last group is filled up with rows of zeros (and zeros for their rows of a given `noise`), whose
        output is dropped.  Leaves `out` filled and `last_norm` [C, S, 2]; nothing is waited for."""
        R = seg.shape[0]
        ranges = torch.empty((R, 2), dtype=torch.float32, device=seg.device)
        shape = self.noise_shape(self.batch)
        for r0, n in group_rows_plan(R, self.batch):
            rows = seg[r0:r0 + n]
            fill = self.batch - n
            if fill:
                rows = torch.cat((rows, rows.new_zeros((fill, rows.shape[1]))))
            nz = None
            if shape is not None:
                if noise is None:
                    nz = torch.randn(shape, device=self.device)
                else:
                    nz = noise[r0:r0 + n]
                    if tuple(nz.shape) != (n,) + tuple(shape[1:]):
                        raise ValueError("enhance_lr: noise for rows %d..%d has shape %s, expected %s"
                                         % (r0, r0 + n - 1, tuple(nz.shape), (n,) + tuple(shape[1:])))
                    if fill:
                        nz = torch.cat((nz, nz.new_zeros((fill,) + tuple(shape[1:]))))
            audio, table = self._group_rows(rows, nz)
            out[r0:r0 + n].copy_(audio[:n])
            ranges[r0:r0 + n].copy_(table[:n, :2])
        self.last_norm = ranges.view(C, S, 2)

    # -- one clip ----------------------------------------------------------------------------------
    def enhance_lr(self, lr_audio, noise=None):
        """lr_audio: [C, L] or [L] on the GPU, already at the high rate -> the generated clip [C, L] ([1, L] for [L]).  Every
        channel is a clip of its own: its S segments are grouped as if it were a mono clip, so
        enhance_lr(x)[c] == enhance_lr(x[c:c+1])[0] given the same noise rows.  `noise`: the mask noise of all C * S segments,
        [C * S, channels, mask_rows, frames], channel-major, sliced per group; drawn per group (one torch.randn) when absent.
        With norm_scope 'clip' the property holds as well, and a channel's range is taken in front of its first group: its S
        segments go through model.clip_norm, the channel's rows of `noise` are folded as they are, and without `noise` the mask
        noise of the channel is drawn in one torch.randn of [S, channels, mask_rows, frames] -- the range of the noise must be
        known before the first group is encoded --, which holds S / batch times the memory of a group's draw for the length of the
        channel: 4 * channels * mask_rows * frames bytes per segment, the (1 - 1 / up_ratio) part of a segment's encoded spectrogram.
        With segment_norm the property holds too, at every batch size, although the C * S rows share groups (_walk_rows): a row's
        encode and decode see that row alone, and what the generator itself does with its batch is all that is left."""
        run = getattr(self.model, '_on_step_stream', None)
        with torch.no_grad():
            return run(self._enhance_lr, lr_audio, noise) if callable(run) else self._enhance_lr(lr_audio, noise)

    def _before_rows(self, lr_audio):
        """In front of the rows, per clip: the checks, the auto crossover's measurement and its event, the mid/side encode -> the
        _Clip the rows and _behind_rows go on with."""
        x = lr_audio.to(self.device).float()
        if x.dim() == 1:
            x = x[None]
        if x.dim() != 2 or x.shape[0] < 1:
            raise ValueError("enhance_lr: expected a [C, L] or [L] waveform, got shape %s" % (tuple(lr_audio.shape),))
        x = x.contiguous()
        C, L = x.shape
        S, stride, V = segment_plan(L, self.T, self.overlap)
        ms = self.stereo == 'ms' and C != 1               # (one channel runs as ever, with no launch of the family)
        if ms and C != 2:
            raise ValueError("enhance_lr: stereo='ms' takes one or two channels, got %d" % C)
        measured = None
        if self.crossover_auto:
            # the two measurement launches and their event go in front of every group: the host then waits for them alone
            measured = (_bandwidth(x, float(self.opt.hr_sampling_rate)), torch.cuda.Event())
            measured[1].record()
        if ms:
            # behind the auto crossover's measurement, which stays on left / right: its plan is the one 'lr' gets.  From here on the
            # two rows are mid and side -- the segments, the groups' normalisation, the mask-noise row blocks and the crossover's
            # low band (a linear filter commutes with the matrix)
            x = stereo_matrix(x, 0.5)
        return _Clip(x, C, L, S, stride, ms, measured)

    def _behind_rows(self, clip, sr):
        """Behind the rows, per clip: the stitched [C, L] -> the crossover, fixed or auto, and the mid/side decode."""
        if self.crossover_plan is not None:
            if clip.measured is not None:
                taps = self._auto_taps(*clip.measured)
            else:
                if self._xover_taps is None:
                    self._xover_taps = crossover_coefficients(*self.crossover_plan).to(self.device)
                taps = self._xover_taps
            sr = crossover(sr, clip.x, self.gain / 2.0, taps)
        if clip.ms:
            # back to left / right, in place.  A side signal of digital silence (dual mono) leaves the chain as NaN -- its group is
            # scaled by 1 / (max - min) --: the decoder reads a non-finite side sample as "no side here"
            sr = sr.contiguous()
            stereo_matrix(sr, 1.0, guard_side=True, out=sr)
        return sr

    def enhance_lr_many(self, clips, noise=None):
        """clips: a list of [C_i, L_i] (or [L_i]) waveforms on the GPU, already at the high rate -> the list of generated clips
        [C_i, L_i]: enhance_lr on each, with the rows of all of them -- R = sum of C_i * S_i, clip after clip, each channel-major --
        sharing groups.  Needs segment_norm (a ValueError otherwise): only there does a row not depend on its neighbours.  Each clip
        goes through enhance_lr's part in front of the rows; one ragged gather (ops.segments_gather_ragged) lays all rows out, the
        one walk of _walk_rows takes them through ceil(R / batch) full groups with fillers in the last group only, one ragged
        stitch (ops.segments_stitch_ragged) brings every clip back, and each goes through enhance_lr's part behind the rows.  A
        clip's rows, ranges and stitch are bit for bit those of enhance_lr on it alone; what the generator itself does with a
        row's neighbours in the batch is all that differs.  `noise`: the mask noise of all R rows in that order, [R, channels,
        mask_rows, frames]; drawn per group (one torch.randn) when absent.  `last_norm` then holds a list of [C_i, S_i, 2] views,
        and with crossover_hz 'auto' `last_crossovers` the list of every clip's {'hz', 'taps', 'edge_hz'}."""
        if not self.segment_norm:
            raise ValueError("enhance_lr_many: the rows of several clips share groups, which needs segment_norm=True")
        clips = list(clips)
        if not clips:
            return []
        run = getattr(self.model, '_on_step_stream', None)
        with torch.no_grad():
            return run(self._enhance_lr_many, clips, noise) if callable(run) else self._enhance_lr_many(clips, noise)

    def _enhance_lr_many(self, clips, noise):
        fronts = [self._before_rows(c) for c in clips]
        seg = segments_gather_ragged([f.x for f in fronts], self.T, fronts[0].stride, [f.S for f in fronts])
        out = torch.empty_like(seg)
        self._walk_rows(seg, out, noise, 1, seg.shape[0])
        ranges, views, at = self.last_norm[0], [], 0
        for f in fronts:
            views.append(ranges[at:at + f.C * f.S].view(f.C, f.S, 2))
            at += f.C * f.S
        self.last_norm = views
        stitched = segments_stitch_ragged(out, [f.L for f in fronts], [f.C for f in fronts], fronts[0].stride, self.gain)
        done, self.last_crossovers = [], []
        for f, sr in zip(fronts, stitched):
            done.append(self._behind_rows(f, sr))
            self.last_crossovers.append(dict(self.last_crossover) if self.crossover_auto else None)
        return done

    def _enhance_lr(self, lr_audio, noise):
        clip = self._before_rows(lr_audio)
        x, C, L, S, stride = clip.x, clip.C, clip.L, clip.S, clip.stride
        seg = segments_gather_planar(x, self.T, stride, S)
        out = torch.empty_like(seg)
        by_clip = self.norm_scope == 'clip'
        if by_clip:
            self.last_norm = torch.empty((C, 2), dtype=torch.float32, device=self.device)
            if S == 0:                                                      # (no segment, no range: the empty fold)
                self.last_norm[:, 0] = float('inf')
                self.last_norm[:, 1] = float('-inf')
        if self.segment_norm:
            self._walk_rows(seg, out, noise, C, S)
        for c in range(0 if self.segment_norm else C):                      # (segment_norm: the rows have been walked, above)
            norm = drawn = None
            if by_clip and S > 0:
                # the channel's range, in front of its first group; the noise every group of it will be given is folded with it
                shape = self.noise_shape(S)
                if shape is not None:
                    drawn = noise[c * S:(c + 1) * S] if noise is not None else torch.randn(shape, device=self.device)
                    if tuple(drawn.shape) != shape:
                        raise ValueError("enhance_lr: noise for channel %d has shape %s, expected %s" % (c, tuple(drawn.shape), shape))
                norm = self.model.clip_norm(seg[c * S:(c + 1) * S], noise=drawn, rows=self.batch)
                self.last_norm[c].copy_(norm[:2])
            for s0 in range(0, S, self.batch):
                b = min(self.batch, S - s0)
                r0 = c * S + s0
                shape = self.noise_shape(b)
                nz = None
                if shape is not None:
                    if drawn is not None:
                        nz = drawn[s0:s0 + b]
                    else:
                        nz = noise[r0:r0 + b] if noise is not None else torch.randn(shape, device=self.device)
                    if tuple(nz.shape) != shape:
                        raise ValueError("enhance_lr: noise for segments %d..%d of channel %d has shape %s, expected %s"
                                         % (s0, s0 + b - 1, c, tuple(nz.shape), shape))
                extra = () if norm is None else (norm,)
                if self.graph and b == self.batch and self._graph_ok():
                    out[r0:r0 + b].copy_(self._run_graphed(seg[r0:r0 + b], nz, *extra))
                else:
                    out[r0:r0 + b].copy_(self._group(seg[r0:r0 + b], nz, *extra))
        return self._behind_rows(clip, segments_stitch_planar(out, C, stride, self.gain, L))

    def _auto_taps(self, res_dev, event):
        """crossover_hz 'auto': the clip's measurement (ops.bandwidth's 32 bytes on the device, `event` recorded behind it) -> the
        coefficients of the clip's crossover on the device.  The copy runs on a side stream behind the event and the host waits
        for that copy alone: the groups queued since are not waited for."""
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        pin = self._pinned('xover_auto', 32)[:32]
        self._side.wait_event(event)
        with torch.cuda.stream(self._side):
            pin.copy_(res_dev.view(torch.uint8), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        done.synchronize()
        k_top = int(pin.view(torch.float64)[0])
        entry = self._xover_auto.get(k_top)
        if entry is None:
            hr_rate, nyquist = float(self.opt.hr_sampling_rate), float(self.opt.lr_sampling_rate) / 2.0
            edge = nyquist if k_top < 0 else min(nyquist, k_top * hr_rate / BANDWIDTH_DEFAULTS['n_fft'])
            plan, edge = crossover_auto_plan(hr_rate, self.opt.lr_sampling_rate, edge, self.crossover_taps)
            if plan == self.crossover_plan:                                 # the band reaches the Nyquist frequency: the fixed crossover's table
                if self._xover_taps is None:
                    self._xover_taps = crossover_coefficients(*self.crossover_plan).to(self.device)
                taps = self._xover_taps
            else:
                taps = crossover_coefficients(*plan).to(self.device)
            entry = self._xover_auto[k_top] = (plan, edge, taps)
        plan, edge, taps = entry
        self.last_crossover = {'hz': plan[1] * float(self.opt.hr_sampling_rate), 'taps': plan[0], 'edge_hz': edge}
        return taps
