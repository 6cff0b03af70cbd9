"""Whole-file super-resolution: wav in, wav out, on the device from the waveform to the waveform.

    python -m pix2pixhdaudiosr_amd.generate --input in.wav --output out.wav --load_pretrain DIR [--overlap 0.25]

    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver(model, opt).enhance_file("in.wav", "out.wav")["sr"]

The chain is the reference's generate_audio.py:27-47 -- segments of `opt.segment_length` samples, `model.inference` and
`util.imdct` per group of `batchSize` segments, the pieces put back together and scaled by sqrt(up_ratio - 1) -- with two
differences.  The segments are cut and joined by two kernels (csrc/stitch.hip), and by default neighbours share
`overlap * segment_length` samples that are cross-faded, where the reference butts the pieces together.  `overlap=0` is the
reference's chain exactly, its amplitude included: with MDCT2 the reference's output is half of sqrt(up_ratio - 1) * x,
because its util.imdct halves what IMDCT2 already returns at unit gain.  With overlapping segments the pipeline returns the
full amplitude -- 6 dB more; `SuperResolver(reference_amplitude=...)` and `--reference_amplitude 0|1` choose explicitly.

A group is semantics: `to_spectro` normalises by the min / max of the whole batch tensor (pix2pixHD_model.py:165-168 of the
reference), so a group holds exactly the segments the reference's loader would put in it and a last, smaller group runs at
its own size -- padding it with silent segments would change its normalisation.
"""
import argparse
import ast
import math
import os
import sys
from types import SimpleNamespace

import torch


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


def segments_gather(audio, T, stride, S):
    """audio [L] f32 on the GPU -> [S, T]: row s holds audio[s * stride : s * stride + T], zeros beyond the end."""
    from . import _lib
    a = _lib.require_gpu_tensor(audio, "segments_gather: audio", torch.float32)
    if a.dim() != 1:
        raise ValueError("segments_gather: expected a 1-D waveform, got shape %s" % (tuple(a.shape),))
    out = torch.empty((max(int(S), 0), max(int(T), 0)), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().p2phd_segments_gather(_lib.ptr(a), a.numel(), int(T), int(stride), int(S), _lib.ptr(out),
                                                _lib.stream_ptr()), "segments_gather")
    return out


def segments_stitch(seg, stride, gain=1.0, out_length=None):
    """seg [S, T] f32 on the GPU -> [out_length] (default: the whole span): gain * the segments laid `stride` apart, the
    T - stride shared samples of neighbours cross-faded with sin^2 / cos^2 weights."""
    from . import _lib
    s = _lib.require_gpu_tensor(seg, "segments_stitch: seg", torch.float32)
    if s.dim() != 2:
        raise ValueError("segments_stitch: expected [S, T], got shape %s" % (tuple(s.shape),))
    S, T = s.shape
    L_out = (S - 1) * int(stride) + T if out_length is None else int(out_length)
    out = torch.empty((max(L_out, 0),), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_segments_stitch(_lib.ptr(s), S, T, int(stride), float(gain), _lib.ptr(out), L_out,
                                                _lib.stream_ptr()), "segments_stitch")
    return out


class SuperResolver:
    """`model`: anything with `.inference(lr_audio, inst, noise=None) -> (sr_spectro, lr_pha, norm_param, lr_spectro)`
    (Pix2PixHDModel); its `mdct_type` picks the inverse transform.  `overlap`: shared fraction of a segment, [0, 0.5].
    `batch`: segments per group (default opt.batchSize).  `graph`: capture the chain of a full group once and replay it
    (options that draw random numbers inside the chain -- mask_mode 'mode1', the single-channel encodings -- run eagerly).
    `reference_amplitude` (mdct2 only): True keeps the amplitude of the reference's generate_audio.py, which is
    sqrt(up_ratio - 1) * x / 2 for a spectrogram that encodes x; False returns sqrt(up_ratio - 1) * x.  Default: True at
    overlap 0, the reference-exact mode, False with overlapping segments."""

    def __init__(self, model, opt, overlap=0.25, batch=None, graph=True, reference_amplitude=None):
        from .models.mdct import IMDCT2, IMDCT4
        from .util import util as U
        self.model, self.opt = model, opt
        self.T = int(opt.segment_length)
        self.overlap = float(overlap)
        segment_plan(0, self.T, self.overlap)                               # validates both
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
            from .dct.dct import IDCT
            self._imdct = IMDCT2(idct_op=IDCT(), **kw)                      # generate_audio.py:23-25
        elif self.mdct_type == 'mdct4':
            self._imdct = IMDCT4(**kw)
        else:
            raise ValueError("SuperResolver: mdct_type must be 'mdct2' or 'mdct4', got %r" % (self.mdct_type,))
        if self.up_ratio < 1:
            raise ValueError("SuperResolver: lr_sampling_rate above hr_sampling_rate")
        # Both inverse transforms return x for the spectrogram of x and util.imdct halves that (util/util.py:127 of the
        # reference), so the hand-composed chain is a factor 2 short of generate_audio.py:47's sqrt(up_ratio - 1) * x; the
        # stitch gain puts the factor back.  The reference's own output (MDCT2, back-to-back segments; tests/golden/generate.npz)
        # carries the halving, and overlap = 0 is the mode that reproduces the reference bit for bit: there -- and only for
        # mdct2, nothing of the reference runs MDCT4 -- the factor is left out, unless the caller decides otherwise.
        if reference_amplitude is None:
            reference_amplitude = self.overlap == 0.0
        self.reference_amplitude = bool(reference_amplitude) and self.mdct_type == 'mdct2'
        self.gain = math.sqrt(self.up_ratio - 1) * (1.0 if self.reference_amplitude else 2.0)
        self._g = None                                                      # captured chain of a full group

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

    def _group(self, seg, noise):
        """[b, T] low-rate segments -> [b, T] generated ones, before the sqrt(up_ratio - 1) gain (generate_audio.py:34-44)."""
        from .util import util as U
        sr_spectro, lr_pha, norm_param, _ = self.model.inference(seg, None, noise=noise)
        audio = U.imdct(spectro=sr_spectro.abs(), pha=lr_pha.squeeze(1), norm_param=norm_param, _imdct=self._imdct,
                        up_ratio=self.up_ratio, explicit_encoding=bool(getattr(self.opt, 'explicit_encoding', False)))
        audio = audio.reshape(seg.shape[0], -1)
        if audio.shape[1] != self.T:
            raise ValueError("SuperResolver: segment_length %d does not come back from the transform (got %d samples): use "
                             "a multiple of hop_length" % (self.T, audio.shape[1]))
        return audio

    def _run_graphed(self, seg, noise):
        """The chain of a full group through a graph over static buffers.  The first use runs the chain once eagerly on the
        buffers (packed weights, tables and workspaces exist before capture), then captures it; every use replays.  Weights
        that changed since (load_network, an optimiser step) make the capture stale: it is redone."""
        from . import _ops
        g = self._g
        if g is None or g['epoch'] != _ops._WEIGHT_EPOCH[0]:
            shape = self.noise_shape(self.batch)
            g = self._g = {'epoch': _ops._WEIGHT_EPOCH[0], 'graph': None, 'out': None,
                           'seg': torch.empty((self.batch, self.T), dtype=torch.float32, device=self.device),
                           'noise': None if shape is None else torch.empty(shape, dtype=torch.float32, device=self.device)}
        g['seg'].copy_(seg)
        if g['noise'] is not None:
            g['noise'].copy_(noise)
        if g['graph'] is None:
            self._group(g['seg'], g['noise'])
            torch.cuda.synchronize()
            # as _train_step_graphed captures: a side stream behind the current (step) stream, thread-local capture mode,
            # no flush of the caching allocator
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                graph.capture_begin(capture_error_mode="thread_local")
                g['out'] = self._group(g['seg'], g['noise'])
                graph.capture_end()
            torch.cuda.current_stream().wait_stream(side)
            g['graph'] = graph
        g['graph'].replay()
        return g['out']

    # -- one clip ----------------------------------------------------------------------------------
    def enhance_lr(self, lr_audio, noise=None):
        """lr_audio: [1, L] or [L] on the GPU, already at the high rate -> the generated clip [1, L].  `noise`: the mask noise
        of all S segments, [S, C, mask_rows, frames], sliced per group; drawn per group (one torch.randn) when absent."""
        run = getattr(self.model, '_on_step_stream', None)
        with torch.no_grad():
            return run(self._enhance_lr, lr_audio, noise) if callable(run) else self._enhance_lr(lr_audio, noise)

    def _enhance_lr(self, lr_audio, noise):
        x = lr_audio.to(self.device).float()
        if x.dim() == 2 and x.shape[0] == 1:
            x = x[0]
        if x.dim() != 1:
            raise ValueError("enhance_lr: expected a [1, L] or [L] waveform, got shape %s" % (tuple(lr_audio.shape),))
        x = x.contiguous()
        L = x.numel()
        S, stride, V = segment_plan(L, self.T, self.overlap)
        seg = segments_gather(x, self.T, stride, S)
        out = torch.empty_like(seg)
        for s0 in range(0, S, self.batch):
            b = min(self.batch, S - s0)
            shape = self.noise_shape(b)
            nz = None
            if shape is not None:
                nz = noise[s0:s0 + b] if noise is not None else torch.randn(shape, device=self.device)
                if tuple(nz.shape) != shape:
                    raise ValueError("enhance_lr: noise for segments %d..%d has shape %s, expected %s"
                                     % (s0, s0 + b - 1, tuple(nz.shape), shape))
            if self.graph and b == self.batch and self._graph_ok():
                out[s0:s0 + b].copy_(self._run_graphed(seg[s0:s0 + b], nz))
            else:
                out[s0:s0 + b].copy_(self._group(seg[s0:s0 + b], nz))
        return segments_stitch(out, stride, self.gain, L).view(1, L)

    def enhance_file(self, path_in, path_out=None, is_lr_input=False):
        """wav -> first channel -> the low-rate round trip of AudioTestDataset (or, with `is_lr_input`, a plain upsample of a
        clip that is already band-limited) -> enhance_lr -> wav at opt.hr_sampling_rate.  Returns {'sr', 'lr', 'hr',
        'metrics'}: [1, L] tensors on the GPU; 'hr' and 'metrics' (util.compute_matrics against the input) are None unless the
        input is a full-band clip at the high rate."""
        from .data import wavio
        from .data.audio_dataset import lr_round_trip
        from .util import util as U
        o = self.opt
        raw, rate = wavio.load(path_in)
        raw = raw[:1].to(self.device)
        lr = lr_round_trip(raw, rate, o.lr_sampling_rate, o.hr_sampling_rate, is_lr_input)
        has_hr = not is_lr_input and int(rate) == int(o.hr_sampling_rate)
        if has_hr:
            lr = lr[..., :raw.shape[-1]]                                    # the round trip rounds the length up
        sr = self.enhance_lr(lr)
        metrics = U.compute_matrics(raw, lr, sr, o) if has_hr else None
        if path_out is not None:
            wavio.save(path_out, sr, int(o.hr_sampling_rate))
        return {'sr': sr, 'lr': lr, 'hr': raw if has_hr else None, 'metrics': metrics}


# ------------------------------------------------------------------------------------------
# command line
# ------------------------------------------------------------------------------------------
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


def _parser():
    ap = argparse.ArgumentParser(prog="python -m pix2pixhdaudiosr_amd.generate", description=__doc__.split("\n")[0])
    ap.add_argument("--input", required=True, help="wav file to enhance")
    ap.add_argument("--output", required=True, help="wav file to write (PCM16 at hr_sampling_rate)")
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
    ap.add_argument("--fp16", action="store_true", help="16-bit activation storage")
    ap.add_argument("--mdct_type", default=None, choices=("mdct2", "mdct4"),
                    help="transform of the checkpoint (default: the options file's, else $P2PHD_MDCT_TYPE, else mdct2 -- "
                         "the one the reference's train.py, which writes opt.txt, is hard-wired to)")
    return ap


def main(argv=None):
    a = _parser().parse_args(argv)
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
    from .models.models import create_model
    model = create_model(opt)
    model.eval()
    if getattr(opt, 'seed', None) is not None:
        torch.manual_seed(int(opt.seed))                                    # the mask noise: one run, one result
    sr = SuperResolver(model, opt, overlap=a.overlap, graph=not a.no_graph,
                       reference_amplitude=None if a.reference_amplitude is None else bool(a.reference_amplitude))
    print('amplitude: %s' % ("the reference's (half of sqrt(up_ratio - 1) * x)" if sr.reference_amplitude else 'full'))
    res = sr.enhance_file(a.input, a.output, a.is_lr_input)
    if res['metrics'] is not None:
        mse, snr_sr, snr_lr, _, _, _, lsd = res['metrics']
        print('MSE: %.4f' % mse)                                            # generate_audio.py:53-59
        print('SNR_SR: %.4f' % snr_sr)
        print('SNR_LR: %.4f' % snr_lr)
        print('LSD: %.4f' % lsd)
    print('wrote %s (%d samples at %d Hz)' % (a.output, res['sr'].shape[-1], int(opt.hr_sampling_rate)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
