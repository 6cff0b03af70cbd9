"""Whole-file generation: the device entry points of csrc/stitch.hip, csrc/pcm.hip, csrc/xover.hip, csrc/specimg.hip,
csrc/loudness.hip, csrc/truepeak.hip, csrc/limiter.hip, csrc/bandwidth.hip, csrc/stereo.hip, csrc/rateconv.hip, csrc/shaper.hip, csrc/flac.hip, csrc/flacenc.hip and csrc/speechlevel.hip as tensor functions."""
import ctypes

import torch

from .. import _lib
from .plans import (BANDWIDTH_DEFAULTS, CROSSOVER_MAX_TAPS, bandwidth_rel, LIMITER_MAX_HOLD, LIMITER_MAX_LOOKAHEAD, LOUDNESS_MAX_CHANNELS, LOUDNESS_MAX_GAIN_DB, check_dither, DITHER_CHUNK, DITHER_CURVES,
                    check_encoding, check_loudness_rate, check_speech_level_rate, SPEECH_LEVEL_DEFAULTS, SPEECH_LEVEL_KERNEL_CHANNELS, limiter_plan, RATECONV_DEFAULTS, spectrogram_lut, STEREO_DEFAULTS, stereo_split_bin, truepeak_plan)

# (format tag, bits per sample) of a RIFF fmt chunk -> P2PHD_PCM_* code of include/p2phd.h: the set wavio.info accepts
PCM_FORMATS = {(1, 8): 0, (1, 16): 1, (1, 24): 2, (1, 32): 3, (3, 32): 4, (3, 64): 5}


def segments_gather(audio, T, stride, S):
    """audio [L] f32 on the GPU -> [S, T]: row s holds audio[s * stride : s * stride + T], zeros beyond the end."""
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
    s = _lib.require_gpu_tensor(seg, "segments_stitch: seg", torch.float32)
    if s.dim() != 2:
        raise ValueError("segments_stitch: expected [S, T], got shape %s" % (tuple(s.shape),))
    S, T = s.shape
    L_out = (S - 1) * int(stride) + T if out_length is None else int(out_length)
    out = torch.empty((max(L_out, 0),), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_segments_stitch(_lib.ptr(s), S, T, int(stride), float(gain), _lib.ptr(out), L_out,
                                                _lib.stream_ptr()), "segments_stitch")
    return out


def _rows(t, name):
    """A [C, L] f32 GPU tensor whose rows are contiguous (a row pitch >= L is fine) -> (tensor, C, L, pitch)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise _lib.P2PHDError("%s: expected a float32 tensor on the GPU (this build has no CPU path)" % name)
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError("%s: expected [C, L] with C >= 1, got shape %s" % (name, tuple(t.shape)))
    C, L = t.shape
    if L > 1 and t.stride(1) != 1 or C > 1 and t.stride(0) < L:
        raise _lib.P2PHDError("%s: expected rows that are contiguous" % name)
    return t, C, L, (t.stride(0) if C > 1 else max(L, 1))


def segments_gather_planar(audio, T, stride, S):
    """audio [C, L] f32 on the GPU (rows contiguous, any row pitch) -> [C * S, T], channel-major: row c * S + s holds
    audio[c, s * stride : s * stride + T], zeros beyond the end.  One launch whatever C is."""
    a, C, L, ld = _rows(audio, "segments_gather_planar: audio")
    out = torch.empty((C * max(int(S), 0), max(int(T), 0)), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().p2phd_segments_gather_planar(_lib.ptr(a), C, max(ld, L), L, int(T), int(stride), int(S), _lib.ptr(out),
                                                       _lib.stream_ptr()), "segments_gather_planar")
    return out


def segments_stitch_planar(seg, C, stride, gain=1.0, out_length=None, ld=None):
    """seg [C * S, T] f32 on the GPU, channel-major -> [C, out_length]: segments_stitch on every channel's S rows, in one
    launch.  `ld`: row pitch of the buffer the result is a view of (default: out_length)."""
    s = _lib.require_gpu_tensor(seg, "segments_stitch_planar: seg", torch.float32)
    C = int(C)
    if s.dim() != 2 or C < 1 or s.shape[0] % C:
        raise ValueError("segments_stitch_planar: expected [C * S, T] with C = %d, got shape %s" % (C, tuple(s.shape)))
    S, T = s.shape[0] // C, s.shape[1]
    L_out = (S - 1) * int(stride) + T if out_length is None else int(out_length)
    ld = max(L_out, 0) if ld is None else int(ld)
    out = torch.empty((C, max(ld, 0)), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_segments_stitch_planar(_lib.ptr(s), C, S, T, int(stride), float(gain), _lib.ptr(out), ld, L_out,
                                                       _lib.stream_ptr()), "segments_stitch_planar")
    return out[:, :max(L_out, 0)]


def _ragged_table(rows):
    """[(address, L, S), ..] of the clip rows in order -> (the N x 4 int64 table of the ragged entries in host memory, with row0
    filled in; the segment rows they close at)."""
    words, at = [], 0
    for addr, L, S in rows:
        words.append((addr, L, S, at))
        at += S
    return torch.tensor(words, dtype=torch.int64).reshape(-1, 4), at


def _ragged_table_dev(N, device):
    """The device buffer a ragged entry copies its checked table into; stream-ordered like any tensor of the allocator."""
    return torch.empty((max(int(_lib.lib().p2phd_segments_ragged_table_bytes(N)), 1),), dtype=torch.uint8, device=device)


def segments_gather_ragged(clips, T, stride, S_list):
    """clips: a list of [C_i, L_i] f32 tensors on the GPU (rows contiguous, any row pitch), S_list: segments per channel of each ->
    seg [sum C_i * S_i, T]: clip after clip, each channel-major, the rows segments_gather_planar(clips[i], T, stride, S_list[i])
    gives -- bit for bit -- in ONE launch for all of them.  Every channel takes the 16-byte path by its own base's alignment."""
    if len(clips) != len(S_list) or not clips:
        raise ValueError("segments_gather_ragged: expected as many segment counts as clips and at least one clip, got %d and %d"
                         % (len(S_list), len(clips)))
    rows, keep = [], []
    for i, (clip, S) in enumerate(zip(clips, S_list)):
        a, C, L, ld = _rows(clip, "segments_gather_ragged: clip %d" % i)
        keep.append(a)
        rows.extend((a.data_ptr() + 4 * c * ld if L else 0, L, int(S)) for c in range(C))
    table, total = _ragged_table(rows)
    dev = keep[0].device
    out = torch.empty((max(total, 0), max(int(T), 0)), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().p2phd_segments_gather_ragged(table.data_ptr(), len(rows), int(T), int(stride), total, _lib.ptr(out),
                                                       _lib.ptr(_ragged_table_dev(len(rows), dev)), _lib.stream_ptr()), "segments_gather_ragged")
    return out


def segments_stitch_ragged(seg, lengths, channel_counts, stride, gain=1.0):
    """seg [sum C_i * S_i, T] f32 on the GPU as segments_gather_ragged lays it out, lengths: L_i, channel_counts: C_i (every channel
    of clip i has S_i = the fewest segments whose span reaches L_i at this stride, at least one) -> a list of [C_i, L_i]: what
    segments_stitch_planar gives on clip i's rows -- bit for bit -- in ONE launch for all of them."""
    s = _lib.require_gpu_tensor(seg, "segments_stitch_ragged: seg", torch.float32)
    if s.dim() != 2 or len(lengths) != len(channel_counts) or not lengths:
        raise ValueError("segments_stitch_ragged: expected [rows, T] and as many lengths as channel counts, at least one")
    T, stride = s.shape[1], int(stride)
    if not 1 <= stride <= T:
        raise ValueError("segments_stitch_ragged: stride must be in [1, T], got %d (T %d)" % (stride, T))
    outs, rows = [], []
    for L, C in zip(lengths, channel_counts):
        L, C = int(L), int(C)
        if L < 0 or C < 1:
            raise ValueError("segments_stitch_ragged: need every length >= 0 and channel count >= 1, got %d and %d" % (L, C))
        S = max(1, -((T - stride - L) // stride))
        out = torch.empty((C, L), dtype=torch.float32, device=s.device)
        outs.append(out)
        rows.extend((out.data_ptr() + 4 * c * L if L else 0, L, S) for c in range(C))
    table, total = _ragged_table(rows)
    if total != s.shape[0]:
        raise ValueError("segments_stitch_ragged: the clips take %d segment rows, seg has %d" % (total, s.shape[0]))
    _lib.check(_lib.lib().p2phd_segments_stitch_ragged(_lib.ptr(s), table.data_ptr(), len(rows), total, T, stride, float(gain),
                                                       _lib.ptr(_ragged_table_dev(len(rows), s.device)), _lib.stream_ptr()), "segments_stitch_ragged")
    return outs


def segments_stitch_stream(seg, C, stride, gain=1.0, carry_in=None, carry_out=None, first=False, out_length=None):
    """One window of a clip that is stitched in windows (p2phd_segments_stitch_stream): seg [C * K, T] f32 on the GPU, channel-major,
    the K consecutive segments s0 .. s0 + K - 1 of every channel -> [C, out_length] (default K * stride: what a window that is not
    the clip's last emits): the clip's stitched samples from position s0 * stride on, bit for bit those of segments_stitch_planar on
    the whole clip (beyond K * stride only in the clip's last window).  `carry_in` [C, T - stride]: the carry_out of the call on the
    window before; not read with `first` (the window holds the clip's segment 0).  `carry_out` [C, T - stride] or None: receives this
    window's own raw tails; it may not overlap carry_in -- two buffers take turns.  One launch of the family "stitch"."""
    s = _lib.require_gpu_tensor(seg, "segments_stitch_stream: seg", torch.float32)
    C = int(C)
    if s.dim() != 2 or C < 1 or s.shape[0] % C or s.shape[0] < C:
        raise ValueError("segments_stitch_stream: expected [C * K, T] with C = %d and K >= 1, got shape %s" % (C, tuple(s.shape)))
    K, T, stride = s.shape[0] // C, s.shape[1], int(stride)
    V = T - stride
    n_out = K * stride if out_length is None else int(out_length)
    for name, t in (("carry_in", None if first else carry_in), ("carry_out", carry_out)):
        if t is not None:
            _lib.require_gpu_tensor(t, "segments_stitch_stream: " + name, torch.float32)
            if tuple(t.shape) != (C, max(V, 0)):
                raise ValueError("segments_stitch_stream: %s must be [%d, %d], got shape %s" % (name, C, max(V, 0), tuple(t.shape)))
    out = torch.empty((C, max(n_out, 0)), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_segments_stitch_stream(_lib.ptr(s), C, K, T, stride, float(gain), None if first or carry_in is None else _lib.ptr(carry_in),
                                                       None if carry_out is None else _lib.ptr(carry_out), 1 if first else 0, _lib.ptr(out),
                                                       max(n_out, 0), n_out, _lib.stream_ptr()), "segments_stitch_stream")
    return out


PCM_BIG_ENDIAN, PCM_SIGNED8 = 1, 2                                      # P2PHD_PCM_* flags of include/p2phd.h


def pcm_decode(payload, frames, channels, format_tag, bits, big_endian=False, signed8=False):
    """payload: uint8 tensor on the GPU holding the interleaved little-endian samples of a data chunk (any byte offset into
    its storage) -> [channels, frames] f32, bit-identical to what wavio.load returns for the file.
    `big_endian`, `signed8`: the payload of an AIFF, AU or SPHERE file (data/containers.py) -- most significant byte first, and 8-bit
    samples in two's complement (8 bit only) -> the bits of its WAV twin (p2phd_pcm_decode_ex: one launch of the family "pcm" as
    well).  With both false the call is p2phd_pcm_decode's."""
    b = _lib.require_gpu_tensor(payload, "pcm_decode: payload", torch.uint8)
    fmt = PCM_FORMATS.get((int(format_tag), int(bits)))
    if fmt is None:
        raise ValueError("pcm_decode: unsupported format (tag %s, %s bit)" % (format_tag, bits))
    frames, channels = int(frames), int(channels)
    if b.numel() < frames * channels * (int(bits) // 8):
        raise ValueError("pcm_decode: %d bytes do not hold %d frames of %d x %d bit" % (b.numel(), frames, channels, bits))
    out = torch.empty((channels, frames), dtype=torch.float32, device=b.device)
    if big_endian or signed8:
        flags = (PCM_BIG_ENDIAN if big_endian else 0) | (PCM_SIGNED8 if signed8 else 0)
        _lib.check(_lib.lib().p2phd_pcm_decode_ex(_lib.ptr(b), frames, channels, fmt, flags, _lib.ptr(out), frames, _lib.stream_ptr()), "pcm_decode_ex")
        return out
    _lib.check(_lib.lib().p2phd_pcm_decode(_lib.ptr(b), frames, channels, fmt, _lib.ptr(out), frames, _lib.stream_ptr()), "pcm_decode")
    return out


G711_LAWS = {'ulaw': 0, 'alaw': 1}                                          # P2PHD_G711_* of include/p2phd.h (format tags 7 and 6)


def g711_decode(payload, frames, channels, law):
    """payload: uint8 tensor on the GPU holding the interleaved G.711 bytes of a data chunk (any byte offset into its storage); law:
    'ulaw' (format tag 7) or 'alaw' (tag 6) -> [channels, frames] f32, bit-identical to what wavio.load returns for the file -- the
    samples of its PCM16 twin (p2phd_g711_decode: one launch of the family "wavcodec", none for frames = 0)."""
    b = _lib.require_gpu_tensor(payload, "g711_decode: payload", torch.uint8)
    if law not in G711_LAWS:
        raise ValueError("g711_decode: law must be one of %s, got %r" % (sorted(G711_LAWS), law))
    frames, channels = int(frames), int(channels)
    if frames < 0 or channels < 1 or b.numel() < frames * channels:
        raise ValueError("g711_decode: %d bytes do not hold %d frames of %d channels" % (b.numel(), frames, channels))
    out = torch.empty((channels, frames), dtype=torch.float32, device=b.device)
    _lib.check(_lib.lib().p2phd_g711_decode(_lib.ptr(b), frames, channels, G711_LAWS[law], _lib.ptr(out), frames, _lib.stream_ptr()), "g711_decode")
    return out


def ima_decode(payload, frames, channels, block_align):
    """payload: uint8 tensor on the GPU holding the IMA ADPCM blocks of a data chunk (any byte offset into its storage; a trailing
    partial block counts with its whole groups) -> the first `frames` frames as [channels, frames] f32, bit-identical to what
    wavio.load returns for the file (p2phd_ima_decode: one launch of the family "wavcodec", none for frames = 0).  A header's step
    index above 88 is clamped, not refused: wavio.ima_scan is the host check that names such a block."""
    b = _lib.require_gpu_tensor(payload, "ima_decode: payload", torch.uint8)
    frames, channels = int(frames), int(channels)
    out = torch.empty((channels if 1 <= channels <= 8 else 1, max(frames, 0)), dtype=torch.float32, device=b.device)
    _lib.check(_lib.lib().p2phd_ima_decode(_lib.ptr(b), b.numel(), channels, int(block_align), frames, _lib.ptr(out), max(frames, 0),
                                           _lib.stream_ptr()), "ima_decode")
    return out


FLAC_REASONS = {1: "its bit stream runs past the frame's end", 2: "a reserved code", 3: "an impossible partition or predictor order",
                4: "its subframes end short of the frame's length", 5: "a table row that does not fit the buffers or the channel count"}


def flac_decode(bytes_dev, table, info, check=True):
    """bytes_dev: uint8 tensor on the GPU holding a FLAC file as it stands; table: its frame index, int64 [frames, 6] (data/flacio.py:
    index_bytes / read_file), on the GPU or on the host (then copied); info: its FlacInfo -> [channels, num_frames] f32 on the GPU,
    bit-identical to what flacio.load returns for the file (p2phd_flac_decode: two launches of the family "flac", none for a file
    without frames).  `check` (default): waits for the decoder's status word and raises a ValueError that names the lowest frame that
    did not decode (such a frame is zeros in the result).  check=False: nothing is waited for and (out, status) is returned --
    status an int64 tensor of one element on the GPU, -1 for "every frame decoded", else frame << 8 | reason."""
    b = _lib.require_gpu_tensor(bytes_dev, "flac_decode: bytes_dev", torch.uint8)
    if isinstance(table, torch.Tensor) and table.is_cuda:
        t = _lib.require_gpu_tensor(table, "flac_decode: table", torch.int64)
    else:
        t = torch.as_tensor(table, dtype=torch.int64).contiguous().to(b.device)
    if t.dim() != 2 or t.shape[1] != 6:
        raise ValueError("flac_decode: expected a table [frames, 6], got shape %s" % (tuple(t.shape),))
    C, L, bits = int(info.num_channels), int(info.num_frames), int(info.bits_per_sample)
    out = torch.zeros((C, L), dtype=torch.float32, device=b.device)
    status = torch.full((1,), -1, dtype=torch.int64, device=b.device)
    lib = _lib.lib()
    if t.shape[0] and L:
        n = lib.p2phd_flac_workspace_bytes(C, L)
        if n == 0:
            _lib.check(-1, "flac_workspace_bytes")
        work = torch.empty((n,), dtype=torch.uint8, device=b.device)
        _lib.check(lib.p2phd_flac_decode(_lib.ptr(b), b.numel(), _lib.ptr(t), t.shape[0], C, bits, _lib.ptr(out), L, _lib.ptr(work), _lib.ptr(status),
                                         _lib.stream_ptr()), "flac_decode")
    if not check:
        return out, status
    v = int(status.item())
    if v != -1:
        raise ValueError("flac_decode: frame %d does not decode: %s" % (v >> 8, FLAC_REASONS.get(v & 255, "reason %d" % (v & 255))))
    return out


def flac_encode(payload, channels, bits, rate, block=None, lpc_order=0):
    """payload: uint8 tensor on the GPU, the interleaved little-endian samples pcm_encode leaves ('pcm16': bits 16, 'pcm24': bits 24;
    a view at any byte offset) -> (stream, lengths) on the GPU: `stream` a uint8 tensor of the plan's worst-case size whose first
    lengths[-1] bytes are the FLAC frames back to back (bytes behind them are not written), `lengths` int64 [frames + 1], each frame's
    bytes and their total -- what data/flacio.py's write_stream puts behind its header, and byte for byte what flacio.encode gives for
    the same payload (p2phd_flac_encode: three launches of the family "flacenc").  `block`: samples per frame (None: 4096).
    `lpc_order` M in 0 .. 12: with M > 0 every LPC order 1 .. M is tried beside the fixed predictors (p2phd_flac_encode_lpc, the frame
    kernel's LPC instantiation, still three launches; block at most 16384), byte for byte flacio.encode(..., lpc_order=M).  Nothing
    is waited for."""
    from ..data import flacio
    b = _lib.require_gpu_tensor(payload, "flac_encode: payload", torch.uint8)
    block = flacio.DEFAULT_BLOCK if block is None else block
    flacio.check_output(channels, bits, rate, block, "flac_encode")
    flacio.check_lpc(lpc_order, block, "flac_encode")
    align = int(channels) * int(bits) // 8
    if b.dim() != 1 or b.numel() == 0 or b.numel() % align:
        raise ValueError("flac_encode: %s bytes are not one or more whole frames of %d x %d bit" % (tuple(b.shape), channels, bits))
    L = b.numel() // align
    frames, worst, nwork = flacio.encode_plan(channels, bits, L, block)
    stream = torch.empty((worst,), dtype=torch.uint8, device=b.device)
    lengths = torch.empty((frames + 1,), dtype=torch.int64, device=b.device)
    work = torch.empty((nwork // 8,), dtype=torch.int64, device=b.device)
    if lpc_order:
        _lib.check(_lib.lib().p2phd_flac_encode_lpc(_lib.ptr(b), int(channels), int(bits), L, int(rate), int(block), lpc_order, _lib.ptr(stream), worst,
                                                    _lib.ptr(lengths), _lib.ptr(work), nwork, _lib.stream_ptr()), "flac_encode_lpc")
        return stream, lengths
    _lib.check(_lib.lib().p2phd_flac_encode(_lib.ptr(b), int(channels), int(bits), L, int(rate), int(block), _lib.ptr(stream), worst, _lib.ptr(lengths),
                                            _lib.ptr(work), nwork, _lib.stream_ptr()), "flac_encode")
    return stream, lengths


def shaper_coefficients(curve):
    """The taps h[1..K] of a noise-shaping curve (a name of DITHER_CURVES; p2phd_shaper_taps_fill) as a float32 tensor on the host (no
    GPU needed): the noise transfer function of dither='shaped' is 1 - sum_k h[k] z^-k."""
    if curve not in DITHER_CURVES:
        raise ValueError("shaper_coefficients: curve must be one of %s, got %r" % (sorted(DITHER_CURVES), curve))
    h = torch.zeros((16,), dtype=torch.float32)
    K = ctypes.c_int32(0)
    _lib.check(_lib.lib().p2phd_shaper_taps_fill(DITHER_CURVES[curve], ctypes.c_void_p(h.data_ptr()), ctypes.byref(K)), "shaper_taps_fill")
    return h[:K.value].clone()


def pcm_encode(waveform, encoding='pcm16', gain=None, dither=None, seed=0, first_index=0, curve=None, chunk=None):
    """waveform [C, L] f32 on the GPU (rows contiguous) -> uint8 tensor of L * C samples, interleaved: the payload
    wavio.write_payload takes.  'pcm16' gives the bytes wavio.save writes; NaN encodes as 0 in the integer formats.
    `gain`: a float32 tensor of one element on the GPU (pcm_peaks' fourth value) that the kernel reads: every sample is
    multiplied by it first.  `dither`: None or 'tpdf' (pcm16 only): +-1 LSB of triangular noise in front of the rounding,
    a hash of (`seed`, `first_index` + the sample's index in the payload) -- encoding a clip in pieces with the right
    `first_index` gives the bytes of one call.  'shaped' (pcm16 only; csrc/shaper.hip, p2phd_pcm_encode_shaped): the same dither in
    front of an error-feedback quantiser with the taps of `curve` (a name of DITHER_CURVES, or a float32 tensor of at most 16 taps
    on the host; None: 'lipshitz9'), whose error history starts at zero every `chunk` samples of a channel (None: 4096; a multiple
    of 64 in [256, 2^20]) -- pieces give the bytes of one call where each starts on a chunk boundary, and a `first_index` that is
    not a multiple of chunk * C is refused."""
    fmt, nbytes = check_encoding(encoding, "pcm_encode")
    w, C, L, ld = _rows(waveform, "pcm_encode: waveform")
    out = torch.empty((L * C * nbytes,), dtype=torch.uint8, device=w.device)
    taps = curve if isinstance(curve, torch.Tensor) else None
    check_dither(dither, encoding, "pcm_encode", None, None if taps is not None and dither == 'shaped' else curve, chunk)
    if gain is not None:
        gain = _lib.require_gpu_tensor(gain, "pcm_encode: gain", torch.float32)
        if gain.numel() != 1:
            raise ValueError("pcm_encode: gain must hold one value, got shape %s" % (tuple(gain.shape),))
    if int(first_index) < 0:
        raise ValueError("pcm_encode: first_index must be >= 0, got %r" % (first_index,))
    if dither == 'shaped':
        if taps is None:
            taps = shaper_coefficients('lipshitz9' if curve is None else curve)
        if taps.is_cuda or taps.dtype != torch.float32 or taps.dim() != 1 or taps.numel() > 16:
            raise ValueError("pcm_encode: curve must be a name or at most 16 float32 taps on the host, got %s %s on %s"
                             % (tuple(taps.shape), taps.dtype, taps.device))
        taps = taps.contiguous()
        _lib.check(_lib.lib().p2phd_pcm_encode_shaped(_lib.ptr(w), L, C, max(ld, L), _lib.ptr(gain), ctypes.c_void_p(taps.data_ptr() if taps.numel() else None),
                                                      taps.numel(), DITHER_CHUNK if chunk is None else int(chunk), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                      int(first_index), _lib.ptr(out), _lib.stream_ptr()), "pcm_encode_shaped")
        return out
    _lib.check(_lib.lib().p2phd_pcm_encode_ex(_lib.ptr(w), L, C, max(ld, L), fmt, _lib.ptr(gain), 1 if dither else 0,
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_index), _lib.ptr(out), _lib.stream_ptr()),
               "pcm_encode_ex")
    return out


def _peak_views(buf, C):
    """The packed peak buffer -- over[C] i64 | nonfinite[C] i64 | peak[C] f32 | gain f32, 20 * C + 4 bytes, on the device or
    its copy on the host -> (peak, over, nonfinite, gain) as typed views."""
    return (buf[16 * C:20 * C].view(torch.float32), buf[:8 * C].view(torch.int64), buf[8 * C:16 * C].view(torch.int64),
            buf[20 * C:20 * C + 4].view(torch.float32))


def _pcm_peaks_packed(waveform, encoding, ceiling, who):
    """-> (the four results of pcm_peaks as views of one byte buffer, the buffer): one copy brings all of them back."""
    fmt, _ = check_encoding(encoding, who)
    ceiling = 0.0 if ceiling is None else float(ceiling)
    if not ceiling >= 0.0 or ceiling == float('inf'):
        raise ValueError("%s: ceiling must be a finite level > 0, or None for the encoding's own limit, got %r" % (who, ceiling))
    w, C, L, ld = _rows(waveform, "%s: waveform" % who)
    buf = torch.empty((20 * C + 4,), dtype=torch.uint8, device=w.device)
    peak, over, nonfinite, gain = views = _peak_views(buf, C)
    _lib.check(_lib.lib().p2phd_pcm_peak(_lib.ptr(w), L, C, max(ld, L), fmt, ceiling, _lib.ptr(peak),
                                         _lib.ptr(over), _lib.ptr(nonfinite), _lib.ptr(gain), _lib.stream_ptr()), "pcm_peak")
    return views, buf


def pcm_peaks(waveform, encoding='pcm16', ceiling=None):
    """What `encoding` would meet in waveform [C, L] f32 on the GPU (rows contiguous) -> (peak [C] f32, over [C] i64,
    nonfinite [C] i64, gain [1] f32), all on the GPU, nothing waited for: per channel the largest |x| among the finite samples,
    the number of samples the encoder would clamp (above the encoding's limit or below -1; beyond +-1 for float32) and the
    number of NaN / inf samples; and the one gain for all channels that brings the largest peak down to `ceiling` (a linear
    level; None: the encoding's limit) -- 1 where it already is.  The same bits on every run."""
    return _pcm_peaks_packed(waveform, encoding, ceiling, "pcm_peaks")[0]


def crossover_coefficients(taps, cutoff, beta):
    """The coefficients of p2phd_xover_taps_fill as a float32 tensor on the host (no GPU needed)."""
    h = torch.empty((max(int(taps), 1),), dtype=torch.float32)
    _lib.check(_lib.lib().p2phd_xover_taps_fill(int(taps), float(cutoff), float(beta), ctypes.c_void_p(h.data_ptr())), "xover_taps_fill")
    return h


def crossover(sr, lr, level, taps_dev):
    """sr, lr: [C, L] f32 on the GPU (rows contiguous, any row pitch), taps_dev: an odd number (<= 4095) of f32 coefficients on
    the GPU -> a new [C, L]: sr + LP * (level * lr - sr), the difference zero-extended beyond the clip (p2phd_xover_fwd)."""
    s, C, L, ld_s = _rows(sr, "crossover: sr")
    l, Cl, Ll, ld_l = _rows(lr, "crossover: lr")
    if (C, L) != (Cl, Ll):
        raise ValueError("crossover: sr and lr must have one shape, got %s and %s" % (tuple(s.shape), tuple(l.shape)))
    h = _lib.require_gpu_tensor(taps_dev, "crossover: taps_dev", torch.float32)
    if h.dim() != 1 or not 1 <= h.numel() <= CROSSOVER_MAX_TAPS or h.numel() % 2 == 0:
        raise ValueError("crossover: taps_dev must hold an odd number of coefficients in [1, %d], got shape %s" % (CROSSOVER_MAX_TAPS, tuple(h.shape)))
    out = torch.empty((C, L), dtype=torch.float32, device=s.device)
    _lib.check(_lib.lib().p2phd_xover_fwd(_lib.ptr(s), max(ld_s, L), _lib.ptr(l), max(ld_l, L), float(level), _lib.ptr(h), h.numel(), C, L,
                                          _lib.ptr(out), max(L, 1), _lib.stream_ptr()), "xover_fwd")
    return out


_SPECIMG_TABLES = {}                                                        # (n_fft, device) -> twiddles and window on the device
_SPECIMG_LUT = {}                                                           # device -> the palette on the device


def _specimg_tables(n_fft, device):
    key = (int(n_fft), str(device))
    t = _SPECIMG_TABLES.get(key)
    if t is None:
        n = _lib.lib().p2phd_specimg_tables_floats(int(n_fft))
        if n == 0:
            _lib.check(-1, "specimg_tables_floats")
        host = torch.empty((n,), dtype=torch.float32)
        _lib.check(_lib.lib().p2phd_specimg_tables_fill(int(n_fft), ctypes.c_void_p(host.data_ptr())), "specimg_tables_fill")
        t = _SPECIMG_TABLES[key] = host.to(device)
    return t


def stft_db(rows, n_fft, hop):
    """rows [R, L] f32 on the GPU (rows contiguous, any row pitch) -> [R, F, K] f32, F = 1 + L // hop, K = n_fft // 2 + 1: the
    power of torch.stft(rows, n_fft, hop, window=hann_periodic, center=True, pad_mode='constant') in dB, scaled so that a
    full-scale sine reads 0 and floored at -200 (p2phd_stft_db).  L = 0: an empty [R, 0, K].  Nothing is waited for."""
    x, R, L, ld = _rows(rows, "stft_db: rows")
    lib = _lib.lib()
    F = 0
    if L > 0:
        F = lib.p2phd_stft_db_frames(L, int(n_fft), int(hop))
        if F == 0:
            _lib.check(-1, "stft_db_frames")
    db = torch.empty((R, F, int(n_fft) // 2 + 1), dtype=torch.float32, device=x.device)
    tables = _specimg_tables(n_fft, x.device) if L > 0 else None
    _lib.check(lib.p2phd_stft_db(_lib.ptr(x), max(ld, L), R, L, int(n_fft), int(hop), _lib.ptr(tables), _lib.ptr(db), _lib.stream_ptr()), "stft_db")
    return db


def spectrogram_rgb(db, top, range_db, width, height, gap):
    """db [R, F, K] f32 on the GPU -> the picture [R * height + (R - 1) * gap, width, 3] uint8 on the GPU: panel r shows
    db[r] with time left to right and bin 0 in its bottom row, every pixel the maximum of the frames and bins it covers, coloured
    by plans.spectrogram_lut from `top` - `range_db` (index 0) to `top` (index 255); `gap` grey rows between panels
    (p2phd_specimg_render).  `top`: a float32 tensor of one element on the GPU, which the kernel reads -- db.amax() for the
    picture's own maximum -- or a number.  Nothing is waited for."""
    d = _lib.require_gpu_tensor(db, "spectrogram_rgb: db", torch.float32)
    if d.dim() != 3 or d.shape[0] < 1 or d.shape[1] < 1:
        raise ValueError("spectrogram_rgb: expected [R, F, K] with at least one panel and one frame, got shape %s" % (tuple(d.shape),))
    R, F, K = d.shape
    if isinstance(top, torch.Tensor):
        top = _lib.require_gpu_tensor(top, "spectrogram_rgb: top", torch.float32)
        if top.numel() != 1:
            raise ValueError("spectrogram_rgb: top must hold one value, got shape %s" % (tuple(top.shape),))
    else:
        top = torch.full((1,), float(top), dtype=torch.float32, device=d.device)
    lib = _lib.lib()
    nbytes = lib.p2phd_specimg_image_bytes(R, int(width), int(height), int(gap))
    if nbytes == 0:
        _lib.check(-1, "specimg_image_bytes")
    lut = _SPECIMG_LUT.get(str(d.device))
    if lut is None:
        lut = _SPECIMG_LUT[str(d.device)] = torch.from_numpy(spectrogram_lut()).to(d.device)
    img = torch.empty((nbytes // (3 * int(width)), int(width), 3), dtype=torch.uint8, device=d.device)
    _lib.check(lib.p2phd_specimg_render(_lib.ptr(d), R, F, K, _lib.ptr(top), float(range_db), _lib.ptr(lut), int(width), int(height), int(gap),
                                        _lib.ptr(img), _lib.stream_ptr()), "specimg_render")
    return img


def loudness_coefficients(rate):
    """The K-weighting pair of p2phd_loudness_coeffs_fill as a float64 tensor of 10 on the host (no GPU needed): b0 b1 b2 a1 a2
    of the high shelf, then of the high-pass.  A rate the entry refuses (not a multiple of 10 in [8000, 384000]) is a ValueError."""
    try:
        rate = float(rate)
    except (TypeError, ValueError):
        raise ValueError("loudness_coefficients: the rate must be a number, got %r" % (rate,))
    out = torch.empty((10,), dtype=torch.float64)
    l = _lib.lib()
    if l.p2phd_loudness_coeffs_fill(rate, ctypes.c_void_p(out.data_ptr())) != 0:
        raise ValueError(l.p2phd_last_error().decode("utf-8", "replace"))
    return out


def loudness_hops(waveform, rate):
    """waveform [C, L] f32 on the GPU (rows contiguous, any row pitch) -> z [C, L // hop] float64 on the GPU, hop = rate // 10: per
    channel and 100 ms hop the energy of the K-weighted signal (p2phd_loudness_hops).  Nothing is waited for."""
    rate = check_loudness_rate(rate, "loudness_hops")
    w, C, L, ld = _rows(waveform, "loudness_hops: waveform")
    z = torch.empty((C, L // (rate // 10)), dtype=torch.float64, device=w.device)
    _lib.check(_lib.lib().p2phd_loudness_hops(_lib.ptr(w), L, C, max(ld, L), rate, _lib.ptr(z), _lib.stream_ptr()), "loudness_hops")
    return z


def loudness_gate(z, rate, weights=None, target=None, target_dev=None, max_gain_db=LOUDNESS_MAX_GAIN_DB, out=None):
    """z [C, J] float64 on the GPU (loudness_hops) -> (res4, gain) on the GPU, nothing waited for: res4 = float64
    {integrated loudness in LUFS, the loudest 400 ms block, the relative threshold, blocks behind both gates} and gain [1] f32, the
    factor that brings the clip to the wanted level within +-`max_gain_db` -- 1 without one, or where a level is not finite
    (p2phd_loudness_gate).  `weights`: one number per channel (None: all 1; plans.loudness_channel_weights).  The wanted level:
    `target_dev`, a float64 tensor on the GPU whose first element the kernel reads (another clip's res4), else `target` in LUFS,
    else none.  `out`: None, or a uint8 tensor of 40 bytes on the GPU that takes both (res4, then gain): the views are returned."""
    rate = check_loudness_rate(rate, "loudness_gate")
    zz = _lib.require_gpu_tensor(z, "loudness_gate: z", torch.float64)
    if zz.dim() != 2 or not 1 <= zz.shape[0] <= LOUDNESS_MAX_CHANNELS:
        raise ValueError("loudness_gate: expected z [C, J] with 1 <= C <= %d, got shape %s" % (LOUDNESS_MAX_CHANNELS, tuple(zz.shape)))
    C, J = zz.shape
    wbuf = None
    if weights is not None:
        wbuf = (ctypes.c_float * C)(*[float(v) for v in weights]) if len(weights) == C else None
        if wbuf is None:
            raise ValueError("loudness_gate: %d weights for %d channels" % (len(weights), C))
    if target_dev is not None:
        target_dev = _lib.require_gpu_tensor(target_dev, "loudness_gate: target_dev", torch.float64)
        if target_dev.numel() < 1:
            raise ValueError("loudness_gate: target_dev is empty")
    if out is None:
        out = torch.empty((40,), dtype=torch.uint8, device=zz.device)
    else:
        out = _lib.require_gpu_tensor(out, "loudness_gate: out", torch.uint8)
        if out.numel() != 40:
            raise ValueError("loudness_gate: out must hold 40 bytes, got %d" % out.numel())
    res4, gain = _loudness_views(out)
    _lib.check(_lib.lib().p2phd_loudness_gate(_lib.ptr(zz), J, C, rate, wbuf, float('nan') if target is None else float(target),
                                              _lib.ptr(target_dev), float(max_gain_db), _lib.ptr(res4), _lib.ptr(gain), _lib.stream_ptr()),
               "loudness_gate")
    return res4, gain


def _loudness_views(buf):
    """The packed result of one loudness_gate -- res4 [4] f64 | gain f32 | 4 spare bytes, on the device or its copy on the host ->
    (res4, gain) as typed views."""
    return buf[:32].view(torch.float64), buf[32:36].view(torch.float32)


def loudness(waveform, rate, weights=None, target=None, target_dev=None, max_gain_db=LOUDNESS_MAX_GAIN_DB, out=None):
    """loudness_hops and loudness_gate in a row: waveform [C, L] f32 on the GPU -> (res4, gain) on the GPU.  Two launches of the
    family "loudness" (one where the clip is shorter than a hop), nothing is waited for."""
    return loudness_gate(loudness_hops(waveform, rate), rate, weights, target, target_dev, max_gain_db, out)


LOUDNESS_SHORT_TERM_HOPS = 30                                               # a short-term block: 3 s of 100 ms hops


def loudness_short_term(z, rate, weights=None, gain_dev=None):
    """z [C, J] float64 on the GPU (loudness_hops) -> p [max(J - 29, 0)] float64 on the GPU, nothing waited for: the power of every
    3 s block of 30 hops at a 100 ms step, the channels weighted as in loudness_gate (p2phd_loudness_short_term).  `gain_dev`: None,
    or a float32 tensor on the GPU whose first element the kernel reads (a loudness_gate's gain): the powers are then those of the
    clip times that gain.  One launch of the family "loudness"; none for a clip under 3 s."""
    rate = check_loudness_rate(rate, "loudness_short_term")
    zz = _lib.require_gpu_tensor(z, "loudness_short_term: z", torch.float64)
    if zz.dim() != 2 or not 1 <= zz.shape[0] <= LOUDNESS_MAX_CHANNELS:
        raise ValueError("loudness_short_term: expected z [C, J] with 1 <= C <= %d, got shape %s" % (LOUDNESS_MAX_CHANNELS, tuple(zz.shape)))
    C, J = zz.shape
    wbuf = None
    if weights is not None:
        wbuf = (ctypes.c_float * C)(*[float(v) for v in weights]) if len(weights) == C else None
        if wbuf is None:
            raise ValueError("loudness_short_term: %d weights for %d channels" % (len(weights), C))
    if gain_dev is not None:
        gain_dev = _lib.require_gpu_tensor(gain_dev, "loudness_short_term: gain_dev", torch.float32)
        if gain_dev.numel() < 1:
            raise ValueError("loudness_short_term: gain_dev is empty")
    p = torch.empty((max(J - (LOUDNESS_SHORT_TERM_HOPS - 1), 0),), dtype=torch.float64, device=zz.device)
    _lib.check(_lib.lib().p2phd_loudness_short_term(_lib.ptr(zz), J, C, rate, wbuf, _lib.ptr(gain_dev), _lib.ptr(p), _lib.stream_ptr()),
               "loudness_short_term")
    return p


def loudness_range(p, out=None):
    """p [NS] float64 on the GPU (loudness_short_term) -> res8 [8] float64 on the GPU, nothing waited for: {the loudness range in LU
    after EBU Tech 3342 (gates at -70 LUFS and 20 LU under the mean of what passed, the 10th to the 95th percentile of the rest), the
    level of the low and of the high percentile in LUFS, the relative threshold, blocks behind both gates, the loudest block (the
    maximum short-term loudness), the two selected powers} (p2phd_loudness_range).  No block: range 0, levels -inf; a NaN block:
    range and levels NaN.  `out`: None, or a float64 tensor of 8 on the GPU that takes the result.  One launch of the family
    "loudness", for every NS; `p` is only read."""
    pp = _lib.require_gpu_tensor(p, "loudness_range: p", torch.float64)
    if pp.dim() != 1:
        raise ValueError("loudness_range: expected p [NS], got shape %s" % (tuple(pp.shape),))
    if out is None:
        out = torch.empty((8,), dtype=torch.float64, device=pp.device)
    else:
        out = _lib.require_gpu_tensor(out, "loudness_range: out", torch.float64)
        if out.numel() != 8:
            raise ValueError("loudness_range: out must hold 8 float64, got %d" % out.numel())
    _lib.check(_lib.lib().p2phd_loudness_range(_lib.ptr(pp), pp.numel(), _lib.ptr(out), _lib.stream_ptr()), "loudness_range")
    return out


def loudness_blocks(z, rate, weights=None, out=None):
    """z [C, J] float64 on the GPU (loudness_hops) -> p [max(J - 3, 0)] float64 on the GPU, nothing waited for: the power of every
    400 ms block of four hops at a 100 ms step, the channels weighted as in loudness_gate, whose own expression it is -- p[b] holds
    the bits the gate computes in place (p2phd_loudness_blocks).  `out`: None, or a contiguous float64 tensor of exactly that many
    elements on the GPU, for instance a slice of the buffer that collects the blocks of every file of a folder: it takes the powers
    and is returned.  One launch of the family "loudness"; none for a clip under 400 ms."""
    rate = check_loudness_rate(rate, "loudness_blocks")
    zz = _lib.require_gpu_tensor(z, "loudness_blocks: z", torch.float64)
    if zz.dim() != 2 or not 1 <= zz.shape[0] <= LOUDNESS_MAX_CHANNELS:
        raise ValueError("loudness_blocks: expected z [C, J] with 1 <= C <= %d, got shape %s" % (LOUDNESS_MAX_CHANNELS, tuple(zz.shape)))
    C, J = zz.shape
    wbuf = None
    if weights is not None:
        wbuf = (ctypes.c_float * C)(*[float(v) for v in weights]) if len(weights) == C else None
        if wbuf is None:
            raise ValueError("loudness_blocks: %d weights for %d channels" % (len(weights), C))
    NB = max(J - 3, 0)
    if out is None:
        p = torch.empty((NB,), dtype=torch.float64, device=zz.device)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float64:
            raise _lib.P2PHDError("loudness_blocks: out: expected a float64 tensor on the GPU (this build has no CPU path)")
        if out.dim() != 1 or out.numel() != NB or not out.is_contiguous():
            raise ValueError("loudness_blocks: out must be a contiguous float64 tensor of %d elements, got shape %s" % (NB, tuple(out.shape)))
        p = out
    _lib.check(_lib.lib().p2phd_loudness_blocks(_lib.ptr(zz), J, C, rate, wbuf, _lib.ptr(p) if NB else None, _lib.stream_ptr()), "loudness_blocks")
    return p


def loudness_gate_blocks(p, target=None, target_dev=None, max_gain_db=LOUDNESS_MAX_GAIN_DB, out=None):
    """p [NB] float64 on the GPU (loudness_blocks; the blocks of one file, or of every file of a folder one behind the other) ->
    (res4, gain) on the GPU as loudness_gate returns them, nothing waited for: both gates over these blocks as one programme -- the
    album loudness of EBU R 128 (p2phd_loudness_gate_blocks).  On the blocks of one file the bits are loudness_gate's on that file's z.
    `target`, `target_dev`, `max_gain_db`, `out` (40 bytes): loudness_gate's.  One launch of the family "loudness", for every NB;
    `p` is only read."""
    pp = _lib.require_gpu_tensor(p, "loudness_gate_blocks: p", torch.float64)
    if pp.dim() != 1:
        raise ValueError("loudness_gate_blocks: expected p [NB], got shape %s" % (tuple(pp.shape),))
    if target_dev is not None:
        target_dev = _lib.require_gpu_tensor(target_dev, "loudness_gate_blocks: target_dev", torch.float64)
        if target_dev.numel() < 1:
            raise ValueError("loudness_gate_blocks: target_dev is empty")
    if out is None:
        out = torch.empty((40,), dtype=torch.uint8, device=pp.device)
    else:
        out = _lib.require_gpu_tensor(out, "loudness_gate_blocks: out", torch.uint8)
        if out.numel() != 40:
            raise ValueError("loudness_gate_blocks: out must hold 40 bytes, got %d" % out.numel())
    res4, gain = _loudness_views(out)
    _lib.check(_lib.lib().p2phd_loudness_gate_blocks(_lib.ptr(pp) if pp.numel() else None, pp.numel(), float('nan') if target is None else float(target),
                                                     _lib.ptr(target_dev), float(max_gain_db), _lib.ptr(res4), _lib.ptr(gain), _lib.stream_ptr()),
               "loudness_gate_blocks")
    return res4, gain


_TRUEPEAK_TABLES = {}                                                    # (factor, taps per phase, beta, device) -> the table on the device


def true_peak_coefficients(factor, taps_per_phase, beta):
    """The polyphase table of p2phd_truepeak_taps_fill as a float32 tensor [factor, taps_per_phase] on the host (no GPU needed)."""
    c = torch.empty((max(int(factor), 1), max(int(taps_per_phase), 1)), dtype=torch.float32)
    _lib.check(_lib.lib().p2phd_truepeak_taps_fill(int(factor), int(taps_per_phase), float(beta), ctypes.c_void_p(c.data_ptr())),
               "truepeak_taps_fill")
    return c


def _true_peak_views(buf, C):
    """The packed true-peak buffer -- tpeak[C] f32 | gain f32, 4 * C + 4 bytes, on the device or its copy on the host ->
    (tpeak, gain) as typed views."""
    return buf[:4 * C].view(torch.float32), buf[4 * C:4 * C + 4].view(torch.float32)


def _true_peak_table(plan, device):
    """The table of truepeak_plan's `plan` on `device`, filled once."""
    key = (plan['factor'], plan['taps_per_phase'], plan['beta'], str(device))
    table = _TRUEPEAK_TABLES.get(key)
    if table is None:
        table = _TRUEPEAK_TABLES[key] = true_peak_coefficients(*key[:3]).to(device)
    return table


def _true_peaks_packed(waveform, rate, ceiling, who):
    """-> (the two results of true_peaks as views of one byte buffer, the buffer): one copy brings both back."""
    plan = truepeak_plan(rate)
    ceiling = 1.0 if ceiling is None else float(ceiling)
    if not 0.0 < ceiling < float('inf'):
        raise ValueError("%s: ceiling must be a finite level > 0, or None for 1, got %r" % (who, ceiling))
    w, C, L, ld = _rows(waveform, "%s: waveform" % who)
    table = _true_peak_table(plan, w.device)
    buf = torch.empty((4 * C + 4,), dtype=torch.uint8, device=w.device)
    tpeak, gain = views = _true_peak_views(buf, C)
    _lib.check(_lib.lib().p2phd_truepeak(_lib.ptr(w), L, C, max(ld, L), _lib.ptr(table), plan['factor'], plan['taps_per_phase'], ceiling,
                                         _lib.ptr(tpeak), _lib.ptr(gain), _lib.stream_ptr()), "truepeak")
    return views, buf


def true_peaks(waveform, rate, ceiling=None):
    """The true peak after ITU-R BS.1770-4 Annex 2 of waveform [C, L] f32 on the GPU (rows contiguous, any row pitch) at `rate` ->
    (tpeak [C] f32, gain [1] f32) on the GPU, nothing waited for: per channel the largest magnitude of the clip oversampled to at
    least 192 kHz (plans.truepeak_plan; a linear level, never below pcm_peaks' peak; NaN / inf samples count as 0), and the one
    gain for all channels that brings the largest of them down to `ceiling` (a linear level; None: 1.0) -- 1 where it already
    is (p2phd_truepeak).  One launch of the family "truepeak"; the same bits on every run."""
    return _true_peaks_packed(waveform, rate, ceiling, "true_peaks")[0]


def ltas(rows, n_fft, hop):
    """rows [R, L] f32 on the GPU (rows contiguous, any row pitch) -> psd [R, K] float64 on the GPU, K = n_fft // 2 + 1: the long-term
    average spectrum, the float64 sum in a fixed order of the fp32 powers |X|^2 (4 / n_fft)^2 (a full-scale sine carries 1 per
    frame) of the F = 1 + (L - n_fft) // hop frames of torch.stft(rows, n_fft, hop, window=hann_periodic, center=False) -- only
    frames that lie wholly inside the clip (p2phd_ltas).  L < n_fft: zeros.  One launch of the family "bandwidth" (none where F =
    0); the same bits on every run, and row r of a call is the call on that row.  Nothing is waited for."""
    x, R, L, ld = _rows(rows, "ltas: rows")
    lib = _lib.lib()
    F = lib.p2phd_ltas_frames(L, int(n_fft), int(hop))
    if F < 0:
        _lib.check(-1, "ltas_frames")
    psd = torch.empty((R, int(n_fft) // 2 + 1), dtype=torch.float64, device=x.device)
    tables = work = None
    if F > 0:
        tables = _specimg_tables(n_fft, x.device)
        work = torch.empty((lib.p2phd_ltas_workspace_bytes(R, L, int(n_fft), int(hop)),), dtype=torch.uint8, device=x.device)
    _lib.check(lib.p2phd_ltas(_lib.ptr(x), max(ld, L), R, L, int(n_fft), int(hop), _lib.ptr(tables), _lib.ptr(psd), _lib.ptr(work),
                              _lib.stream_ptr()), "ltas")
    return psd


def bandwidth_detect(psd, rows_per_group, band_bins, threshold_db, out=None):
    """psd [G * Q, K] float64 on the GPU (ltas), Q = `rows_per_group` consecutive rows -- the channels of a clip -- forming one
    programme -> res [G, 4] float64 on the GPU, nothing waited for: {k_top, b_top, ref, thr} -- the levels of the bands of
    `band_bins` bins of the group's summed spectrum, ref the largest, thr = ref * 10^(-threshold_db / 10), b_top the highest band
    above thr and k_top the highest bin of that band above thr: where the band ends; {-1, -1, ref, thr} where no band passes
    (p2phd_bandwidth, whose float64 arithmetic include/p2phd.h writes down).  `out`: None, or a contiguous float64 tensor of G * 4
    on the GPU that takes the result.  One launch of the family "bandwidth"."""
    pp = _lib.require_gpu_tensor(psd, "bandwidth_detect: psd", torch.float64)
    Q = int(rows_per_group)
    if pp.dim() != 2 or Q < 1 or pp.shape[0] % Q:
        raise ValueError("bandwidth_detect: expected psd [G * Q, K] with Q = %d, got shape %s" % (Q, tuple(pp.shape)))
    G, K = pp.shape[0] // Q, pp.shape[1]
    if out is None:
        out = torch.empty((G, 4), dtype=torch.float64, device=pp.device)
    else:
        out = _lib.require_gpu_tensor(out, "bandwidth_detect: out", torch.float64)
        if out.numel() != G * 4:
            raise ValueError("bandwidth_detect: out must hold %d float64, got %d" % (G * 4, out.numel()))
    _lib.check(_lib.lib().p2phd_bandwidth(_lib.ptr(pp), G, Q, K, int(band_bins), bandwidth_rel(threshold_db), _lib.ptr(out), _lib.stream_ptr()),
               "bandwidth")
    return out.view(G, 4)


def bandwidth(waveform, rate, plan=None, out=None):
    """ltas and bandwidth_detect in a row: waveform [C, L] f32 on the GPU at `rate`, all channels one programme -> res [4] float64
    on the GPU: res[0] * rate / n_fft is where the clip's band ends, in Hz (res[0] = -1: nothing passed -- silence, or a clip
    shorter than n_fft).  `plan`: {'n_fft', 'hop', 'band_bins', 'threshold_db'} (plans.check_bandwidth; None: BANDWIDTH_DEFAULTS).
    `rate` does not enter the device work: the figure is a bin.  `out`: None, or a float64 tensor of 4 on the GPU that takes the
    result.  Two launches of the family "bandwidth" (one where the clip is shorter than n_fft), nothing is waited for."""
    p = BANDWIDTH_DEFAULTS if plan is None else plan
    if isinstance(rate, bool) or not isinstance(rate, (int, float)) or not 0.0 < rate < float('inf'):
        raise ValueError("bandwidth: the rate must be a number > 0, got %r" % (rate,))
    psd = ltas(waveform, p['n_fft'], p['hop'])
    return bandwidth_detect(psd, psd.shape[0], p['band_bins'], p['threshold_db'], out).view(4)


def cross_spectrum(rows, n_fft, hop):
    """rows [2 G, L] f32 on the GPU (rows contiguous, any row pitch), rows 2 g and 2 g + 1 the left and right channel of pair g
    -> xs [G, 4, K] float64 on the GPU, K = n_fft // 2 + 1: the long-term cross-spectrum over ltas's frames (only those wholly
    inside the clip), window and scale -- per bin the float64 sums in a fixed order of |A|^2, |B|^2, Re(A conj B) and Im(A conj B),
    A and B the two channels' transforms (p2phd_xspec).  L < n_fft: zeros.  One launch of the family "stereo" (none where F = 0);
    the same bits on every run, and pair g of a call is the call on that pair.  Nothing is waited for."""
    x, R, L, ld = _rows(rows, "cross_spectrum: rows")
    if R % 2:
        raise ValueError("cross_spectrum: expected [2 * G, L], the left and right rows of G pairs, got shape %s" % (tuple(x.shape),))
    G = R // 2
    lib = _lib.lib()
    F = lib.p2phd_ltas_frames(L, int(n_fft), int(hop))
    if F < 0:
        _lib.check(-1, "ltas_frames")
    xs = torch.empty((G, 4, int(n_fft) // 2 + 1), dtype=torch.float64, device=x.device)
    tables = work = None
    if F > 0:
        tables = _specimg_tables(n_fft, x.device)
        work = torch.empty((lib.p2phd_xspec_workspace_bytes(G, L, int(n_fft), int(hop)),), dtype=torch.uint8, device=x.device)
    _lib.check(lib.p2phd_xspec(_lib.ptr(x), max(ld, L), G, L, int(n_fft), int(hop), _lib.ptr(tables), _lib.ptr(xs), _lib.ptr(work),
                               _lib.stream_ptr()), "xspec")
    return xs


def stereo_bands(xs, k_split, out=None):
    """xs [G, 4, K] float64 on the GPU (cross_spectrum) -> res [G, 8] float64 on the GPU, nothing waited for: {S_ll, S_rr, Re, Im}
    summed over the bins [0, k_split), then over [k_split, K) (p2phd_stereo_bands, whose float64 order include/p2phd.h writes down).
    `out`: None, or a contiguous float64 tensor of G * 8 on the GPU that takes the result.  One launch of the family "stereo"."""
    xx = _lib.require_gpu_tensor(xs, "stereo_bands: xs", torch.float64)
    if xx.dim() != 3 or xx.shape[1] != 4:
        raise ValueError("stereo_bands: expected xs [G, 4, K], got shape %s" % (tuple(xx.shape),))
    G, K = xx.shape[0], xx.shape[2]
    if out is None:
        out = torch.empty((G, 8), dtype=torch.float64, device=xx.device)
    else:
        out = _lib.require_gpu_tensor(out, "stereo_bands: out", torch.float64)
        if out.numel() != G * 8:
            raise ValueError("stereo_bands: out must hold %d float64, got %d" % (G * 8, out.numel()))
    _lib.check(_lib.lib().p2phd_stereo_bands(_lib.ptr(xx), G, K, int(k_split), _lib.ptr(out), _lib.stream_ptr()), "stereo_bands")
    return out.view(G, 8)


def stereo_image(waveform, hr_rate, lr_rate, plan=None, out=None):
    """cross_spectrum and stereo_bands in a row: waveform [2, L] f32 on the GPU at `hr_rate` -> res [8] float64 on the GPU, the four
    sums below and the four at and above the low rate's Nyquist frequency (plans.stereo_split_bin; plans.stereo_figures turns the
    fetched eight into correlation, coherence, side level and balance).  `plan`: {'n_fft', 'hop'} (plans.check_stereo_report; None:
    STEREO_DEFAULTS).  `out`: None, or a float64 tensor of 8 on the GPU that takes the result.  Two launches of the family "stereo"
    (one where the clip is shorter than n_fft), nothing is waited for.  Anything but two rows is a ValueError."""
    p = STEREO_DEFAULTS if plan is None else plan
    if not isinstance(waveform, torch.Tensor) or waveform.dim() != 2 or waveform.shape[0] != 2:
        raise ValueError("stereo_image: expected a waveform [2, L], left and right, got shape %s"
                         % (tuple(waveform.shape) if isinstance(waveform, torch.Tensor) else type(waveform).__name__,))
    k_split = stereo_split_bin(hr_rate, lr_rate, p['n_fft'])
    return stereo_bands(cross_spectrum(waveform, p['n_fft'], p['hop']), k_split, out).view(8)


def stereo_matrix(x, a, guard_side=False, out=None):
    """x [2, L] f32 on the GPU (rows contiguous, any row pitch) -> a new [2, L]: row 0 = a * (x0 + s), row 1 = a * (x0 - s) with
    s = x1 and, with `guard_side`, +0 where x1 is not finite (p2phd_stereo_matrix; plain fp32, what numpy float32 gives).  a = 0.5
    encodes left / right as mid / side, a = 1 with the guard decodes.  `out`: None, or a [2, L] f32 tensor on the GPU that takes
    the result -- `x` itself is allowed (in place), any other overlap is not.  One launch of the family "stereo" (none for L = 0)."""
    xx, C, L, ld = _rows(x, "stereo_matrix: x")
    if C != 2:
        raise ValueError("stereo_matrix: expected [2, L], got shape %s" % (tuple(xx.shape),))
    if out is None:
        out = torch.empty((2, L), dtype=torch.float32, device=xx.device)
    oo, Co, Lo, ld_o = _rows(out, "stereo_matrix: out")
    if (Co, Lo) != (2, L):
        raise ValueError("stereo_matrix: out must have the shape of x, got %s and %s" % (tuple(oo.shape), tuple(xx.shape)))
    _lib.check(_lib.lib().p2phd_stereo_matrix(_lib.ptr(xx), max(ld, L), L, float(a), 1 if guard_side else 0, _lib.ptr(oo), max(ld_o, L),
                                              _lib.stream_ptr()), "stereo_matrix")
    return oo


_RATECONV_TABLES = {}                                                      # (o, n, taps per phase, beta, cutoff, device) -> the table on the device


def rateconv_plan(in_rate, out_rate, passband=None, atten_db=None):
    """The filter of the output stage's rate converter, host arithmetic only (p2phd_rateconv_plan, no GPU needed) -> {'in_rate',
    'out_rate', 'o', 'n' (the rates over their greatest common divisor), 'taps_per_phase', 'beta', 'cutoff' (what
    rateconv_coefficients takes: min(in, out) / in), 'passband_hz' (flat up to here), 'stopband_hz' (`atten_db` down from here; what
    aliases or images lies above passband_hz), 'atten_db'}.  `passband`: the flat part as a fraction of the lower rate's Nyquist
    frequency, `atten_db`: the stopband attenuation (None: RATECONV_DEFAULTS).  Equal rates, a rate that is no int >= 1 and a plan
    the entry refuses -- rates so far apart, or with so small a common divisor, that the table is not built -- are a ValueError
    with its text."""
    for name, v in (('in_rate', in_rate), ('out_rate', out_rate)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v < 2 ** 31:
            raise ValueError("rateconv_plan: %s must be an int >= 1, got %r" % (name, v))
    passband = RATECONV_DEFAULTS['passband'] if passband is None else passband
    atten_db = RATECONV_DEFAULTS['atten_db'] if atten_db is None else atten_db
    for name, v in (('passband', passband), ('atten_db', atten_db)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError("rateconv_plan: %s must be a number, got %r" % (name, v))
    o, n, P, beta = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    l = _lib.lib()
    if l.p2phd_rateconv_plan(in_rate, out_rate, float(passband), float(atten_db), ctypes.byref(o), ctypes.byref(n), ctypes.byref(P),
                             ctypes.byref(beta)) != 0:
        raise ValueError(l.p2phd_last_error().decode("utf-8", "replace"))
    nyquist = min(in_rate, out_rate) / 2.0
    return {'in_rate': in_rate, 'out_rate': out_rate, 'o': o.value, 'n': n.value, 'taps_per_phase': P.value, 'beta': beta.value,
            'cutoff': min(in_rate, out_rate) / float(in_rate), 'passband_hz': float(passband) * nyquist,
            'stopband_hz': 2.0 * nyquist - float(passband) * nyquist, 'atten_db': float(atten_db)}


def rateconv_coefficients(plan):
    """The polyphase table of p2phd_rateconv_taps_fill for rateconv_plan's `plan` as a float32 tensor [n, taps_per_phase] on the host
    (no GPU needed)."""
    c = torch.empty((max(int(plan['n']), 1), max(int(plan['taps_per_phase']), 1)), dtype=torch.float32)
    l = _lib.lib()
    if l.p2phd_rateconv_taps_fill(int(plan['o']), int(plan['n']), int(plan['taps_per_phase']), float(plan['beta']), float(plan['cutoff']),
                                  ctypes.c_void_p(c.data_ptr())) != 0:
        raise ValueError(l.p2phd_last_error().decode("utf-8", "replace"))
    return c


def rateconv_out_len(frames, in_rate, out_rate):
    """ceil(frames * out_rate / in_rate) in exact arithmetic (p2phd_rateconv_out_len): the samples of a converted row."""
    l = _lib.lib()
    v = l.p2phd_rateconv_out_len(int(frames), int(in_rate), int(out_rate))
    if v < 0:
        raise ValueError(l.p2phd_last_error().decode("utf-8", "replace"))
    return v


def rate_convert(x, in_rate, out_rate, plan=None, table=None, out=None):
    """x [C, L] f32 on the GPU (rows contiguous, any row pitch) at `in_rate` -> [C, ceil(L out_rate / in_rate)] at `out_rate`: the
    rational polyphase converter of csrc/rateconv.hip, every output one fp32 fma chain over the taps in ascending order
    (p2phd_rateconv_fwd).  Equal rates: `x` itself, and nothing is launched.  `plan`: rateconv_plan's dict (None: the one of the two
    rates with RATECONV_DEFAULTS); `table`: the [n, taps_per_phase] f32 table on the GPU where the caller brings its own (None:
    rateconv_coefficients(plan), filled once per device); `out`: None, or a [C, L_out] f32 tensor on the GPU (rows contiguous, any
    row pitch) that takes the result and must not overlap `x`.  One launch of the family "rateconv" (none for L = 0), nothing is
    waited for."""
    if in_rate == out_rate:
        return x
    if plan is None:
        plan = rateconv_plan(in_rate, out_rate)
    elif (plan['in_rate'], plan['out_rate']) != (in_rate, out_rate):
        raise ValueError("rate_convert: the plan is one of %r -> %r Hz, the call says %r -> %r" % (plan['in_rate'], plan['out_rate'], in_rate, out_rate))
    o, n, P = int(plan['o']), int(plan['n']), int(plan['taps_per_phase'])
    w, C, L, ld = _rows(x, "rate_convert: x")
    if table is None:
        key = (o, n, P, plan['beta'], plan['cutoff'], str(w.device))
        table = _RATECONV_TABLES.get(key)
        if table is None:
            table = _RATECONV_TABLES[key] = rateconv_coefficients(plan).to(w.device)
    else:
        table = _lib.require_gpu_tensor(table, "rate_convert: table", torch.float32)
        if table.numel() != n * P:
            raise ValueError("rate_convert: the table must hold n * taps_per_phase = %d contiguous floats, got shape %s" % (n * P, tuple(table.shape)))
    L_out = rateconv_out_len(L, o, n)
    if out is None:
        out = torch.empty((C, L_out), dtype=torch.float32, device=w.device)
    oo, Co, Lo, ld_o = _rows(out, "rate_convert: out")
    if (Co, Lo) != (C, L_out):
        raise ValueError("rate_convert: out must have the shape %s, got %s" % ((C, L_out), tuple(oo.shape)))
    _lib.check(_lib.lib().p2phd_rateconv_fwd(_lib.ptr(w), L, C, max(ld, L), _lib.ptr(table), o, n, P, _lib.ptr(oo), L_out, max(ld_o, L_out),
                                             _lib.stream_ptr()), "rateconv_fwd")
    return oo


_LIMITER_WINDOWS = {}                                                    # (lookahead, device) -> the window on the device


def limiter_window(lookahead):
    """The smoothing window of p2phd_limiter_window_fill as a float32 tensor of `lookahead` + 1 on the host (no GPU needed):
    a Hann window without its zeros, sum 1, symmetric bit for bit."""
    A = int(lookahead)
    w = torch.empty((max(A, 0) + 1,), dtype=torch.float32)
    l = _lib.lib()
    if l.p2phd_limiter_window_fill(A, ctypes.c_void_p(w.data_ptr())) != 0:
        raise ValueError(l.p2phd_last_error().decode("utf-8", "replace"))
    return w


def _limiter_ceiling(ceiling, who):
    ceiling = 1.0 if ceiling is None else float(ceiling)
    if not 0.0 < ceiling < float('inf'):
        raise ValueError("%s: ceiling must be a finite level > 0, or None for 1, got %r" % (who, ceiling))
    return ceiling


def limiter_envelope(waveform, rate_or_plan, ceiling=None, peak_out=None):
    """waveform [C, L] f32 on the GPU (rows contiguous, any row pitch) -> (r [L] f32, peak [1] f32) on the GPU, nothing waited for:
    r[i] = the gain that alone would bring sample i and the oversampled crests on both of its sides, in every channel, to
    `ceiling` (a linear level; None: 1.0) -- 1 where they are under it -- and the clip's true peak, the largest of true_peaks'
    (p2phd_limiter_envelope).  `rate_or_plan`: the clip's rate (plans.truepeak_plan picks the interpolator), or such a plan as a
    dict, with 'table' (the [factor, taps_per_phase] f32 table on the GPU) where the caller brings its own.  `peak_out`: None, or a
    float32 tensor of one element on the GPU that takes the peak.  One launch of the family "limiter"."""
    plan = dict(rate_or_plan) if isinstance(rate_or_plan, dict) else truepeak_plan(rate_or_plan)
    ceiling = _limiter_ceiling(ceiling, "limiter_envelope")
    w, C, L, ld = _rows(waveform, "limiter_envelope: waveform")
    table = plan.get('table')
    if table is None:
        table = _true_peak_table(plan, w.device)
    else:
        table = _lib.require_gpu_tensor(table, "limiter_envelope: table", torch.float32)
        if not table.is_contiguous() or table.numel() != int(plan['factor']) * int(plan['taps_per_phase']):
            raise ValueError("limiter_envelope: the table must hold factor * taps_per_phase contiguous floats, got shape %s" % (tuple(table.shape),))
    r = torch.empty((L,), dtype=torch.float32, device=w.device)
    if peak_out is None:
        peak_out = torch.empty((1,), dtype=torch.float32, device=w.device)
    else:
        peak_out = _lib.require_gpu_tensor(peak_out, "limiter_envelope: peak_out", torch.float32)
        if peak_out.numel() != 1:
            raise ValueError("limiter_envelope: peak_out must hold one value, got shape %s" % (tuple(peak_out.shape),))
    _lib.check(_lib.lib().p2phd_limiter_envelope(_lib.ptr(w), L, C, max(ld, L), _lib.ptr(table), int(plan['factor']), int(plan['taps_per_phase']),
                                                 ceiling, _lib.ptr(r), _lib.ptr(peak_out), _lib.stream_ptr()), "limiter_envelope")
    return r, peak_out


def _limiter_stats_views(buf):
    """The 8 bytes of the limiter's statistics, on the device or their copy on the host -> (the smallest g as f32 [1], the number
    of reduced samples [1]: the u32's bits in an int32, & 0xFFFFFFFF reads them) as typed views."""
    return buf[:4].view(torch.float32), buf[4:8].view(torch.int32)


def limiter_apply(waveform, r, plan, window_dev=None, stats_out=None, want_g=True):
    """waveform [C, L] f32 on the GPU (rows contiguous, any row pitch), r [L] f32 on the GPU (limiter_envelope's, or any values in
    (0, 1]), plan {'lookahead': A, 'hold': H} (plans.limiter_plan) -> (out [C, L], g [L], stats) on the GPU, nothing waited for:
    the gain curve g -- the smoothed sliding minimum of r over H samples back and A ahead, never above r -- out = waveform * g in a
    new buffer, and stats, a uint8 tensor of 8 bytes: the smallest g (f32) and the number of samples with g < 1 (u32)
    (p2phd_limiter_apply).  `window_dev`: A + 1 f32 on the GPU (None: limiter_window(A), filled once per device); `stats_out`:
    None, or the 8-byte uint8 tensor on the GPU that takes the statistics; `want_g` False: g is not written and None is returned
    for it.  One launch of the family "limiter"."""
    A, H = plan['lookahead'], plan['hold']
    for name, v, lo, hi in (('lookahead', A, 1, LIMITER_MAX_LOOKAHEAD), ('hold', H, 0, LIMITER_MAX_HOLD)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError("limiter_apply: %s must be an int in [%d, %d], got %r" % (name, lo, hi, v))
    w, C, L, ld = _rows(waveform, "limiter_apply: waveform")
    rr = _lib.require_gpu_tensor(r, "limiter_apply: r", torch.float32)
    if rr.dim() != 1 or rr.numel() != L or not rr.is_contiguous():
        raise ValueError("limiter_apply: r must hold one contiguous value per sample (%d), got shape %s" % (L, tuple(rr.shape)))
    if window_dev is None:
        key = (A, str(w.device))
        window_dev = _LIMITER_WINDOWS.get(key)
        if window_dev is None:
            window_dev = _LIMITER_WINDOWS[key] = limiter_window(A).to(w.device)
    else:
        window_dev = _lib.require_gpu_tensor(window_dev, "limiter_apply: window_dev", torch.float32)
        if window_dev.dim() != 1 or window_dev.numel() != A + 1 or not window_dev.is_contiguous():
            raise ValueError("limiter_apply: window_dev must hold lookahead + 1 = %d contiguous floats, got shape %s" % (A + 1, tuple(window_dev.shape)))
    if stats_out is None:
        stats_out = torch.empty((8,), dtype=torch.uint8, device=w.device)
    else:
        stats_out = _lib.require_gpu_tensor(stats_out, "limiter_apply: stats_out", torch.uint8)
        if stats_out.numel() != 8:
            raise ValueError("limiter_apply: stats_out must hold 8 bytes, got %d" % stats_out.numel())
    out = torch.empty((C, L), dtype=torch.float32, device=w.device)
    g = torch.empty((L,), dtype=torch.float32, device=w.device) if want_g else None
    _lib.check(_lib.lib().p2phd_limiter_apply(_lib.ptr(w), L, C, max(ld, L), _lib.ptr(rr), A, H, _lib.ptr(window_dev), _lib.ptr(out), max(L, 1),
                                              _lib.ptr(g), _lib.ptr(stats_out), _lib.stream_ptr()), "limiter_apply")
    return out, g, stats_out


def limit(waveform, rate, ceiling=None, lookahead_ms=None, hold_ms=None):
    """limiter_envelope and limiter_apply in a row: waveform [C, L] f32 on the GPU at `rate` -> (out [C, L], g [L], stats, peak
    [1]) on the GPU -- the clip with its crests held at `ceiling` (a linear level; None: 1.0) by a gain curve that looks
    `lookahead_ms` ahead and holds `hold_ms` (plans.limiter_plan), the curve, its statistics (limiter_apply) and the true peak the
    clip came with.  The result's own true peak may lie a rounding over the ceiling: true_peaks' gain behind it removes that.  Two
    launches of the family "limiter", nothing is waited for."""
    plan = limiter_plan(rate, lookahead_ms, hold_ms)
    r, peak = limiter_envelope(waveform, rate, ceiling)
    return limiter_apply(waveform, r, plan) + (peak,)


def speech_level_consts(rate):
    """The constants of p2phd_speechlevel_consts_fill on the host (no GPU needed) -> (float64 tensor of 8: g, h, gL, hL, M, the lowest
    threshold, L, I; the hangover I in samples as an int)."""
    rate = check_speech_level_rate(rate, "speech_level_consts")
    out = torch.empty(8, dtype=torch.float64)
    hang = ctypes.c_int32(0)
    _lib.check(_lib.lib().p2phd_speechlevel_consts_fill(rate, ctypes.c_void_p(out.data_ptr()), ctypes.byref(hang)), "speech_level_consts")
    return out, int(hang.value)


def speech_level_envelope(waveform, rate, m=None, workspace=None):
    """waveform [C, L] f32 on the GPU (rows contiguous, any row pitch) -> (m [C, L] uint8, sq [C] float64) on the GPU, nothing
    waited for: per sample the number of thresholds the two-pole envelope stands at or over, per row the energy
    (p2phd_speechlevel_envelope).  `m`: None, or a uint8 tensor [C, >= L] with contiguous rows that takes the indices (its first
    L columns are returned); `workspace`: None, or a uint8 tensor of at least the queried bytes.  One launch of the family
    "speechlevel"; none for an empty clip."""
    rate = check_speech_level_rate(rate, "speech_level_envelope")
    w, C, L, ld = _rows(waveform, "speech_level_envelope: waveform")
    if C > SPEECH_LEVEL_KERNEL_CHANNELS:
        raise ValueError("speech_level_envelope: at most %d rows, got %d" % (SPEECH_LEVEL_KERNEL_CHANNELS, C))
    lib = _lib.lib()
    if m is None:
        m = torch.empty((C, (L + 3) // 4 * 4), dtype=torch.uint8, device=w.device)       # (rows on 4-byte boundaries: word stores)
    else:
        if not isinstance(m, torch.Tensor) or not m.is_cuda or m.dtype != torch.uint8 or m.dim() != 2 or m.shape[0] != C or m.shape[1] < L \
                or (m.shape[1] > 1 and m.stride(1) != 1):
            raise ValueError("speech_level_envelope: m must be a uint8 tensor [%d, >= %d] on the GPU with contiguous rows" % (C, L))
    ld_m = m.stride(0) if C > 1 else max(m.shape[1], 1)
    need = lib.p2phd_speechlevel_workspace_bytes(L, C)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=w.device)
    else:
        workspace = _lib.require_gpu_tensor(workspace, "speech_level_envelope: workspace", torch.uint8)
        if workspace.numel() < need:
            raise ValueError("speech_level_envelope: the workspace holds %d bytes, %d are needed" % (workspace.numel(), need))
    sq = torch.empty((C,), dtype=torch.float64, device=w.device)
    _lib.check(lib.p2phd_speechlevel_envelope(_lib.ptr(w), L, C, max(ld, L), rate, _lib.ptr(m), max(ld_m, L), _lib.ptr(sq), _lib.ptr(workspace),
                                              _lib.stream_ptr()), "speech_level_envelope")
    return m[:, :L], sq


def speech_level_counts(m, rate):
    """m [C, L] uint8 on the GPU (rows contiguous, any row pitch) -> a [C, 16] int64 on the GPU, nothing waited for: a[c][j] = the
    samples of row c at which the trailing maximum of m over the 200 ms hangover is over j (p2phd_speechlevel_counts); column 15
    is padding.  One launch of the family "speechlevel"; none for an empty clip."""
    rate = check_speech_level_rate(rate, "speech_level_counts")
    if not isinstance(m, torch.Tensor) or not m.is_cuda or m.dtype != torch.uint8:
        raise _lib.P2PHDError("speech_level_counts: m: expected a uint8 tensor on the GPU (this build has no CPU path)")
    if m.dim() != 2 or not 1 <= m.shape[0] <= SPEECH_LEVEL_KERNEL_CHANNELS:
        raise ValueError("speech_level_counts: expected m [C, L] with 1 <= C <= %d, got shape %s" % (SPEECH_LEVEL_KERNEL_CHANNELS, tuple(m.shape)))
    C, L = m.shape
    if L > 1 and m.stride(1) != 1 or C > 1 and m.stride(0) < L:
        raise _lib.P2PHDError("speech_level_counts: m: expected rows that are contiguous")
    a = torch.empty((C, 16), dtype=torch.int64, device=m.device)
    _lib.check(_lib.lib().p2phd_speechlevel_counts(_lib.ptr(m), L, C, max(m.stride(0) if C > 1 else L, L, 1), rate, _lib.ptr(a), _lib.stream_ptr()),
               "speech_level_counts")
    return a


def speech_level_packed_bytes(channels):
    """Bytes of the packed result of one speech_level_decide: res [(C + 1), 4] f64 | gain f32 | 4 spare bytes."""
    return (int(channels) + 1) * 32 + 8


def _speech_level_views(buf, channels):
    """The packed result of one speech_level_decide, on the device or its copy on the host -> (res [(C + 1), 4] f64, gain [1] f32)."""
    n = (int(channels) + 1) * 32
    return buf[:n].view(torch.float64).view(int(channels) + 1, 4), buf[n:n + 4].view(torch.float32)


def speech_level_decide(sq, a, frames, target=None, target_dev=None, max_gain_db=None, out=None):
    """sq [C] float64 and a [C, 16] int64 on the GPU -> (res, gain) on the GPU, nothing waited for: res [(C + 1), 4] float64, row c =
    {active speech level in dBov, long-term level, activity factor, the bracket's threshold}, row C = the file's figure {active,
    long-term, activity, the channel it is}; gain [1] f32 brings the file's figure to the wanted level, at most `max_gain_db`
    (None: 40) either way, 1 where no level is wanted or a level is not finite (p2phd_speechlevel_decide).  The wanted level:
    `target_dev`, a float64 tensor on the GPU whose first element the kernel reads (another clip's res[C]: no host round trip), else
    `target` (None: none).  `out`: None, or a uint8 tensor of speech_level_packed_bytes(C) on the GPU that takes both.  One
    launch of the family "speechlevel"."""
    sq = _lib.require_gpu_tensor(sq, "speech_level_decide: sq", torch.float64)
    a = _lib.require_gpu_tensor(a, "speech_level_decide: a", torch.int64)
    if sq.dim() != 1 or not 1 <= sq.shape[0] <= SPEECH_LEVEL_KERNEL_CHANNELS or tuple(a.shape) != (sq.shape[0], 16):
        raise ValueError("speech_level_decide: expected sq [C] and a [C, 16] with 1 <= C <= %d, got shapes %s and %s"
                         % (SPEECH_LEVEL_KERNEL_CHANNELS, tuple(sq.shape), tuple(a.shape)))
    C = sq.shape[0]
    if max_gain_db is None:
        max_gain_db = SPEECH_LEVEL_DEFAULTS['max_gain_db']
    if target_dev is not None:
        target_dev = _lib.require_gpu_tensor(target_dev, "speech_level_decide: target_dev", torch.float64)
        if target_dev.numel() < 1:
            raise ValueError("speech_level_decide: target_dev is empty")
    nbytes = speech_level_packed_bytes(C)
    if out is None:
        out = torch.empty((nbytes,), dtype=torch.uint8, device=sq.device)
    else:
        out = _lib.require_gpu_tensor(out, "speech_level_decide: out", torch.uint8)
        if out.numel() != nbytes:
            raise ValueError("speech_level_decide: out must hold %d bytes, got %d" % (nbytes, out.numel()))
    res, gain = _speech_level_views(out, C)
    _lib.check(_lib.lib().p2phd_speechlevel_decide(_lib.ptr(sq), _lib.ptr(a), int(frames), C, float('nan') if target is None else float(target),
                                                   _lib.ptr(target_dev), float(max_gain_db), _lib.ptr(res), _lib.ptr(gain), _lib.stream_ptr()),
               "speech_level_decide")
    return res, gain


def speech_level(clip, rate, target=None, target_dev=None, max_gain_db=None, out=None):
    """speech_level_envelope, speech_level_counts and speech_level_decide in a row: clip [C, L] f32 on the GPU -> (res, gain) on the
    GPU.  Three launches of the family "speechlevel" (none of the first two for an empty clip), nothing is waited for."""
    m, sq = speech_level_envelope(clip, rate)
    return speech_level_decide(sq, speech_level_counts(m, rate), clip.shape[1], target, target_dev, max_gain_db, out)
