"""The output stage of whole-file generation on the GPU (csrc/pcm.hip: p2phd_pcm_peak, p2phd_pcm_encode_ex; generate.py:
pcm_peaks, pcm_encode's new arguments, enhance_file's clip / ceiling_dbfs / dither / report_peaks): every figure and every
byte against the numpy restatement (tests/_outstage_ref.py), bit for bit."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _outstage_ref as O
import _pcm_ref as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENCODINGS = ("pcm16", "pcm24", "float32")
CODE = {"pcm16": 1, "pcm24": 2, "float32": 4}


def _specials():
    v = [1.0, -1.0, 0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 1.1754942e-38]
    for enc in ("pcm16", "pcm24"):
        hi = O.hi_of(enc)
        v += [hi, np.nextafter(hi, np.float32(2)), np.nextafter(hi, np.float32(0)), -hi]
    v += [np.nextafter(np.float32(-1), np.float32(-2)), np.nextafter(np.float32(-1), np.float32(0)),
          np.nextafter(np.float32(1), np.float32(2))]
    v += list(((np.arange(-6, 6) + 0.5) / 32768.0).astype(np.float32))          # k + 0.5 LSB: the dither decides
    return np.array(v, dtype=np.float32)


def _clip_values(frames, channels, seed=0):
    """planar float32 [channels, frames]: the special values first (interleaved order, so every channel gets some), random
    values inside and outside the range behind."""
    rng = np.random.default_rng(seed + 131 * frames + channels)
    n = frames * channels
    body = np.where(rng.random(n) < 0.9, rng.uniform(-1.0, 1.0, n), rng.standard_normal(n) * 1.5).astype(np.float32)
    sp = _specials()
    k = min(n, len(sp))
    body[:k] = sp[:k]
    return np.ascontiguousarray(body.reshape(frames, channels).T)


def _peaks(x, encoding, ceiling=None):
    from pix2pixhdaudiosr_amd.generate import pcm_peaks
    return [t.cpu().numpy() for t in pcm_peaks(x, encoding, ceiling)]


def _assert_peaks(got, want, what):
    peak, over, nonfinite, gain = got
    assert peak.dtype == np.float32 and over.dtype == np.int64 and nonfinite.dtype == np.int64 and gain.shape == (1,)
    assert peak.view(np.uint32).tolist() == want[0].view(np.uint32).tolist(), what
    assert over.tolist() == want[1].tolist() and nonfinite.tolist() == want[2].tolist(), what
    assert gain.view(np.uint32)[0] == np.float32(want[3]).view(np.uint32), (what, gain, want[3])


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------
# shapes: a piece tail, a workgroup tail, the odd-channel PCM24 byte phase
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [0, 1, 7, 255, 256, 257, 4099])
def test_shapes_against_the_restatement(frames):
    from pix2pixhdaudiosr_amd.generate import pcm_encode
    for channels in (1, 2, 3):
        x = _clip_values(frames, channels)
        dx = torch.from_numpy(x).to(DEV)
        gain = torch.tensor([0.625], device=DEV)
        for enc in ENCODINGS:
            _assert_peaks(_peaks(dx, enc), O.peaks(x, enc), (frames, channels, enc))
            assert _bytes(pcm_encode(dx, enc, gain=gain)) == O.encode_ex(x, enc, gain=0.625), (frames, channels, enc)
        for seed in (0, 2 ** 63 + 5):
            assert _bytes(pcm_encode(dx, "pcm16", dither='tpdf', seed=seed)) == O.encode_ex(x, "pcm16", tpdf=True, seed=seed)
        assert _bytes(pcm_encode(dx, "pcm16", gain=gain, dither='tpdf', seed=3, first_index=12345)) == \
            O.encode_ex(x, "pcm16", gain=0.625, tpdf=True, seed=3, first_index=12345)


def test_row_pitch_and_unaligned_rows():
    """ld = frames + 5 and a buffer that starts 0, 1 and 3 floats off a 16-byte boundary: rows that start anywhere."""
    from pix2pixhdaudiosr_amd.generate import pcm_encode
    frames, channels = 1001, 3
    ld = frames + 5
    x = _clip_values(frames, channels, seed=4)
    x[2, -1] = 9.5                                                # the peak sits in the last element of the last row
    big = torch.full((channels * ld + 3,), 1e30, device=DEV)      # (1e30 in the gaps: a read beyond a row would show as the peak)
    for off in (0, 1, 3):
        w = big[off:off + channels * ld].view(channels, ld)[:, :frames]
        w.copy_(torch.from_numpy(x))
        assert w.data_ptr() % 16 == (4 * off) % 16 and w.stride(0) == ld
        for enc in ENCODINGS:
            _assert_peaks(_peaks(w, enc), O.peaks(x, enc), (off, enc))
        assert _peaks(w, "pcm16")[0][2] == np.float32(9.5)
        g = torch.tensor([0.5], device=DEV)
        assert _bytes(pcm_encode(w, "pcm24", gain=g)) == O.encode_ex(x, "pcm24", gain=0.5)
        assert _bytes(pcm_encode(w, "pcm16", dither='tpdf', seed=1)) == O.encode_ex(x, "pcm16", tpdf=True, seed=1)


def test_many_workgroups_feed_the_fold():
    from pix2pixhdaudiosr_amd.generate import pcm_encode, pcm_peaks
    frames = 300001
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.9, 0.9, (2, frames)).astype(np.float32)
    x[0, -1] = -1.7                                               # the peak: last element of channel 0 ...
    x[1, 1000:250000:97] = 1.01                                   # ... the most clipped samples: channel 1
    x[1, 77777] = np.nan
    x[0, 123456] = -np.inf
    dx = torch.from_numpy(x).to(DEV)
    for enc in ENCODINGS:
        want = O.peaks(x, enc)
        _assert_peaks(_peaks(dx, enc), want, enc)
        assert want[0].tolist() == [np.float32(1.7), np.float32(1.01)] and want[1][1] > want[1][0] == 2 and want[2].tolist() == [1, 1]
    a = pcm_peaks(dx, "pcm16", 0.5)                               # repeatability: the same bits on every run
    for _ in range(3):
        b = pcm_peaks(dx, "pcm16", 0.5)
        assert all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b))
    gain = pcm_peaks(dx, "pcm16")[3]
    assert _bytes(pcm_encode(dx, "pcm16", gain=gain, dither='tpdf', seed=2 ** 63 + 5)) == \
        O.encode_ex(x, "pcm16", gain=O.peaks(x, "pcm16")[3], tpdf=True, seed=2 ** 63 + 5)


def test_special_rows():
    x = _clip_values(64, 3, seed=2)
    x[1, :] = np.nan                                              # a row without a finite sample: peak 0
    x[2, :] = np.where(np.isfinite(x[2]), x[2], 0) * 0.25
    x[0, 5] = np.inf
    dx = torch.from_numpy(x).to(DEV)
    for enc in ENCODINGS:
        got, want = _peaks(dx, enc), O.peaks(x, enc)
        _assert_peaks(got, want, enc)
        assert got[0][1] == 0.0 and got[2][1] == 64 and got[1][1] == 0 and got[2][2] == 0
    # outputs need no memset: a buffer of garbage is overwritten, frames = 0 included
    from pix2pixhdaudiosr_amd.generate import pcm_peaks
    p = pcm_peaks(torch.zeros((2, 0), device=DEV), "pcm24")
    assert p[0].tolist() == [0.0, 0.0] and p[1].tolist() == [0, 0] and p[2].tolist() == [0, 0] and p[3].tolist() == [1.0]


# ------------------------------------------------------------------------------------------
# the C ABI: _ex without gain and dither is the old encoder; argument errors
# ------------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw_encode_ex(lib, x, code, nbytes, gain=None, dither=0, seed=0, first=0):
    from pix2pixhdaudiosr_amd import _lib as L
    C, n = x.shape
    out = torch.zeros(C * n * nbytes, dtype=torch.uint8, device=DEV)
    rc = lib.p2phd_pcm_encode_ex(L.ptr(x), n, C, x.stride(0) if C > 1 else n, code, L.ptr(gain), dither, seed, first, L.ptr(out), _stream())
    return rc, out


@pytest.mark.parametrize("encoding", ENCODINGS)
def test_ex_without_gain_and_dither_is_the_old_encoder(encoding):
    from pix2pixhdaudiosr_amd import _lib as L
    from pix2pixhdaudiosr_amd.generate import PCM_ENCODINGS, pcm_encode
    code, nbytes = PCM_ENCODINGS[encoding]
    f32 = np.frombuffer(P.payload("f32", 200, 3), dtype="<f4").reshape(200, 3).T       # NaNs with payloads, denormals, +-inf
    for x in (np.ascontiguousarray(f32), P.encode_input(777, 2), _clip_values(515, 3)):
        dx = torch.from_numpy(x).to(DEV)
        old = pcm_encode(dx, encoding)
        rc, new = _raw_encode_ex(L.lib(), dx, code, nbytes)
        assert rc == 0 and torch.equal(old, new)
        assert _bytes(new) == P.encode(x, encoding) or encoding == "float32"
        if encoding == "float32":
            assert np.array_equal(new.cpu().numpy().view("<u4"), np.ascontiguousarray(x.T).view("<u4").ravel())


def test_argument_errors():
    from pix2pixhdaudiosr_amd import _lib as L
    from pix2pixhdaudiosr_amd.generate import pcm_encode, pcm_peaks
    lib = L.lib()
    x = torch.zeros((2, 8), device=DEV)
    for code in (2, 4):                                           # dither is for PCM16
        rc, _ = _raw_encode_ex(lib, x, code, 4, dither=1)
        assert rc != 0 and b"dither" in lib.p2phd_last_error()
    assert _raw_encode_ex(lib, x, 1, 2, dither=2)[0] != 0 and _raw_encode_ex(lib, x, 0, 2)[0] != 0
    assert _raw_encode_ex(lib, x, 1, 2, dither=1, first=-1)[0] != 0
    out = torch.zeros(64, dtype=torch.uint8, device=DEV)
    peak, over, nonf, gain = out[:8].view(torch.float32), out[8:24].view(torch.int64), out[24:40].view(torch.int64), out[40:44].view(torch.float32)
    args = lambda fmt, ld: (L.ptr(x), 8, 2, ld, fmt, 0.0, L.ptr(peak), L.ptr(over), L.ptr(nonf), L.ptr(gain), _stream())
    assert lib.p2phd_pcm_peak(*args(1, 8)) == 0
    assert lib.p2phd_pcm_peak(*args(3, 8)) != 0 and b"format" in lib.p2phd_last_error()
    assert lib.p2phd_pcm_peak(*args(1, 7)) != 0 and b"ld" in lib.p2phd_last_error()
    assert lib.p2phd_pcm_peak(L.ptr(x), 8, 2, 8, 1, 0.0, None, L.ptr(over), L.ptr(nonf), L.ptr(gain), _stream()) != 0
    with pytest.raises(ValueError, match="pcm16"):
        pcm_encode(x, "pcm24", dither='tpdf')
    with pytest.raises(ValueError, match="dither"):
        pcm_encode(x, "pcm16", dither='rect')
    with pytest.raises(ValueError, match="gain"):
        pcm_encode(x, "pcm16", gain=torch.ones(2, device=DEV))
    with pytest.raises(L.P2PHDError):
        pcm_encode(x, "pcm16", gain=torch.ones(1))
    with pytest.raises(ValueError, match="ceiling"):
        pcm_peaks(x, "pcm16", -0.5)
    with pytest.raises(ValueError, match="encoding"):
        pcm_peaks(x, "pcm8")
    with pytest.raises(L.P2PHDError):
        pcm_peaks(x.cpu(), "pcm16")


def test_launch_family_counts_the_new_entries():
    from pix2pixhdaudiosr_amd import _lib as L
    from pix2pixhdaudiosr_amd.generate import pcm_encode, pcm_peaks
    lib = L.lib()
    x = torch.zeros((2, 16), device=DEV)
    lib.p2phd_launch_count(b"pcm", 1)
    g = pcm_peaks(x, "pcm16")[3]
    assert lib.p2phd_launch_count(b"pcm", 0) == 1
    pcm_encode(x, "pcm16", gain=g)
    assert lib.p2phd_launch_count(b"pcm", 1) == 2


# ------------------------------------------------------------------------------------------
# dither: the index carries into the high word; pieces are the whole
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5])
def test_dither_index_and_pieces(seed):
    from pix2pixhdaudiosr_amd.generate import pcm_encode
    frames, channels = 256, 2
    first = 2 ** 32 - 100                                         # sample 100 of the payload has index 2^32
    x = _clip_values(frames, channels, seed=6) * np.float32(0.01)
    x[:, 64:128] = ((np.arange(128).reshape(64, 2).T - 64 + 0.5) / 32768.0).astype(np.float32)      # ties
    x = np.where(np.isfinite(x), x, np.float32(0)).astype(np.float32)
    dx = torch.from_numpy(x).to(DEV)
    whole = _bytes(pcm_encode(dx, "pcm16", dither='tpdf', seed=seed, first_index=first))
    assert whole == O.encode_ex(x, "pcm16", tpdf=True, seed=seed, first_index=first)
    cut = 37
    parts = _bytes(pcm_encode(dx[:, :cut], "pcm16", dither='tpdf', seed=seed, first_index=first)) + \
        _bytes(pcm_encode(dx[:, cut:], "pcm16", dither='tpdf', seed=seed, first_index=first + cut * channels))
    assert parts == whole
    plain = np.frombuffer(_bytes(pcm_encode(dx, "pcm16")), dtype="<i2").astype(int)
    dith = np.frombuffer(whole, dtype="<i2").astype(int)
    assert np.abs(dith - plain).max() == 1 and np.count_nonzero(dith != plain) > 50
    assert whole != _bytes(pcm_encode(dx, "pcm16", dither='tpdf', seed=seed + 1, first_index=first))


# ------------------------------------------------------------------------------------------
# guard
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ceiling_dbfs", [None, -1.0])
def test_guard(ceiling_dbfs):
    from pix2pixhdaudiosr_amd.generate import ceiling_from_dbfs, pcm_encode, pcm_peaks
    frames = 5000
    t = np.arange(frames) / 48000.0
    x = np.stack([1.7 * np.sin(2 * np.pi * 440 * t + 0.3), 0.8 * np.sin(2 * np.pi * 1000 * t), 1.2 * np.cos(2 * np.pi * 50 * t)]).astype(np.float32)
    x[0, 1234] = 1.7                                              # the clip peaks at 1.7, in channel 0
    assert np.abs(x).max() == np.float32(1.7)
    dx = torch.from_numpy(x).to(DEV)
    for enc in ENCODINGS:
        ceiling = ceiling_from_dbfs(ceiling_dbfs, enc)
        level = np.float32(ceiling) if ceiling is not None else O.hi_of(enc)
        want = O.peaks(x, enc, 0.0 if ceiling is None else ceiling)
        peak, over, nonfinite, gain = pcm_peaks(dx, enc, ceiling)
        _assert_peaks([v.cpu().numpy() for v in (peak, over, nonfinite, gain)], want, (enc, ceiling_dbfs))
        assert want[3] == level / np.float32(1.7) and want[1][0] > 100 and want[1][1] == 0 and want[1][2] > 100      # counted on the unscaled clip
        data = _bytes(pcm_encode(dx, enc, gain=gain))             # the kernel reads the gain from the device
        assert data == O.encode_ex(x, enc, gain=want[3])
        if enc == "float32":
            y = np.frombuffer(data, dtype="<f4").reshape(frames, 3)
            assert np.abs(y).max() <= level and np.array_equal(y, (x * want[3]).T)      # one gain for every channel
        else:
            scale = 2 ** (O.BITS[enc] - 1)
            raw = np.frombuffer(data, dtype=np.uint8).reshape(-1, O.BITS[enc] // 8).astype(np.int64)
            q = sum(raw[:, b] << (8 * b) for b in range(raw.shape[1]))
            q = np.where(q >= scale, q - 2 * scale, q)
            assert np.abs(q).max() <= round(float(level) * scale)
            assert np.abs(q).max() >= round(float(level) * scale) - 2             # and the peak does sit at the ceiling (two fp32 roundings)
        # a clip that fits is left alone
        quiet = pcm_peaks(dx * 0.25, enc, ceiling)
        assert quiet[3].item() == 1.0 and quiet[1].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------
# the fp16 library holds the same two entries
# ------------------------------------------------------------------------------------------
def test_fp16_library():
    from pix2pixhdaudiosr_amd import _lib as L
    lib = L.lib("f16")
    assert lib.p2phd_half_type() == 2 and hasattr(lib, "p2phd_pcm_peak") and hasattr(lib, "p2phd_pcm_encode_ex")
    x = _clip_values(333, 2, seed=9)
    dx = torch.from_numpy(x).to(DEV)
    buf = torch.full((44,), 255, dtype=torch.uint8, device=DEV)
    over, nonf, peak, gain = buf[:16].view(torch.int64), buf[16:32].view(torch.int64), buf[32:40].view(torch.float32), buf[40:].view(torch.float32)
    L.check(lib.p2phd_pcm_peak(L.ptr(dx), 333, 2, 333, 1, 0.5, L.ptr(peak), L.ptr(over), L.ptr(nonf), L.ptr(gain), _stream()), "pcm_peak")
    want = O.peaks(x, "pcm16", 0.5)
    _assert_peaks([v.cpu().numpy() for v in (peak, over, nonf, gain)], want, "f16 library")
    rc, out = _raw_encode_ex(lib, dx, 1, 2, gain=gain, dither=1, seed=77, first=5)
    assert rc == 0 and _bytes(out) == O.encode_ex(x, "pcm16", gain=want[3], tpdf=True, seed=77, first_index=5)


# ------------------------------------------------------------------------------------------
# end to end: files
# ------------------------------------------------------------------------------------------
def test_enhance_file_output_stage(tmp_path):
    from test_gpu_generate import PassThrough, _clip, _tiny
    from test_gpu_generate_multi import _data
    from pix2pixhdaudiosr_amd import _lib as L
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    real, opt = _tiny("mdct4", lr_sampling_rate=12000)            # up_ratio 4: the pipeline writes sqrt(3) * x
    sr = SuperResolver(PassThrough(real), opt)
    n = 3 * opt.segment_length + 211
    a, b = _clip(n, 0), _clip(n, 6000)
    clip = torch.stack([a / a.abs().max(), -0.3 * b / b.abs().max()])           # a normalised input
    src = str(tmp_path / "in.wav")
    wavio.save(src, clip, 48000, encoding="float32")
    lib = L.lib()

    # the default call: the file as before, no 'output'
    plain = str(tmp_path / "plain.wav")
    res = sr.enhance_file(src, plain, channels='all')
    assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'sr']
    x = res['sr'].cpu().numpy()
    assert _data(plain)[0] == P.encode(x, "pcm16")
    want = O.peaks(x, "pcm16")
    assert 1.0 < want[0][0] < 1.9 and want[1][0] > 0 and want[1][1] == 0         # ... and it is hard-clipped in channel 0

    # guard + dither + report
    out = str(tmp_path / "guard.wav")
    lib.p2phd_launch_count(b"pcm", 1)
    res2 = sr.enhance_file(src, out, channels='all', clip='guard', dither='tpdf', dither_seed=5, report_peaks=True)
    assert lib.p2phd_launch_count(b"pcm", 1) == 3                 # decode, peak, encode
    assert torch.equal(res2['sr'], res['sr']) and res2['metrics'] == res['metrics']          # only the written bytes change
    data, meta = _data(out)
    assert (meta.num_channels, meta.num_frames, meta.bits_per_sample) == (2, n, 16)
    assert data == O.encode_ex(x, "pcm16", gain=want[3], tpdf=True, seed=5)
    o = res2['output']
    assert sorted(o) == ['clipped', 'gain', 'nonfinite', 'peak', 'peak_dbfs']
    assert o['peak'] == [float(v) for v in want[0]] and o['clipped'] == want[1].tolist() and o['nonfinite'] == [0, 0]
    assert o['gain'] == float(want[3]) and o['peak_dbfs'] == [20.0 * math.log10(float(v)) for v in want[0]]
    assert data != P.encode(x, "pcm16") and want[3] < 1.0

    # a ceiling, another encoding; report only (clamp) leaves the bytes alone and reports gain 1
    out24 = str(tmp_path / "g24.wav")
    res3 = sr.enhance_file(src, out24, channels='all', encoding='pcm24', clip='guard', ceiling_dbfs=-1.0)
    c = np.float32(10.0 ** (-1.0 / 20.0))
    assert _data(out24)[0] == O.encode_ex(x, "pcm24", gain=O.peaks(x, "pcm24", c)[3]) and res3['output']['gain'] == float(c / want[0][0])
    rep = str(tmp_path / "rep.wav")
    res4 = sr.enhance_file(src, rep, channels='all', report_peaks=True)
    assert _data(rep)[0] == _data(plain)[0] and res4['output']['gain'] == 1.0 and res4['output']['clipped'] == want[1].tolist()

    # error: raises, names the file, leaves nothing on disk
    bad = str(tmp_path / "sub" / "bad.wav")
    with pytest.raises(ValueError, match=r"bad\.wav.*%d samples.*dBFS" % int(want[1].sum())):
        sr.enhance_file(src, bad, channels='all', clip='error')
    assert not os.path.exists(bad) and not os.path.exists(os.path.dirname(bad))
    ok = str(tmp_path / "ok.wav")                                 # float32 holds the sample; |x| > 1 still counts as clipped there
    with pytest.raises(ValueError, match="would clip"):
        sr.enhance_file(src, ok, channels='all', encoding='float32', clip='error')
    quiet = str(tmp_path / "quiet.wav")
    wavio.save(quiet, 0.25 * clip, 48000, encoding="float32")
    r5 = sr.enhance_file(quiet, ok, channels='all', clip='error')
    assert os.path.exists(ok) and r5['output']['clipped'] == [0, 0] and _data(ok)[0] == P.encode(r5['sr'].cpu().numpy(), "pcm16")
    # before any GPU work
    lib.p2phd_launch_count(None, 1)
    with pytest.raises(ValueError, match="pcm16"):
        sr.enhance_file(src, ok, encoding='pcm24', dither='tpdf')
    assert lib.p2phd_launch_count(b"pcm", 0) == 0 and lib.p2phd_launch_count(b"stitch", 0) == 0

    # a folder: file k is dithered with seed + k; a record carries 'output'
    folder = tmp_path / "many"
    folder.mkdir()
    for name in ("a.wav", "b.wav"):
        wavio.save(str(folder / name), 0.5 * clip[:, :opt.segment_length + 9], 48000, encoding="float32")
    recs = sr.enhance_folder(str(folder), str(tmp_path / "many_out"), channels='all', dither='tpdf', dither_seed=40)
    assert [r['path'] for r in recs] == ["a.wav", "b.wav"] and all(r['output']['gain'] == 1.0 for r in recs)
    one = sr.enhance_file(str(folder / "b.wav"), None, channels='all')['sr'].cpu().numpy()
    assert _data(str(tmp_path / "many_out" / "a.wav"))[0] == O.encode_ex(one, "pcm16", tpdf=True, seed=40)
    assert _data(str(tmp_path / "many_out" / "b.wav"))[0] == O.encode_ex(one, "pcm16", tpdf=True, seed=41)
