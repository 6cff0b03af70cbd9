"""The grid-stride kernels PAST their workgroup cap, per element, through the C ABI: every case of tests/_long.py is about 2.5
trips of the capped grid plus an odd remainder.  Each test first asks p2phd_stream_grid (pinned on the host by
tests/test_long_host.py) and asserts used < wanted and work > 2 * unit_work, so a changed cap fails here instead of quietly
running one trip.  Outputs sit between 4 KiB canaries, prefilled with the sentinel; inputs are a hash of the index (tests/_long.py);
every element is compared, and a failure names the first differing index, that index modulo unit_work and the count."""
import ctypes

import numpy as np
import pytest
import torch

import _companions as C
import _exact as E
import _long as K
import _outstage_ref as O
import _pcm_ref as P
import _stereo_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT32 = 0xA5A5A5A5                                                  # a payload prefilled with E.GUARD_BYTE, read as uint32


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _past_the_cap(cid, lib=None):
    """(work, unit_work) of the case, after asserting that its launch loops and that some thread takes a third trip."""
    cid, family, dtype, rows, _ = next(c for c in K.CASES if c[0] == cid)
    work = K.case_work(cid)
    rc, unit, wanted, used = K.stream_grid(lib or _lib().lib(), family, dtype, work, rows)
    assert rc == 0 and used < wanted and work > 2 * unit, (cid, work, unit, wanted, used)
    return work, unit


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _out(nbytes):
    g = E.Guarded(nbytes, DEV, E.GUARD_BYTE)
    return g


def _host(g, dtype):
    torch.cuda.synchronize()
    assert not g.touched(), f"writes outside the output at byte offsets {g.touched()}"
    return g.bytes.cpu().numpy().view(dtype)


def _same(got, want, unit, what):
    msg = K.first_difference(got, want, unit)
    assert msg is None, f"{what}: {msg}"


def _vp(p):
    return ctypes.c_void_p(int(p))


# ------------------------------------------------------------------------------------------
# gather, stitch
# ------------------------------------------------------------------------------------------
def test_gather_planar_vec4():
    """Two rows with a pitch larger than the row, T and stride multiples of 4 (the 16-byte path), overlapping segments, the last
    segments beyond the end of the audio (zeros)."""
    L = _lib()
    work, unit = _past_the_cap("gather_vec_planar")
    T, stride, Sg = K.GATHER_VEC["T"], K.GATHER_VEC["stride"], K.GATHER_VEC["S"]
    Lin = (Sg - 2) * stride + T // 2 + 3                             # the last two segments are partly / wholly zeros
    ld = (Lin + 8) // 4 * 4
    audio = K.hashed_floats(2 * ld, seed=11).reshape(2, ld)
    g = _out(2 * Sg * T * 4)
    audio_d = _dev(audio)
    L.check(L.lib().p2phd_segments_gather_planar(L.ptr(audio_d), 2, ld, Lin, T, stride, Sg, _vp(g.ptr()), L.stream_ptr()), "gather_planar")
    got = _host(g, np.uint32).reshape(2, Sg * T)
    for r in range(2):
        _same(got[r], K.gather_vec(audio[r, :Lin], T, stride, Sg).view(np.uint32).reshape(-1), unit, f"gather_planar row {r}")


def test_gather_scalar_path():
    """Odd T = stride: the element-by-element path, single row."""
    L = _lib()
    work, unit = _past_the_cap("gather_scalar")
    T, Sg = K.GATHER_SCALAR["T"], K.GATHER_SCALAR["S"]
    Lin = Sg * T - 1234
    audio = K.hashed_floats(Lin, seed=12)
    g = _out(Sg * T * 4)
    audio_d = _dev(audio)
    L.check(L.lib().p2phd_segments_gather(L.ptr(audio_d), Lin, T, T, Sg, _vp(g.ptr()), L.stream_ptr()), "gather")
    _same(_host(g, np.uint32), K.gather_vec(audio, T, T, Sg).view(np.uint32).reshape(-1), unit, "gather scalar")


def _stitch(cid, T, stride, gain, shift):
    L = _lib()
    L_out, unit = _past_the_cap(cid)
    V = T - stride
    Sg = K.cdiv(L_out - V, stride)
    assert L_out <= (Sg - 1) * stride + T and L_out % 4 != 0
    seg = K.hashed_floats(Sg * T, seed=13 + shift).reshape(Sg, T)
    seg_d = torch.empty(Sg * T + 4, dtype=torch.float32, device=DEV)    # shift = 1: both bases one float in (the scalar path)
    seg_d[shift:shift + Sg * T] = _dev(seg.reshape(-1))
    g = _out((L_out + shift) * 4)
    L.check(L.lib().p2phd_segments_stitch(_vp(seg_d.data_ptr() + 4 * shift), Sg, T, stride, gain, _vp(g.ptr() + 4 * shift), L_out, L.stream_ptr()), cid)
    got = _host(g, np.uint32)
    assert (got[:shift] == SENT32).all()
    _same(got[shift:], K.stitch_vec(seg, stride, gain, L_out).view(np.uint32), unit, cid)


def test_stitch_cross_fade_vec4():
    """V > 0 on aligned bases: plain float4 runs, quads that straddle an overlap or a segment seam, the incomplete last quad."""
    _stitch("stitch_fade_vec", 4096, 3072, 0.75, 0)


def test_stitch_concatenation_scalar_path():
    """V = 0 (the reference's torch.cat times gain), both bases one float in."""
    _stitch("stitch_cat_scalar", 4099, 4099, 0.5, 1)


def test_stitch_planar_two_rows():
    """Two rows with a pitch larger than the row on both sides (seg rows S * T apart, out rows ld apart), V > 0, the 16-byte path."""
    L = _lib()
    L_out, unit = _past_the_cap("stitch_planar")
    T, stride = 4096, 3072
    V = T - stride
    Sg = K.cdiv(L_out - V, stride) + 1                                # one segment more than the output needs: L_out ends inside the span
    ld = (L_out + 12) // 4 * 4
    assert L_out <= (Sg - 1) * stride + T and L_out % 4 != 0 and ld > L_out
    seg = K.hashed_floats(2 * Sg * T, seed=17).reshape(2, Sg, T)
    g = _out(2 * ld * 4)
    seg_d = _dev(seg)
    L.check(L.lib().p2phd_segments_stitch_planar(L.ptr(seg_d), 2, Sg, T, stride, 1.25, _vp(g.ptr()), ld, L_out, L.stream_ptr()), "stitch_planar")
    got = _host(g, np.uint32).reshape(2, ld)
    assert (got[:, L_out:] == SENT32).all()                           # the rest of a row is not written
    for r in range(2):
        _same(got[r, :L_out], K.stitch_vec(seg[r], stride, 1.25, L_out).view(np.uint32), unit, f"stitch_planar row {r}")


# ------------------------------------------------------------------------------------------
# PCM codec
# ------------------------------------------------------------------------------------------
def _payload(name, n):
    bits = P.FORMATS[name][1]
    if name == "f64":                                                 # values that need the rounding to float32; no NaN (its payload bits are not pinned)
        return (K.hashed_floats(n, seed=21).astype("<f8") * (1.0 + 2.0 ** -30)).tobytes()
    if name == "f32":
        return K.hashed_floats(n, seed=22).astype("<f4").tobytes()
    return K.index_hash(K.cdiv(n * bits, 32), seed=23).astype("<u4").tobytes()[:n * bits // 8]


@pytest.mark.parametrize("name", list(P.FORMATS))
def test_pcm_decode(name):
    L = _lib()
    work, unit = _past_the_cap("pcm_decode")
    frames, ch = K.PCM_FRAMES, K.PCM_CHANNELS
    code = P.FORMATS[name][2]
    pay = _payload(name, work)
    ld = frames + 3
    g = _out(ch * ld * 4)
    src = torch.frombuffer(bytearray(pay), dtype=torch.uint8).to(DEV)
    L.check(L.lib().p2phd_pcm_decode(L.ptr(src), frames, ch, code, _vp(g.ptr()), ld, L.stream_ptr()), "pcm_decode")
    got = _host(g, np.uint32).reshape(ch, ld)
    assert (got[:, frames:] == SENT32).all()                          # the rest of a row is not written
    want = P.decode(pay, ch, name).view(np.uint32)
    # the interleaved order is the kernel's work order: compare there, so that the index reads as a position of the walk
    _same(np.ascontiguousarray(got[:, :frames].T), np.ascontiguousarray(want.T), unit, f"pcm_decode {name}")


def _planar(frames, ch, ld, seed):
    x = np.full((ch, ld), np.nan, dtype=np.float32)
    x[:, :frames] = (K.hashed_floats(frames * ch, seed=seed) * np.float32(1.25)).reshape(ch, frames)     # a fifth clamps
    return x


@pytest.mark.parametrize("mode", ["pcm16", "pcm24", "float32", "pcm24_gain", "float32_gain", "pcm16_tpdf"])
def test_pcm_encode(mode):
    """The plain encoder for the three formats; encode_ex with a gain; encode_ex with TPDF dither whose sample index crosses 2^32
    inside the second trip."""
    L = _lib()
    plain = "_" not in mode
    work, unit = _past_the_cap("pcm_encode" if plain else "pcm_encode_ex")
    frames, ch = K.PCM_FRAMES, K.PCM_CHANNELS
    encoding = mode.split("_")[0]
    bits, code = P.ENCODINGS[encoding][1:]
    ld = frames + 5
    x = _planar(frames, ch, ld, 31)
    nbytes = work * bits // 8
    g = _out(nbytes)
    if plain:
        x_d = _dev(x)
        L.check(L.lib().p2phd_pcm_encode(L.ptr(x_d), frames, ch, ld, code, _vp(g.ptr()), L.stream_ptr()), mode)
        want = P.encode(x[:, :frames], encoding)
    else:
        tpdf = mode.endswith("tpdf")
        gain = None if tpdf else np.float32(0.8125)
        first = (1 << 32) - (unit + unit // 2) if tpdf else 0        # first + e passes 2^32 in the middle of the second trip
        gain_d = None if gain is None else _dev(np.array([gain], dtype=np.float32))
        x_d = _dev(x)
        L.check(L.lib().p2phd_pcm_encode_ex(L.ptr(x_d), frames, ch, ld, code, L.ptr(gain_d), int(tpdf), 0x1234567890ABCDEF, first,
                                            _vp(g.ptr()), L.stream_ptr()), mode)
        want = O.encode_ex(x[:, :frames], encoding, gain=gain, tpdf=tpdf, seed=0x1234567890ABCDEF, first_index=first)
    got = _host(g, np.uint8)
    sample = bits // 8
    _same(got.reshape(-1, sample), np.frombuffer(want, dtype=np.uint8).reshape(-1, sample), unit * sample, mode)


def test_pcm_peak_second_round():
    """8 rows at a pitch of 1 mod 4 (rows start at every float alignment).  The row maximum, an over-range sample, a NaN and an inf lie
    only in pieces that the second round of four pieces in flight reads; another set in the scalar tail; and the largest value of
    the row in the last piece -- the one a clamped re-read fetches again: counted twice it shows in `over`."""
    L = _lib()
    frames, unit = _past_the_cap("pcm_peak_c8")
    ch, ld = 8, frames + 6
    assert ld % 4 == 1                                                # row r starts r floats past a 16-byte boundary
    x = np.full((ch, ld), np.nan, dtype=np.float32)
    x[:, :frames] = (K.hashed_floats(frames * ch, seed=41) * np.float32(0.5)).reshape(ch, frames)
    gx = K.expected_grid("pcm_peak", 0, frames, ch)[2]
    for r in range(ch):
        head = (-r * ld) % 4                                          # floats in front of the row's first 16-byte boundary
        pieces = (frames - head) // 4
        tail0 = head + 4 * pieces
        second = head + 4 * (4 * gx * 256 + 1000 * r + 7)             # a piece of the second round
        assert 4 * gx * 256 < pieces - 1 and second + 16 < head + 4 * (pieces - 1)
        x[r, second:second + 4] = [0.9375, 1.5, np.nan, np.inf] if r % 2 else [-0.9375, -1.5, -np.nan, -np.inf]
        x[r, head + 4 * (pieces - 1)] = 3.0 + r                       # the clamped re-read's piece
        x[r, tail0:frames] = [2.0, np.nan, -np.inf][:frames - tail0]
    assert {(frames - (-r * ld) % 4) % 4 for r in range(ch)} == {0, 1, 2, 3}      # every length of the scalar tail occurs
    res = {k: E.guarded_like((n,), dt, DEV, sentinel=s) for k, n, dt, s in (("peak", ch, torch.float32, 0.7), ("over", ch, torch.int64, -7),
                                                                              ("nonfinite", ch, torch.int64, -7), ("gain", 1, torch.float32, 0.7))}
    for encoding in ("pcm16", "float32"):
        code = P.ENCODINGS[encoding][2]
        x_d = _dev(x)
        L.check(L.lib().p2phd_pcm_peak(L.ptr(x_d), frames, ch, ld, code, 0.0, L.ptr(res["peak"][1]), L.ptr(res["over"][1]),
                                       L.ptr(res["nonfinite"][1]), L.ptr(res["gain"][1]), L.stream_ptr()), "pcm_peak")
        torch.cuda.synchronize()
        E.check_guards({k: v[0] for k, v in res.items()}, "pcm_peak")
        peak, over, nonfinite, gain = O.peaks(x[:, :frames], encoding)
        assert res["peak"][1].cpu().numpy().view(np.uint32).tolist() == peak.view(np.uint32).tolist(), encoding
        assert res["over"][1].cpu().tolist() == over.tolist(), encoding
        assert res["nonfinite"][1].cpu().tolist() == nonfinite.tolist(), encoding
        assert res["gain"][1].cpu().numpy().view(np.uint32).tolist() == [int(np.float32(gain).view(np.uint32))], encoding


# ------------------------------------------------------------------------------------------
# mid/side matrix
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,guard", [("stereo_vec", 0), ("stereo_vec", 1), ("stereo_scalar", 1), ("stereo_scalar", 0)])
def test_stereo_matrix(cid, guard):
    """Aligned pitches (float4 body and scalar tail) and odd pitches (the scalar path), with and without the side guard; the side
    row holds NaN and inf in every trip."""
    L = _lib()
    Ln, unit = _past_the_cap(cid)
    ld, ld_out = ((Ln + 8) // 4 * 4, (Ln + 12) // 4 * 4) if cid == "stereo_vec" else (Ln + 4, Ln + 6)
    assert (ld % 4 == 0 and ld_out % 4 == 0) == (cid == "stereo_vec")
    x = np.full((2, ld), np.nan, dtype=np.float32)
    x[:, :Ln] = K.hashed_floats(2 * Ln, seed=51).reshape(2, Ln)
    x[1, 5:Ln:100003] = np.inf
    x[1, 6:Ln:100019] = np.nan
    g = _out(2 * ld_out * 4)
    x_d = _dev(x)
    L.check(L.lib().p2phd_stereo_matrix(L.ptr(x_d), ld, Ln, 0.5, guard, _vp(g.ptr()), ld_out, L.stream_ptr()), cid)
    got = _host(g, np.uint32).reshape(2, ld_out)
    assert (got[:, Ln:] == SENT32).all()
    want = S.matrix_ref(x[:, :Ln], 0.5, bool(guard))
    nan = np.isnan(want)                                              # a NaN result: NaN on both sides, its payload is not pinned
    got_f = got[:, :Ln].view(np.float32)
    assert np.array_equal(np.isnan(got_f), nan)
    for r in range(2):
        _same(np.where(nan[r], 0, got[r, :Ln]), np.where(nan[r], 0, want[r].view(np.uint32)), unit, f"{cid} guard {guard} row {r}")


# ------------------------------------------------------------------------------------------
# activation backward, Adam
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_act_bwd(dt):
    """LeakyReLU / ReLU backward from the saved output on small-integer operands: one multiply, one rounding -- bit for bit."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(C.DT[dt])
    code = 0 if dt == "f32" else 1
    n, unit = _past_the_cap("act_bwd_f32" if dt == "f32" else "act_bwd_h16", Lb)
    g = torch.from_numpy(K.hashed_small_ints(n, seed=61)).to(C.DT[dt])
    a = torch.from_numpy(K.hashed_small_ints(n, seed=62)).to(C.DT[dt])
    gd, ad = g.to(DEV), a.to(DEV)
    for act in (C.LRELU, C.RELU):
        go, out = E.guarded_like((n,), C.DT[dt], DEV, sentinel=C.SENTINEL)
        ops.check(Lb.p2phd_act_bwd(code, ops.ptr(gd), ops.ptr(ad), ops.ptr(out), n, act, ops.stream_ptr()), "act_bwd")
        torch.cuda.synchronize()
        E.check_guards({"dx": go}, "act_bwd")
        want, bound = C.act_bwd_reference(g, a, act, C.DT[dt])
        assert bound is None
        bits = {2: torch.int16, 4: torch.int32}[out.element_size()]
        _same(out.cpu().view(bits).numpy(), want.to(C.DT[dt]).view(bits).numpy(), unit, f"act_bwd {dt} act {act}")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_layout_kernels(dt):
    """nchw_to_nhwc (an element per thread) and nhwc_to_nchw (a 16-byte piece per thread) with Cp > C and a channel offset, on
    small-integer operands: bit for bit; the channels outside [ch_off, ch_off + C) and the rest of the pitch are not written."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(C.DT[dt])
    code, Cp = (0, 8) if dt == "f32" else (1, 16)
    Cc, off = K.LAYOUT_C, 2
    bits = {2: torch.int16, 4: torch.int32}[torch.empty((), dtype=C.DT[dt]).element_size()]
    # f32 [1, C, HW] -> [1, HW, Cp]
    work, unit = _past_the_cap("nchw_to_nhwc", Lb)
    HW = K.TO_NHWC_HW
    src = K.hashed_small_ints(Cc * HW, seed=65).reshape(Cc, HW)
    go, out = E.guarded_like((HW, Cp), C.DT[dt], DEV, sentinel=C.SENTINEL)
    src_d = _dev(src)
    ops.check(Lb.p2phd_nchw_to_nhwc(code, ops.ptr(src_d), ops.ptr(out), 1, Cc, HW, Cp, off, ops.stream_ptr()), "nchw_to_nhwc")
    torch.cuda.synchronize()
    E.check_guards({"dst": go}, "nchw_to_nhwc")
    want = torch.full((HW, Cp), C.SENTINEL, dtype=C.DT[dt])
    want[:, off:off + Cc] = torch.from_numpy(np.ascontiguousarray(src.T)).to(C.DT[dt])
    got = out.cpu()
    # the kernel's work order is [C, HW]: compare there, so that the index reads as a position of the walk
    _same(got[:, off:off + Cc].T.contiguous().view(bits).numpy(), want[:, off:off + Cc].T.contiguous().view(bits).numpy(), unit, f"nchw_to_nhwc {dt}")
    _same(got.view(bits).numpy(), want.view(bits).numpy(), unit * Cp, f"nchw_to_nhwc {dt}: whole pitch")
    # [1, HW, Cp] -> f32 [1, C, HW]: HW * Cp / epp = 2 HW pieces
    work, unit = _past_the_cap("nhwc_to_nchw", Lb)
    HW = K.TO_NCHW_HW
    assert work == HW * Cp // (4 if dt == "f32" else 8)
    x = torch.from_numpy(K.hashed_small_ints(HW * Cp, seed=66).reshape(HW, Cp)).to(C.DT[dt])
    go, out = E.guarded_like((Cc, HW), torch.float32, DEV, sentinel=C.SENTINEL)
    ops.check(Lb.p2phd_nhwc_to_nchw(code, ops.ptr(x.to(DEV)), ops.ptr(out), 1, Cc, HW, Cp, off, ops.stream_ptr()), "nhwc_to_nchw")
    torch.cuda.synchronize()
    E.check_guards({"dst": go}, "nhwc_to_nchw")
    want = x[:, off:off + Cc].float().T.contiguous()
    # position of the walk: piece e = pc * HW + p; compare in [C, HW] order, a trip covers unit pieces = unit / 2 pixels of one piece column
    _same(out.cpu().view(torch.int32).numpy(), want.view(torch.int32).numpy(), unit, f"nhwc_to_nchw {dt}")


def test_nchw_cat_to_nhwc():
    """Two f32 sources of 3 and 2 channels into a pitch of 8 (f32) / 16 (16-bit storage): two pieces per pixel, pad channels +0."""
    from pix2pixhdaudiosr_amd import _ops as ops
    HW = K.TO_NCHW_HW
    for dt in ("f32", "bf16", "f16"):
        Lb = ops.lib_for(C.DT[dt])
        code, Cp = (0, 8) if dt == "f32" else (1, 16)
        work, unit = _past_the_cap("nchw_cat_to_nhwc", Lb)
        assert work == HW * Cp // (4 if dt == "f32" else 8)
        srcs = [K.hashed_small_ints(3 * HW, seed=67).reshape(3, HW), K.hashed_small_ints(2 * HW, seed=68).reshape(2, HW)]
        devs = [_dev(x) for x in srcs]
        ptrs = (ctypes.c_void_p * 2)(*[d.data_ptr() for d in devs])
        chans = (ctypes.c_int * 2)(3, 2)
        go, out = E.guarded_like((HW, Cp), C.DT[dt], DEV, sentinel=C.SENTINEL)
        ops.check(Lb.p2phd_nchw_cat_to_nhwc(code, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(chans, ctypes.c_void_p), 2, ops.ptr(out), 1, HW, Cp,
                                            ops.stream_ptr()), "nchw_cat_to_nhwc")
        torch.cuda.synchronize()
        E.check_guards({"dst": go}, "nchw_cat_to_nhwc")
        want = torch.zeros((HW, Cp), dtype=C.DT[dt])
        want[:, 0:3] = torch.from_numpy(np.ascontiguousarray(srcs[0].T)).to(C.DT[dt])
        want[:, 3:5] = torch.from_numpy(np.ascontiguousarray(srcs[1].T)).to(C.DT[dt])
        bits = {2: torch.int16, 4: torch.int32}[out.element_size()]
        # the walk's piece e = pc * HW + p: compare piece column by piece column
        epp = Cp // 2
        for pc in range(2):
            _same(out.cpu()[:, pc * epp:(pc + 1) * epp].contiguous().view(bits).numpy(), want[:, pc * epp:(pc + 1) * epp].contiguous().view(bits).numpy(),
                  unit * epp, f"nchw_cat_to_nhwc {dt} piece column {pc}")


def _np_of(t):
    return t.float().numpy()


def test_avgpool_forward():
    """AvgPool2d(3, 2, 1, count_include_pad=False) in f32 on 2.5 trips of output pieces: odd H, even W, every border count."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(torch.float32)
    work, unit = _past_the_cap("avgpool_fwd", Lb)
    N, Cc, H, W = (K.POOL_FWD[k] for k in "NCHW")
    Ho, Wo = C.pool_out(H), C.pool_out(W)
    assert work == N * Ho * Wo * 2
    x = K.hashed_floats(N * H * W * Cc, seed=95).reshape(N, H, W, Cc)
    go, out = E.guarded_like((N, Ho, Wo, Cc), torch.float32, DEV, sentinel=C.SENTINEL)
    x_d = _dev(x)
    ops.check(Lb.p2phd_avgpool3s2_fwd(0, ops.ptr(x_d), ops.ptr(out), N, H, W, Cc, ops.stream_ptr()), "avgpool_fwd")
    torch.cuda.synchronize()
    E.check_guards({"y": go}, "avgpool_fwd")
    want, mag = K.avgpool_fwd_vec(x)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)
    bound = C.POOL_ULPS * C.U32 * mag * C.SMALL
    bad = np.flatnonzero(~(err <= bound).reshape(-1))
    assert len(bad) == 0, f"avgpool_fwd: first at element {bad[0]} (piece {bad[0] // 4}, mod unit_work {bad[0] // 4 % unit}); {len(bad)} of {err.size} outside the bound"


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_avgpool_backward(dt):
    """The exact adjoint on 2.5 trips of input pieces (two pieces per pixel), under POOL_ULPS and the storage rounding."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(C.DT[dt])
    code, Cc = (0, 8) if dt == "f32" else (1, 16)
    work, unit = _past_the_cap("avgpool_bwd_f32" if dt == "f32" else "avgpool_bwd_h16", Lb)
    N, H, W = (K.POOL_BWD[k] for k in "NHW")
    Ho, Wo = C.pool_out(H), C.pool_out(W)
    assert work == N * H * W * 2
    dy = torch.from_numpy(K.hashed_floats(N * Ho * Wo * Cc, seed=96).reshape(N, Ho, Wo, Cc)).to(C.DT[dt])
    go, out = E.guarded_like((N, H, W, Cc), C.DT[dt], DEV, sentinel=C.SENTINEL)
    ops.check(Lb.p2phd_avgpool3s2_bwd(code, ops.ptr(dy.to(DEV)), ops.ptr(out), N, H, W, Cc, ops.stream_ptr()), "avgpool_bwd")
    torch.cuda.synchronize()
    E.check_guards({"dx": go}, "avgpool_bwd")
    want, mag = K.avgpool_bwd_vec(_np_of(dy), H, W)
    want, b32 = torch.from_numpy(want), torch.from_numpy(C.POOL_ULPS * C.U32 * mag * C.SMALL)
    C.assert_within(out.reshape(N, H * W, Cc), want.reshape(N, H * W, Cc), C.stored_bound(want, b32, C.DT[dt]).reshape(N, H * W, Cc), f"avgpool_bwd {dt}", Cc)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_losses(dt):
    """loss_fwd (1024 workgroups: five trips and more) and loss_bwd (2048: 2.5 trips) on P x 72 with 67 valid channels, both
    kinds: the forward under the existing bound of the sum (tests/test_long_host.py shows that a float32 emulation in kernel order
    stays inside it at this size), the backward bit for bit."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(C.DT[dt])
    code = 0 if dt == "f32" else 1
    sfx = "f32" if dt == "f32" else "h16"
    work, unit_f = _past_the_cap("loss_fwd_" + sfx, Lb)
    work, unit_b = _past_the_cap("loss_bwd_" + sfx, Lb)
    P, Cc, Cp = K.LOSS_P[code], K.LOSS_C, K.LOSS_CP
    a, b = K.loss_operands(P, dt)
    ad, bd = a.to(DEV), b.to(DEV)
    target, coeff, gup = 0.9, 0.5, 1.75
    gup_d = torch.tensor([gup], dtype=torch.float32, device=DEV)
    bits = {2: torch.int16, 4: torch.int32}[a.element_size()]
    for kind in (0, 1):
        go, out = E.guarded_like((1,), torch.float32, DEV, sentinel=C.OUT0)
        ops.check(Lb.p2phd_loss_fwd(kind, code, ops.ptr(ad), ops.ptr(bd), target, P, Cc, coeff, ops.ptr(out), ops.stream_ptr()), "loss_fwd")
        gda, da = E.guarded_like((P, Cp), C.DT[dt], DEV, sentinel=C.SENTINEL)
        ops.check(Lb.p2phd_loss_bwd(kind, code, ops.ptr(ad), ops.ptr(bd), target, P, Cc, coeff, ops.ptr(gup_d), ops.ptr(da), ops.stream_ptr()), "loss_bwd")
        torch.cuda.synchronize()
        E.check_guards({"out": go, "da": gda}, "loss")
        want, bound = C.loss_fwd_reference(kind, a, b, target, Cc, coeff, C.OUT0)
        got = float(out.cpu())
        print(f"loss_fwd kind {kind} {dt}: got {got!r}, want {want!r}, |difference| {abs(got - want):.3e}, bound {bound:.3e}")
        assert abs(got - want) <= bound, (kind, dt, got, want, bound)
        wb = C.loss_bwd_reference(kind, a, b, target, Cc, coeff, gup, C.DT[dt])
        _same(da.cpu().view(bits).numpy(), wb.view(bits).numpy(), unit_b, f"loss_bwd kind {kind} {dt}")


# ------------------------------------------------------------------------------------------
# loudness blocks, pack pair, range fold
# ------------------------------------------------------------------------------------------
def test_loudness_blocks_and_short_term():
    """Integer hop energies in [2^19, 2^20), C = 2: every 400 ms and every 3 s block power bit for bit against the numpy sliding
    sums; then the single-workgroup gate and range kernels on that many blocks (the report of a 36-hour file), under the rules of
    tests/test_gpu_loudness_album.py and tests/test_gpu_loudness_range.py."""
    import math
    import _loudness_ref as R
    import _loudness_range_ref as RR
    L = _lib()
    NB, unit = _past_the_cap("loudness_blocks")
    NS, _ = _past_the_cap("loudness_short_term")
    J, RATE = NB + 3, 48000
    assert NS == J - 29
    z = (K.index_hash(2 * J, seed=97) % np.uint32(1 << 19)).astype(np.float64).reshape(2, J) + float(1 << 19)
    zd = _dev(z)
    w = (ctypes.c_float * 2)(1.0, 1.0)
    gp = _out(NB * 8)
    L.check(L.lib().p2phd_loudness_blocks(L.ptr(zd), J, 2, RATE, ctypes.cast(w, ctypes.c_void_p), _vp(gp.ptr()), L.stream_ptr()), "loudness_blocks")
    p = _host(gp, np.float64)
    ref = R.gating(z, RATE, (1.0, 1.0))
    _same(p.view(np.uint64), ref["p"].view(np.uint64), unit, "loudness_blocks")
    gs = _out(NS * 8)
    L.check(L.lib().p2phd_loudness_short_term(L.ptr(zd), J, 2, RATE, ctypes.cast(w, ctypes.c_void_p), None, _vp(gs.ptr()), L.stream_ptr()), "short_term")
    ps = _host(gs, np.float64)
    _same(ps.view(np.uint64), RR.block_powers(z, RATE, (1.0, 1.0)).view(np.uint64), unit, "loudness_short_term")

    def same_level(got, want, tol):
        return math.isnan(got) if math.isnan(want) else (got == want if math.isinf(want) else abs(got - want) <= tol)
    res4 = torch.full((4,), -7.25, dtype=torch.float64, device=DEV)
    gain = torch.full((1,), -7.25, dtype=torch.float32, device=DEV)
    L.check(L.lib().p2phd_loudness_gate_blocks(_vp(gp.ptr()), NB, -23.0, None, 40.0, L.ptr(res4), L.ptr(gain), L.stream_ptr()), "gate_blocks")
    r4 = res4.cpu().numpy()
    assert min(np.abs(ref["l"] + 70.0).min(), np.abs(ref["l"] - ref["gamma"]).min()) > 1e-3      # no block near a threshold
    assert same_level(r4[0], ref["I"], 1e-6) and same_level(r4[1], ref["max"], 1e-6) and same_level(r4[2], ref["gamma"], 1e-6), (r4, ref["I"])
    assert r4[3] == ref["kept"] == NB
    wg = np.float32(R.gain(float(r4[0]), -23.0, 40.0))
    assert abs(np.float32(gain.cpu()[0]) - wg) <= np.spacing(wg)
    res8 = torch.full((8,), -7.25, dtype=torch.float64, device=DEV)
    L.check(L.lib().p2phd_loudness_range(_vp(gs.ptr()), NS, L.ptr(res8), L.stream_ptr()), "loudness_range")
    r8 = res8.cpu().numpy()
    want = RR.loudness_range(ps)
    assert r8[4] == want["n"] == NS
    assert r8[6:8].view(np.uint64).tolist() == np.array([want["q_lo"], want["q_hi"]]).view(np.uint64).tolist()
    for k, name in ((0, "lra"), (1, "low"), (2, "high"), (3, "threshold"), (5, "short_term_max")):
        assert same_level(float(r8[k]), want[name], 1e-9), (name, r8[k], want[name])


@pytest.mark.parametrize("dt,shift", [("bf16", 0), ("f16", 0), ("f32", 0), ("f32", 1)])
def test_pack_pair_raw(dt, shift):
    """The raw mode (channels 0, 1 = the two sources rounded once to storage, 2..7 = +0) on 2.5 trips of quads, bit for bit against
    tests/_timed_ref.pack_raw_expected (the device's own cast), compared on the device; shift 1: sources one float in, the scalar
    loads."""
    import _timed_ref as T
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(C.DT[dt])
    n, unit = _past_the_cap("pack_pair", Lb)
    assert n % 4 != 0
    a = _dev(K.hashed_floats(n + 4, seed=98))[shift:shift + n]
    b = _dev(K.hashed_floats(n + 4, seed=99))[shift:shift + n]
    go, out = E.guarded_like((n, 8), C.DT[dt], DEV, sentinel=C.SENTINEL)
    ops.check(Lb.p2phd_timed_pack_pair(0 if dt == "f32" else 1, ops.ptr(a), ops.ptr(b), n, 0, 0.0, ops.ptr(out), ops.stream_ptr()), "pack_pair")
    torch.cuda.synchronize()
    E.check_guards({"dst": go}, "pack_pair")
    want = T.pack_raw_expected(a, b, C.DT[dt])
    bits = {2: torch.int16, 4: torch.int32}[out.element_size()]
    diff = (out.view(bits) != want.view(bits)).any(dim=1).nonzero().flatten()
    assert diff.numel() == 0, f"pack_pair {dt}: first differing pixel {int(diff[0])} (mod unit_work {int(diff[0]) % unit}); {diff.numel()} of {n} pixels differ"


def test_pack_pair_db():
    """The dB mode in f32 on the same 2.5 trips: 20 log10(max(|x|, min_value)) - 20 of both sources within the bound
    tests/_timed_ref.pack_db_ref derives, channels 2..7 +0."""
    import _timed_ref as T
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(torch.float32)
    n, unit = _past_the_cap("pack_pair", Lb)
    decade = (K.index_hash(n, seed=121) >> np.uint32(8)).astype(np.float32) * np.float32(8.0 / (1 << 24))
    a = (K.hashed_floats(n, seed=122) * np.float32(10.0) ** -decade).astype(np.float32)       # eight decades: the clamp at min_value is reached
    b = (K.hashed_floats(n, seed=123) * np.float32(1e3)).astype(np.float32)
    go, out = E.guarded_like((n, 8), torch.float32, DEV, sentinel=C.SENTINEL)
    ad, bd = _dev(a), _dev(b)                                         # (both alive until the launch has run)
    ops.check(Lb.p2phd_timed_pack_pair(0, ops.ptr(ad), ops.ptr(bd), n, 1, T.MIN_VALUE, ops.ptr(out), ops.stream_ptr()), "pack_pair dB")
    torch.cuda.synchronize()
    E.check_guards({"dst": go}, "pack_pair dB")
    assert bool((out[:, 2:].view(torch.int32) == 0).all())
    want, tol = T.pack_db_ref(a, b, T.MIN_VALUE, torch.float32)
    err = np.abs(out[:, :2].cpu().numpy().astype(np.float64) - want)
    bad = np.flatnonzero(~(err <= tol).all(axis=1))
    assert len(bad) == 0, f"pack_pair dB: first pixel {bad[0]} (mod unit_work {bad[0] % unit}); {len(bad)} of {n} pixels outside the bound"


@pytest.mark.parametrize("cid,shift", [("range_fold", 0), ("range_fold_scalar", 1)])
def test_range_fold(cid, shift):
    """The plain min / max fold (no rounding: exact) on the float4 path with its scalar tail and on the path of any alignment.  The
    minimum lies in the second trip, the maximum in the third, partial one; NaN entries are passed over; the incoming range is kept
    where it is wider."""
    L = _lib()
    n, unit = _past_the_cap(cid)
    x = K.hashed_floats(n, seed=101)
    x[unit + unit // 3] = -5.0
    x[2 * unit + unit // 5] = 7.0
    x[n - 1] = 6.0                                                    # (the scalar tail behind the last float4)
    x[3::100003] = np.nan
    buf = _dev(np.concatenate([np.zeros(shift, dtype=np.float32), x]))
    gpart = E.Guarded(4 * 1024 * 4, DEV, 0xFF)
    for start, want in (((np.inf, -np.inf), (-5.0, 7.0)), ((-9.0, 1.0), (-9.0, 7.0))):
        gio, io = E.guarded_like((2,), torch.float32, DEV, sentinel=0.0)
        io.copy_(torch.tensor(start, dtype=torch.float32))
        L.check(L.lib().p2phd_range_fold(_vp(buf.data_ptr() + 4 * shift), n, L.ptr(io), _vp(gpart.ptr()), L.stream_ptr()), cid)
        torch.cuda.synchronize()
        E.check_guards({"minmax": gio, "partials": gpart}, cid)
        assert tuple(io.cpu().tolist()) == want, (cid, start, io.cpu().tolist())
    x[n - 1] = 8.0                                                    # now the maximum is the last scalar element
    buf[shift + n - 1] = 8.0
    gio, io = E.guarded_like((2,), torch.float32, DEV, sentinel=0.0)
    io.copy_(torch.tensor((np.inf, -np.inf), dtype=torch.float32))
    L.check(L.lib().p2phd_range_fold(_vp(buf.data_ptr() + 4 * shift), n, L.ptr(io), _vp(gpart.ptr()), L.stream_ptr()), cid)
    torch.cuda.synchronize()
    assert tuple(io.cpu().tolist()) == (-5.0, 8.0)


def test_spectro_encode_statistics_and_range():
    """p2phd_spectro_encode_ex with noise rows and signs (mask mode 1): the normalisation pass on 2.5 trips of its 8192 workgroups,
    the noise statistics on 2.5 trips of their 1024, and p2phd_spectro_range on 2.5 trips of float4 with a scalar tail -- against
    tests/_transform_ref.encode_ref and its derived bounds, unchanged.  The extremes of the spectrum and of the noise lie beyond
    the first trip."""
    import _transform_ref as R
    from _exact import assert_bits_equal, guarded_like, check_guards
    L = _lib()
    total, unit_e = _past_the_cap("spectro_encode")
    n_noise, unit_s = _past_the_cap("spectro_stats")
    n_spec, unit_r = _past_the_cap("spectro_range")
    B, Cc, F, M, mask_rows = (K.SPECTRO[k] for k in ("B", "C", "F", "M", "mask_rows"))
    decade = (K.index_hash(n_spec, seed=111) >> np.uint32(8)).astype(np.float64) * (4.0 / (1 << 24))
    spec = (K.hashed_floats(n_spec, seed=110).astype(np.float64) * 100.0 * 10.0 ** -decade).astype(np.float32).reshape(B, F, M)
    rows = [(unit_r + unit_r // 3) // M, (2 * unit_r + unit_r // 4) // M, F - 1]       # bin 0 of a row of the second trip, of the third
    spec[0, rows[0], 0], spec[0, rows[1], 0], spec[0, rows[2], 0] = 1e3, -1e3, 0.0
    spec.reshape(-1)[n_spec - 1] = 5e-8                               # the scalar tail of the range pass: the clamp branch
    noise = K.hashed_floats(n_noise, seed=112).reshape(B, Cc, mask_rows, F).copy()
    noise.reshape(-1)[unit_s + 17], noise.reshape(-1)[2 * unit_s + 4099] = -3.0, 2.5
    sign = np.where(K.index_hash(n_noise, seed=113) & np.uint32(1), np.float32(1), np.float32(-1)).astype(np.float32).reshape(noise.shape)
    bufs = {}
    bufs["log_spectro"], out = guarded_like((B, Cc, M, F), torch.float32, DEV, 0.7)
    bufs["pha"], pha = guarded_like((B, 1, M, F), torch.float32, DEV, 0.7)
    bufs["norm"], norm = guarded_like((8,), torch.float32, DEV, 0.7)
    bufs["partials"], part = guarded_like((int(L.lib().p2phd_spectro_partials_floats(B, F, M)),), torch.float32, DEV, 0.7)
    sd, nd, gd = _dev(spec), _dev(noise), _dev(sign)
    what = "spectro_encode_ex past the cap"
    L.check(L.lib().p2phd_spectro_encode_ex(L.ptr(sd), B, F, M, Cc, 0.6, R.MIN_VALUE, mask_rows, 1, L.ptr(nd), L.ptr(gd), L.ptr(out), L.ptr(pha),
                                            L.ptr(norm), L.ptr(part), L.stream_ptr()), what)
    torch.cuda.synchronize()
    check_guards(bufs, what)
    got, norm_h = out.cpu().numpy(), norm.cpu().numpy()
    ref = R.encode_ref(spec, Cc, 0.6, R.MIN_VALUE, mask_rows, 1, noise, sign)
    keep = ref["keep"]
    assert_bits_equal(pha.cpu(), torch.from_numpy(ref["pha"]), "flat", what + " pha")
    for i, name in enumerate(("min", "max", "mean", "std")):
        err, tol = abs(float(norm_h[i]) - ref["norm"][i]), ref["norm_tol"][i]
        print(f"{what}: {name} got {norm_h[i]!r} want {ref['norm'][i]!r} |err| / tol = {err / tol if tol else 0.0:.3f}")
        assert err <= tol, (name, float(norm_h[i]), ref["norm"][i], tol)
    assert norm_h[4] == np.float32(-3.0) and norm_h[5] == np.float32(2.5), norm_h[4:6]      # float32 extremes are exact
    R.assert_elements_close(got[:, :, :keep], ref["out"][:, :, :keep], ref["out_tol"][:, :, :keep], what + " kept rows", ("b", "c", "m", "f"))
    R.assert_elements_close(got[:, :, keep:], ref["out"][:, :, keep:], ref["out_tol"][:, :, keep:], what + " masked rows", ("b", "c", "m", "f"))
    # the range pass: the bits the encode left in norm[0:2] (its contract), so within the same bounds of the float64 extremes
    gio, io = guarded_like((2,), torch.float32, DEV, 0.0)
    io.copy_(torch.tensor((np.inf, -np.inf), dtype=torch.float32))
    part.fill_(0.7)
    L.check(L.lib().p2phd_spectro_range(L.ptr(sd), B, F, M, Cc, 0.6, R.MIN_VALUE, L.ptr(io), L.ptr(part), L.stream_ptr()), "spectro_range")
    torch.cuda.synchronize()
    check_guards({"minmax": gio, "partials": bufs["partials"]}, "spectro_range")
    mm = io.cpu().numpy()
    assert mm.view(np.uint32).tolist() == norm_h[0:2].view(np.uint32).tolist(), (mm, norm_h[0:2])
    assert abs(float(mm[0]) - ref["norm"][0]) <= ref["norm_tol"][0] and abs(float(mm[1]) - ref["norm"][1]) <= ref["norm_tol"][1]


LR, B1, B2, AEPS, GSCALE, SCALE = 3e-4, 0.5, 0.999, 1e-8, 0.25, 1024.0


def _adam_state(n, seed):
    p, g, m = (torch.from_numpy(K.hashed_floats(n, seed=seed + i)) for i in range(3))
    v = torch.from_numpy(np.abs(K.hashed_floats(n, seed=seed + 3))) * 0.1
    return p, g, m * 0.1, v


def _adam_bufs(state):
    bufs, tens = {}, []
    for name, t in zip("pgmv", state):
        bufs[name], d = E.guarded_like(tuple(t.shape), torch.float32, DEV, sentinel=C.SENTINEL)
        d.copy_(t)
        tens.append(d)
    return bufs, tens


@pytest.mark.parametrize("entry", ["adam_step", "adam_step_dev"])
def test_adam(entry):
    """One step at step count 1000 on 2.5 trips of the 4096-workgroup grid, ending in the scalar tail: the float64 reference and
    the derived bounds of tests/_companions.py."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(torch.float32)
    n, unit = _past_the_cap(entry, Lb)
    assert n % 4 != 0
    state = _adam_state(n, 71)
    bufs, (p, g, m, v) = _adam_bufs(state)
    t = 1000
    if entry == "adam_step":
        ops.check(Lb.p2phd_adam_step(ops.ptr(p), ops.ptr(g), ops.ptr(m), ops.ptr(v), n, LR, B1, B2, AEPS, t, GSCALE, ops.stream_ptr()), entry)
    else:
        lr_dev = torch.tensor([LR], dtype=torch.float32, device=DEV)
        step_dev = torch.tensor([t - 1], dtype=torch.int64, device=DEV)
        ops.check(Lb.p2phd_adam_step_dev(ops.ptr(p), ops.ptr(g), ops.ptr(m), ops.ptr(v), n, ops.ptr(lr_dev), ops.ptr(step_dev), B1, B2, AEPS,
                                         GSCALE, ops.stream_ptr()), entry)
    torch.cuda.synchronize()
    E.check_guards(bufs, entry)
    want, bounds = C.adam_reference(*state, LR, B1, B2, AEPS, t, GSCALE)
    for name, got, w, b in zip("pmv", (p, m, v), want, bounds):
        C.assert_within(got, w, b, f"{entry} n {n} {name}")
    assert torch.equal(g.cpu().view(torch.int32), state[1].view(torch.int32))
    if entry == "adam_step_dev":
        assert int(step_dev.item()) == t


def test_scaled_adam_skips_on_an_inf_in_the_last_partial_trip():
    """The non-finite scan (2048 workgroups, four float4 in flight) on 2.5 of its trips: a single Inf in the last, partial trip --
    p, m, v keep their bits, the step count does not move, the flag of found_index is set.  Then the same buffers with the Inf
    taken out: the step is taken (Adam's own grid is past five trips there)."""
    from pix2pixhdaudiosr_amd import _ops as ops
    Lb = ops.lib_for(torch.float32)
    n, unit = _past_the_cap("adam_step_scaled", Lb)
    p, g, m, v = _adam_state(n, 81)
    g = g * SCALE
    pos = 2 * unit + unit // 4 + 3                                    # inside the third trip of the scan, in its body
    assert pos < n // 4 * 4 and n % 4 != 0
    for bad_at in (pos, None):
        gg = g.clone()
        if bad_at is not None:
            gg[bad_at] = float("inf")
        state = (p, gg, m, v)
        bufs, tens = _adam_bufs(state)
        bufs["scaler"], scaler = E.guarded_like((5,), torch.float32, DEV, sentinel=0.0)
        scaler.copy_(torch.tensor([SCALE, 1.0 / SCALE, 3.0, 0.0, 0.0]))
        lr_dev = torch.tensor([LR], dtype=torch.float32, device=DEV)
        step_dev = torch.tensor([6], dtype=torch.int64, device=DEV)
        ops.check(Lb.p2phd_adam_step_scaled(*(ops.ptr(t) for t in tens), n, ops.ptr(lr_dev), ops.ptr(step_dev), B1, B2, AEPS, GSCALE,
                                            ops.ptr(scaler), 1, ops.stream_ptr()), "adam_step_scaled")
        torch.cuda.synchronize()
        E.check_guards(bufs, "adam_step_scaled")
        if bad_at is not None:
            for name, got, w in zip("pgmv", tens, state):
                _same(got.cpu().view(torch.int32).numpy(), w.view(torch.int32).numpy(), unit, f"adam_step_scaled skipped: {name}")
            assert int(step_dev.item()) == 6 and scaler.cpu().tolist() == [SCALE, 1.0 / SCALE, 3.0, 0.0, 1.0]
        else:
            want, bounds = C.adam_reference(*state, LR, B1, B2, AEPS, 7, GSCALE / SCALE)
            for name, got, w, b in zip("pmv", (tens[0], tens[2], tens[3]), want, bounds):
                C.assert_within(got, w, b, f"adam_step_scaled clean n {n} {name}")
            assert int(step_dev.item()) == 7 and scaler.cpu().tolist() == [SCALE, 1.0 / SCALE, 3.0, 0.0, 0.0]
