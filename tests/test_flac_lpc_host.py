"""The LPC option of the FLAC encoder on the host (csrc/flacenc.hip: p2phd_flac_lpc_fit / p2phd_flac_lpc_analyse /
p2phd_flac_encode_lpc_host; data/flacio.py: encode(lpc_order=M)) against the restatement tests/_flac_lpc_ref.py, byte for byte: no
tolerance anywhere.  Every stream is also put through code this encoder did not write: the index (every CRC, the chaining), the host
decoder and the restatement's decoder of the FLAC reader, and must return the payload.

The restatement's writer and decoder are plain Python, so the product channels x bits x block x length x M is covered like this: every
combination at the blocks up to 256; at 4096, 4608 and 16384 every value of every factor, in combinations that rotate with the case."""
import ctypes
import hashlib

import numpy as np
import pytest

import _flac_enc_cases as K
import _flac_enc_ref as E
import _flac_lpc_cases as C
import _flac_lpc_ref as P
import _flac_ref as R


def _flacio():
    from pix2pixhdaudiosr_amd.data import flacio
    return flacio


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L.lib()


def _unpack(ok, q, shift):
    return {o + 1: ([int(v) for v in q[o, :o + 1]], int(shift[o])) for o in range(12) if ok[o]}


def lib_fit(Rl):
    Rl = np.asarray(Rl, dtype=np.int64)
    ok, q, shift = np.full(12, -1, dtype=np.int32), np.full((12, 12), -1, dtype=np.int32), np.full(12, -1, dtype=np.int32)
    rc = _lib().p2phd_flac_lpc_fit(ctypes.c_void_p(Rl.ctypes.data), len(Rl) - 1, *(ctypes.c_void_p(a.ctypes.data) for a in (ok, q, shift)))
    assert rc == 0, _lib().p2phd_last_error()
    assert not q[ok == 0].any() and not shift[ok == 0].any() and all(not q[o, o + 1:].any() for o in range(12))
    return _unpack(ok, q, shift)


def lib_analyse(x, bps, M):
    x = np.ascontiguousarray(x, dtype=np.int32)
    ok, q, shift, Rl = np.full(12, -1, dtype=np.int32), np.full((12, 12), -1, dtype=np.int32), np.full(12, -1, dtype=np.int32), np.full(13, -1, dtype=np.int64)
    rc = _lib().p2phd_flac_lpc_analyse(ctypes.c_void_p(x.ctypes.data), len(x), bps, M, *(ctypes.c_void_p(a.ctypes.data) for a in (ok, q, shift, Rl)))
    assert rc == 0, _lib().p2phd_last_error()
    Mo = min(M, len(x) - 1)
    assert not Rl[Mo + 1:].any() and not ok[Mo:].any()
    return [int(v) for v in Rl[:Mo + 1]], _unpack(ok, q, shift)


def _check_stream(channels, bits, rate, block, M, want=None):
    """Host encoder == restatement, and the stream stands: -> (frames of the restatement, its decisions)."""
    f = _flacio()
    Cn, L = len(channels), len(channels[0])
    want, decisions = P.encode_frames(channels, bits, rate, block, M) if want is None else want
    pay = E.payload(channels, bits)
    got, lengths = f.encode(pay, Cn, bits, rate, block, lpc_order=M)
    assert lengths.tolist() == [len(x) for x in want] + [sum(map(len, want))]
    assert got == b"".join(want)
    nframes, worst, _ = f.encode_plan(Cn, bits, L, block)
    assert nframes == len(want) == -(-L // block) and len(got) <= worst
    data = f.stream_header(lengths, rate, Cn, bits, L, block, hashlib.md5(pay).digest()) + got
    meta, table = f.index_bytes(data)                                       # p2phd_flac_info / p2phd_flac_index: every CRC, the chaining
    assert (meta.sample_rate, meta.num_frames, meta.num_channels, meta.bits_per_sample, meta.num_flac_frames) == (rate, L, Cn, bits, nframes)
    assert table[:, 1].tolist() == lengths[:-1].tolist()
    assert np.array_equal(f.decode_frames(data, table, 0, nframes, Cn), np.array(channels))      # p2phd_flac_decode_host
    info, out = R.decode_stream(data)                                       # the restatement's decoder of the FLAC reader
    assert out == [[int(v) for v in c] for c in channels]
    return want, decisions


# ---- steps 1 to 3 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [16, 17, 192, 256, 1152, 4096])
def test_analyse_is_the_restatement(bs):
    """R, the admitted flags, q and shift of every order, at 16, 17 (a side channel), 24 and 25 bits per sample."""
    for i, bps in enumerate((16, 17, 24, 25)):
        bits = 16 if bps < 24 else 24
        for x in (C.resonant(bs, bs + i, bits), K.tone(bs, bits, i), K.full_noise(bs, bits, i), C.resonant(bs, i, bits, (900.0, 5000.0), 0.01)):
            x = np.array(x) * (2 if bps in (17, 25) else 1)                 # (the extra bit in use)
            for M in (1, 5, 12):
                assert lib_analyse(x, bps, M) == P.analyse(x, bps, M)
    Rl, fits = P.analyse(C.resonant(bs, 1), 16, 12)
    assert len(Rl) == min(12, bs - 1) + 1 and sorted(fits) == list(range(1, len(Rl))) and all(abs(r) < 1 << 46 for r in Rl)


def test_fit_is_the_restatement_where_it_stops():
    """Steps 2 and 3 from R itself, through the routine both encoders call.  No block was found whose err ends <= 0 -- the autocorrelation
    of a windowed block is positive definite, and a pure alternating +-A keeps |k| below 1 (the case "alternating" below) -- so the stop
    rule is held with sequences R that no block produces: k = 1 at order 1, k = -1 at order 2 behind a zero, |k| > 1 (err < 0) at
    order 3, and random indefinite ones."""
    assert P.fit([5, 5, 5]) == {} and lib_fit([5, 5, 5]) == {}
    assert P.fit([0, 3, 1]) == {} and lib_fit([0, 3, 1]) == {}              # R[0] = 0: no candidate
    assert P.fit([4, 0, -4, 1]) == {} == lib_fit([4, 0, -4, 1])             # order 1: no coefficient; order 2: err = 0; nothing above
    got = P.fit([100, 50, 200, 10, 3])
    assert sorted(got) == [1] and lib_fit([100, 50, 200, 10, 3]) == got      # order 2 ends with err < 0
    rng = np.random.default_rng(5)
    stops = 0
    for _ in range(300):
        Rl = [int(v) for v in rng.integers(-1 << 40, 1 << 40, 13)]
        Rl[0] = abs(Rl[0]) + 1
        want = P.fit(Rl)
        stops += len(want) < 12
        assert lib_fit(Rl) == want
        assert sorted(want) == list(range(1, len(want) + 1)) or not want    # what is admitted is a prefix (no cmax = 0 here)
    assert stops > 250
    # positive definite ones: every order admitted
    for seed in range(20):
        v = np.random.default_rng(seed).integers(-30000, 30001, 300)
        Rl = [int((v[l:] * v[:300 - l]).sum()) for l in range(13)]
        assert lib_fit(Rl) == P.fit(Rl) and len(P.fit(Rl)) == 12


def test_analyse_and_fit_refusals():
    x = np.zeros(16, dtype=np.int32)
    out = [np.zeros(n, dtype=t) for n, t in ((12, np.int32), (144, np.int32), (12, np.int32), (13, np.int64))]
    ptrs = [ctypes.c_void_p(a.ctypes.data) for a in out]
    xp = ctypes.c_void_p(x.ctypes.data)
    for args, text in (((xp, 0, 16, 12), b"bs"), ((xp, 16385, 16, 12), b"bs"), ((xp, 16, 20, 12), b"bps"), ((xp, 16, 16, 0), b"lpc_order"),
                       ((xp, 16, 16, 13), b"lpc_order"), ((None, 16, 16, 12), b"null")):
        assert _lib().p2phd_flac_lpc_analyse(*args, *ptrs) != 0 and text in _lib().p2phd_last_error()
    x[3] = 1 << 15
    assert _lib().p2phd_flac_lpc_analyse(xp, 16, 16, 12, *ptrs) != 0 and b"does not fit" in _lib().p2phd_last_error()
    Rl = np.zeros(13, dtype=np.int64)
    rp = ctypes.c_void_p(Rl.ctypes.data)
    for args, text in (((rp, -1), b"orders"), ((rp, 13), b"orders"), ((None, 3), b"null")):
        assert _lib().p2phd_flac_lpc_fit(*args, *ptrs[:3]) != 0 and text in _lib().p2phd_last_error()
    Rl[2] = 1 << 53
    assert _lib().p2phd_flac_lpc_fit(rp, 12, *ptrs[:3]) != 0 and b"exact" in _lib().p2phd_last_error()


# ---- streams -------------------------------------------------------------------------------------------------------------------
def _lengths(block):
    return (1, block - 1, block + 1, 3 * block)


@pytest.mark.parametrize("block", [16, 17, 192, 256])
@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("Cn", [1, 2, 3])
def test_matrix_small_blocks(Cn, bits, block):
    """Every length and every M at every (channels, bits, block) of the small blocks."""
    for i, L in enumerate(_lengths(block)):
        channels = C.signal(Cn, bits, L, i + Cn + bits + block)
        for M in (1, 4, 12):
            _check_stream(channels, bits, 48000, block, M)


# (channels, bits, length as a function of the block, M): every value of every factor at each large block
LARGE = {4096: [(1, 16, 1, 12), (2, 24, -1, 4), (3, 16, +1, 1), (1, 24, 3, 12), (2, 16, 3, 1), (3, 24, -1, 12)],
         4608: [(2, 16, 1, 4), (3, 24, +1, 12), (1, 16, -1, 1), (1, 24, 3, 4), (2, 24, +1, 1), (3, 16, -1, 12)],
         16384: [(3, 24, 1, 1), (1, 16, +1, 12), (2, 24, -1, 4), (1, 16, 3, 4), (2, 16, +1, 12), (3, 24, -1, 1), (1, 24, -1, 12)]}


@pytest.mark.parametrize("block", sorted(LARGE))
def test_matrix_large_blocks(block):
    for i, (Cn, bits, rel, M) in enumerate(LARGE[block]):
        L = 1 if rel == 1 else 3 * block if rel == 3 else block + rel
        _check_stream(C.signal(Cn, bits, L, i + block), bits, 44100, block, M)


def test_order_zero_is_the_existing_entry():
    """M = 0 through the new entry: the existing entry's bytes and lengths."""
    lib = _lib()
    for Cn, bits, block, L in ((1, 16, 16, 40), (2, 24, 256, 700), (3, 16, 4096, 5000), (2, 16, 65535, 70000)):
        channels = C.signal(Cn, bits, L, Cn + block)
        pay = np.frombuffer(E.payload(channels, bits), dtype=np.uint8)
        nframes, worst, _ = _flacio().encode_plan(Cn, bits, L, block)
        outs = []
        for lpc in (False, True):
            out, lengths = np.zeros(worst, dtype=np.uint8), np.zeros(nframes + 1, dtype=np.int64)
            args = (ctypes.c_void_p(pay.ctypes.data), Cn, bits, L, 48000, block) + ((0,) if lpc else ()) + \
                   (ctypes.c_void_p(out.ctypes.data), worst, ctypes.c_void_p(lengths.ctypes.data))
            assert (lib.p2phd_flac_encode_lpc_host if lpc else lib.p2phd_flac_encode_host)(*args) == 0
            outs.append((out.tobytes(), lengths.tolist()))
        assert outs[0] == outs[1]
        assert _flacio().encode(pay, Cn, bits, 48000, block, lpc_order=0)[0] == outs[0][0][:outs[0][1][-1]]
        assert b"".join(P.encode_frames(channels, bits, 48000, block, 0)[0]) == b"".join(E.encode_frames(channels, bits, 48000, block)[0])


@pytest.mark.parametrize("name", sorted(C.decisions()))
def test_decisions(name):
    """Each decision is asserted on the restatement first, then the host encoder's bytes are the restatement's."""
    (channels, bits, rate, block, M), expect = C.decisions()[name]
    want = P.encode_frames(channels, bits, rate, block, M)
    assert expect(want[1]), want[1]
    _check_stream(channels, bits, rate, block, M, want)
    x = np.asarray(channels[0])
    if name == "short-last-frame":
        Rl, fits = P.analyse(x[16:], 16, 12)
        assert len(x[16:]) == 5 and len(Rl) == 5 and sorted(fits) == [1, 2, 3, 4] and lib_analyse(x[16:], 16, 12) == (Rl, fits)
        assert all(o < 5 for o, p in P.lpc_candidates(x[16:], 16, 16, 12))
    if name == "silent-analysis":
        assert P.analyse(x, 24, 12) == ([0] * 13, {}) == lib_analyse(x, 24, 12) and len(set(x.tolist())) > 1
        assert P.lpc_candidates(x, 24, 24, 12) == {}
    if name == "period-4":                                                  # k = 0 at order 1: cmax = 0, that order alone is not admitted
        Rl, fits = P.analyse(x, 16, 12)
        assert Rl[1] == 0 and sorted(fits) == list(range(2, 13)) and lib_analyse(x, 16, 12) == (Rl, fits)
    if name == "alternating":                                               # the window keeps |k| below 1: nothing stops (see test_fit_...)
        Rl, fits = P.analyse(x, 16, 12)
        assert sorted(fits) == list(range(1, 13)) and -Rl[0] < Rl[1] < -0.95 * Rl[0]
    if name == "side-full-scale":                                           # 25 bit: every admitted order's residuals stay inside the bound
        side = x - np.asarray(channels[1])
        assert int(np.abs(side).max()) >= 1 << 23
        for at in (0, 256):
            Rl, fits = P.analyse(side[at:at + 256], 25, 12)
            assert len(fits) == 12 and lib_analyse(side[at:at + 256], 25, 12) == (Rl, fits)
            assert all(int(np.abs(P.residual(side[at:at + 256], q, s)).max()) < P.RES_LIMIT for q, s in fits.values())
            assert len(P.lpc_candidates(side[at:at + 256], 25, 24, 12)) == sum(1 for o in range(1, 13) for p in range(9) if (256 >> p) > o)
    if name == "residual-bound":                                            # every order fits; the bound of step 4 rejects orders 5 .. 12
        side = np.asarray(C.bound_side())
        assert np.array_equal(side, x - np.asarray(channels[1])) and want[1][0][0] == R.MID_SIDE
        Rl, fits = P.analyse(side, 25, 12)
        assert sorted(fits) == list(range(1, 13)) and lib_analyse(side, 25, 12) == (Rl, fits)
        top = {o: int(np.abs(P.residual(side, q, s)).max()) for o, (q, s) in fits.items()}
        rejected = sorted(o for o, v in top.items() if v >= P.RES_LIMIT)
        assert rejected == list(range(5, 13)) and sorted({o for o, p in P.lpc_candidates(side, 25, 24, 12)}) == [1, 2, 3, 4]
        kind, o, p, ks = want[1][0][1][1]
        assert kind == "lpc" and o < min(rejected)
        # ... and the bound decides: without it a rejected order would have been cheaper than the chosen one
        free = min(8 + k * 25 + 4 + 5 + k * P.P + 6 + min(b for b, _ in P.rice_bits(np.clip(P.residual(side, *fits[k]), -(1 << 30), 1 << 30), 16384, k, 24).values())
                   for k in rejected)
        assert free < P.lpc_candidates(side, 25, 24, 12)[(o, p)][0]
    if name == "shift-clamp":
        import math
        Rl, fits = P.analyse(x, 16, 2)
        lp1 = Rl[1] / Rl[0]
        assert P.P - 1 - math.frexp(abs(lp1))[1] > 15 and fits[1][1] == 15 and fits[1][0] == [round(lp1 * 32768)]
    if name in C.TIES:
        fixed = E.choose(x, bits, bits)[1]
        c = P.lpc_candidates(x, bits, bits, M)
        low = min(t for t, _, _, _ in c.values())
        assert sorted(op for op, v in c.items() if v[0] == low) == C.TIES[name]
        assert low == fixed if name == "tie-lpc-fixed" else low < fixed


# ---- consequences --------------------------------------------------------------------------------------------------------------
ORDERS = (0, 1, 2, 4, 8, 12)


@pytest.mark.parametrize("kind", ["noise", "tone", "resonant"])
def test_frames_never_grow_with_the_order(kind):
    """The predictor of order o does not depend on M: every frame's length is non-increasing in M, and the plan's worst case holds."""
    x = {"noise": lambda: K.full_noise(2 * 4096 + 100, 16, 1), "tone": lambda: K.tone(2 * 4096 + 100, 16, 2, noise=3),
         "resonant": lambda: C.resonant(2 * 4096 + 100, 3)}[kind]()
    f = _flacio()
    pay = E.payload([x], 16)
    lengths = [f.encode(pay, 1, 16, 48000, 4096, lpc_order=M)[1] for M in ORDERS]
    for a, b in zip(lengths, lengths[1:]):
        assert (b <= a).all()
    assert lengths[-1][-1] <= f.encode_plan(1, 16, len(x), 4096)[1]
    if kind == "noise":
        assert all((v == lengths[0]).all() for v in lengths)                # VERBATIM throughout
    o12 = {o: v for o, v in P.analyse(x[:4096], 16, 12)[1].items()}
    for M in (1, 2, 4, 8):
        assert P.analyse(x[:4096], 16, M)[1] == {o: v for o, v in o12.items() if o <= M}


def test_resonant_fixture():
    """Seeded noise through five pole pairs at radius 0.97 (the formant frequencies of _flac_lpc_cases.FORMANTS), 16 bit, block 4096:
    at M = 12 the stream is at most 0.80 of the M = 0 stream -- on the restatement (it reads 0.63), whose bytes are the host encoder's."""
    x = C.resonant(3 * 4096, 7)
    sizes = {}
    for M in ORDERS:
        want = P.encode_frames([x], 16, 48000, 4096, M)
        sizes[M] = sum(map(len, want[0]))
        if M in (0, 12):
            _check_stream([x], 16, 48000, 4096, M, want)
        else:
            assert _flacio().encode(E.payload([x], 16), 1, 16, 48000, 4096, lpc_order=M)[0] == b"".join(want[0])
    print("resonant fixture, bytes of the frames by M:", sizes, "M = 12 over M = 0: %.3f" % (sizes[12] / sizes[0]))
    assert sizes[12] <= 0.80 * sizes[0]
    assert all(kind == "lpc" and o > 4 for _, subs in want[1] for kind, o, _, _ in subs)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    f = _flacio()
    pay = E.payload([K.tone(40, 16, 1)], 16)
    for kw, text in ((dict(lpc_order=13), "LPC order"), (dict(lpc_order=-1), "LPC order"), (dict(lpc_order=True), "LPC order"), (dict(lpc_order=4.0), "LPC order"),
                     (dict(lpc_order=1, block=16385), "at most 16384"), (dict(lpc_order=12, block=65535), "at most 16384"),
                     (dict(lpc_order=4, channels=9), "channels"), (dict(lpc_order=4, bits=20), "pcm16 or pcm24"), (dict(lpc_order=4, block=15), "block"),
                     (dict(lpc_order=4, rate=0), "rate")):
        args = dict(channels=1, bits=16, rate=48000, block=16)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            f.encode(pay, **args)
    assert f.encode(pay, 1, 16, 48000, 16385, lpc_order=0)[0] == f.encode(pay, 1, 16, 48000, 16385)[0]   # the block's limit comes with M > 0
    # the C entry itself
    p = np.frombuffer(pay, dtype=np.uint8)
    out, lengths = np.zeros(1 << 12, dtype=np.uint8), np.zeros(4, dtype=np.int64)
    pp, op, lp = (ctypes.c_void_p(a.ctypes.data) for a in (p, out, lengths))
    for args, text in (((pp, 1, 16, 40, 48000, 16, 13, op, 1 << 12, lp), b"lpc_order"), ((pp, 1, 16, 40, 48000, 16, -1, op, 1 << 12, lp), b"lpc_order"),
                       ((pp, 1, 16, 40, 48000, 16385, 1, op, 1 << 12, lp), b"at most 16384"), ((pp, 1, 16, 40, 48000, 16, 4, op, 8, lp), b"worst case"),
                       ((None, 1, 16, 40, 48000, 16, 4, op, 1 << 12, lp), b"null"), ((pp, 9, 16, 40, 48000, 16, 4, op, 1 << 12, lp), b"channels")):
        assert _lib().p2phd_flac_encode_lpc_host(*args) != 0 and text in _lib().p2phd_last_error()
        assert not out.any() and not lengths.any()
