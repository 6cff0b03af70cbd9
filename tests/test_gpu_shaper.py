"""The noise-shaped dither of the output stage on the GPU (csrc/shaper.hip: p2phd_pcm_encode_shaped; generate.pcm_encode with
dither='shaped') against the restatement of tests/_shaper_ref.py, byte for byte: operands fp32 holds exactly (no fmaf rounds, so
plain arithmetic is the oracle) at every chunk, length, channel count and placement; zero taps against p2phd_pcm_encode_ex with
TPDF; the three published tables where the restatement's tie flag is clear; pieces, clipping and non-finite samples, runs and
streams, the launch counter and every refusal.  Every call writes its payload between canaries."""
import ctypes

import numpy as np
import pytest
import torch

import _outstage_ref as O
import _shaper_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5
OFFSETS = (0, 1, 3, 0, 3)                                          # floats past a 16-byte boundary: where row 0 starts
PITCHES = (5, 2, 3, 1, 64, 9)                                      # floats between the end of a row and the next one
OUT_OFFSETS = (0, 2, 1, 6, 16, 7, 14)                              # bytes past a 16-byte boundary: where the payload starts
# seeds at which no emulated fmaf of the restatement lands on a float32 tie for the inputs of test_real_tables (found on the CPU;
# the test asserts the flag)
REAL_SEEDS = {('lipshitz9', 256): 127, ('lipshitz9', 2048): 5, ('e5', 256): 1, ('e5', 2048): 1, ('light3', 256): 1, ('light3', 2048): 1}


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"shaper", 1 if reset else 0)


def _tile(channels, chunk):
    T = int(_lib().lib().p2phd_shaper_tile_len(channels, chunk))
    assert T > 0
    return T


def _call(x, taps, chunk, gain=None, seed=0, first_index=0, case=0, over=None, stream=None):
    """p2phd_pcm_encode_shaped on rows placed as case `case` asks -> (return code, payload bytes, canaries intact).  `over`: arguments
    to hand over in place of the right ones (the refusals)."""
    L_ = _lib()
    x = np.ascontiguousarray(x, dtype=np.float32)
    C, F = x.shape
    ld = F + PITCHES[case % len(PITCHES)]
    off = OFFSETS[case % len(OFFSETS)]
    host = np.full(4 + off + C * ld + 4, np.float32(77.0))
    for c in range(C):
        host[4 + off + c * ld:4 + off + c * ld + F] = x[c]
    keep = torch.from_numpy(host).to(DEV)
    assert keep.data_ptr() % 16 == 0
    rows = keep[4 + off:]
    oo = OUT_OFFSETS[case % len(OUT_OFFSETS)]
    buf = torch.full((32 + oo + 2 * F * C + 32,), CANARY, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[32 + oo:]
    h = np.ascontiguousarray(taps, dtype=np.float32)
    g = None if gain is None else torch.tensor([gain], dtype=torch.float32, device=DEV)
    a = dict(planar=L_.ptr(rows), frames=F, channels=C, ld=ld, gain=L_.ptr(g), taps=ctypes.c_void_p(h.ctypes.data if h.size else None), K=h.size,
             chunk=chunk, seed=seed & 0xFFFFFFFFFFFFFFFF, first_index=first_index, out=L_.ptr(out))
    a.update(over or {})
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())            # the rows and the canaries were written on the current stream
    rc = L_.lib().p2phd_pcm_encode_shaped(a['planar'], a['frames'], a['channels'], a['ld'], a['gain'], a['taps'], a['K'], a['chunk'], a['seed'],
                                          a['first_index'], a['out'], L_.stream_ptr() if stream is None else ctypes.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    lo, hi = 32 + oo, 32 + oo + 2 * F * C
    if rc != 0:
        lo = hi = 0                                                # a refused call writes nothing at all
    intact = bool((got[:lo] == CANARY).all() and (got[hi:] == CANARY).all())
    return rc, got[lo:hi].tobytes(), intact


def _exact_operands(rng, C, F, gain):
    """x with v = x * gain * 32768 a multiple of 2^-8 under 100: with taps in {+-1, +-2} every u is a multiple of 2^-16 under 2^8 (|e| <
    1.5 whatever the taps are, so |u| < 100 + 16 * 2 * 1.5), no fmaf rounds and the restatement is plain arithmetic."""
    m = rng.integers(-25599, 25600, (C, F)).astype(np.float64)
    return (m * 2.0 ** -23 / (1.0 if gain is None else gain)).astype(np.float32)


@pytest.mark.parametrize("K", [1, 2, 9, 16])
def test_exact_operands_bit_for_bit(K):
    rng = np.random.default_rng(100 + K)
    taps = rng.choice([-2.0, -1.0, 1.0, 2.0], K).astype(np.float32)
    case = K
    for chunk in (256, 320):
        T = _tile(3, chunk)
        for F in sorted({1, 63, 255, 256, 257, 2 * 256 + 5, T - 1, T, T + 1, chunk + T + 1}):
            for C in (1, 2, 3):
                for gain in (None, 0.5):
                    x = _exact_operands(rng, C, F, gain)
                    seed = int(rng.integers(0, 1 << 62))
                    want = R.encode_shaped(x, taps, chunk, gain=gain, seed=seed)
                    assert not want['tie'] and np.abs(want['e']).max() <= 1.5
                    _count(reset=True)
                    rc, got, intact = _call(x, taps, chunk, gain=gain, seed=seed, case=case)
                    assert rc == 0 and intact and _count() == 1, (K, chunk, F, C, gain, case)
                    assert got == want['bytes'], (K, chunk, F, C, gain, case)
                    case += 1


@pytest.mark.parametrize("C,F", [(3, 256 * 2050 + 5),               # more than 1024 chunks: a workgroup takes several
                                 (5, 256 * 1500 + 77),              # ... and its rows do not fill the wave
                                 (33, 300), (64, 257), (70, 300), (130, 65)])          # one chunk per workgroup; more channels than a wave has lanes
def test_exact_operands_every_grid_shape(C, F):
    rng = np.random.default_rng(C)
    taps = np.array([2.0, -1.0], dtype=np.float32)
    x = _exact_operands(rng, C, F, None)
    want = R.encode_shaped(x, taps, 256, seed=9)
    assert not want['tie']
    for case in (0, 2):                                            # an aligned payload and an odd one
        rc, got, intact = _call(x, taps, 256, seed=9, case=case)
        assert rc == 0 and intact and got == want['bytes'], (C, F, case)


def test_zero_taps_are_tpdf():
    L_ = _lib()
    rng = np.random.default_rng(5)
    case = 0
    for C, F in ((1, 1000), (3, 5 * 256 + 100)):
        x = rng.uniform(-1.2, 1.2, (C, F)).astype(np.float32)
        x[0, 7], x[-1, F // 2] = np.float32("nan"), np.float32("-inf")
        xd = torch.from_numpy(x).to(DEV)
        for chunk in (256, 2048):
            for seed in (0, (1 << 40) + 3):
                for gain in (None, 0.7):
                    first = 3 * chunk * C
                    g = None if gain is None else torch.tensor([gain], dtype=torch.float32, device=DEV)
                    ref = torch.empty(2 * F * C, dtype=torch.uint8, device=DEV)
                    assert L_.lib().p2phd_pcm_encode_ex(L_.ptr(xd), F, C, F, 1, L_.ptr(g), 1, seed, first, L_.ptr(ref), L_.stream_ptr()) == 0
                    want = ref.cpu().numpy().tobytes()
                    assert want == O.encode_ex(x, "pcm16", gain=gain, tpdf=True, seed=seed, first_index=first)
                    for taps in (np.zeros(0, np.float32), np.zeros(9, np.float32), np.zeros(16, np.float32)):
                        rc, got, intact = _call(x, taps, chunk, gain=gain, seed=seed, first_index=first, case=case)
                        assert rc == 0 and intact and got == want, (C, F, chunk, seed, gain, taps.size)
                        case += 1


def _noise(C, F, level=0.3, seed=77):
    return (level * np.random.default_rng(seed).standard_normal((C, F)) / 3.0).clip(-level, level).astype(np.float32)


@pytest.mark.parametrize("curve", ["lipshitz9", "e5", "light3"])
@pytest.mark.parametrize("chunk", [256, 2048])
def test_real_tables(curve, chunk):
    """Noise at 0.3 of full scale, 3 channels, five chunks of 256 and a short one (or, at 2048, one lane per channel)."""
    from pix2pixhdaudiosr_amd.generate import pcm_encode, shaper_coefficients
    taps = shaper_coefficients(curve).numpy()
    assert np.array_equal(taps, R.taps_of(curve))
    x = _noise(3, 5 * 256 + 100)
    seed = REAL_SEEDS[(curve, chunk)]
    want = R.encode_shaped(x, taps, chunk, seed=seed)
    assert not want['tie'], "choose another seed: an emulated fmaf landed on a float32 tie"
    rc, got, intact = _call(x, taps, chunk, seed=seed, case=chunk // 256)
    assert rc == 0 and intact and got == want['bytes']
    assert pcm_encode(torch.from_numpy(x).to(DEV), dither='shaped', curve=curve, chunk=chunk, seed=seed).cpu().numpy().tobytes() == want['bytes']


def test_pieces_on_chunk_boundaries():
    taps = R.taps_of('lipshitz9')
    x = _noise(2, 3 * 256 + 40, seed=3)
    rc, whole, intact = _call(x, taps, 256, seed=21, first_index=4 * 256 * 2)
    assert rc == 0 and intact
    cut = 2 * 256
    rc1, a, ok1 = _call(x[:, :cut], taps, 256, seed=21, first_index=4 * 256 * 2, case=1)
    rc2, b, ok2 = _call(x[:, cut:], taps, 256, seed=21, first_index=(4 * 256 + cut) * 2, case=2)
    assert (rc1, rc2, ok1, ok2) == (0, 0, True, True) and a + b == whole
    # a piece that starts inside a chunk would start a history of its own: refused
    for first in (2, 256, 256 * 2 + 2, 255 * 2):
        rc, _, intact = _call(x, taps, 256, seed=21, first_index=first)
        assert rc != 0 and intact and b"first_index" in _lib().lib().p2phd_last_error(), first
    from pix2pixhdaudiosr_amd.generate import pcm_encode
    with pytest.raises(_lib().P2PHDError, match="first_index"):
        pcm_encode(torch.from_numpy(x).to(DEV), dither='shaped', chunk=256, first_index=6)


def test_clipping_and_non_finite_samples():
    taps = R.taps_of('lipshitz9')
    F = 3 * 256
    x = _noise(1, F, seed=11)
    x[0, :300] = 4.0                                               # clips across the first chunk boundary
    x[0, 400], x[0, 600] = np.float32("nan"), np.float32("inf")
    seed = 87                                                      # (the tie flag is clear at this one)
    want = R.encode_shaped(x, taps, 256, seed=seed)
    assert not want['tie'] and np.abs(want['e']).max() <= 1.5
    rc, got, intact = _call(x, taps, 256, seed=seed)
    assert rc == 0 and intact and got == want['bytes']
    q = np.frombuffer(got, dtype="<i2")
    assert (q[:300] == 32767).all() and q[400] == 0 and q[600] == 32767
    for lo, hi in ((300, 400), (401, 512), (601, F)):              # behind each of them the history is a history again: not stuck at a rail
        part = q[lo:hi].astype(np.int64)
        assert np.abs(part).max() < 32767 and len(set(part.tolist())) > 8
        assert np.abs(part - want['v'][0, lo:hi]).max() <= 1.5 * (1.0 + np.abs(taps).sum())


def test_runs_and_streams_repeat_the_bytes():
    taps = R.taps_of('e5')
    x = _noise(2, 1500, seed=8)
    first = _call(x, taps, 512, seed=4)
    assert first[0] == 0
    side = torch.cuda.Stream()
    for stream in (None, side, None):
        again = _call(x, taps, 512, seed=4, case=3, stream=stream)
        assert again[0] == 0 and again[2] and again[1] == first[1]


def test_launch_counter_and_refusals():
    L_ = _lib()
    taps = R.taps_of('light3')
    x = _noise(2, 300)
    _count(reset=True)
    assert _call(x, taps, 256)[0] == 0 and _count() == 1
    assert _call(x, taps, 256, gain=0.5)[0] == 0 and _count(reset=True) == 2
    assert _call(x[:, :0], taps, 256)[0] == 0 and _count() == 0                    # nothing to do: no launch
    assert L_.lib().p2phd_launch_count(b"pcm", 1) >= 0
    assert _call(x, taps, 256)[0] == 0 and L_.lib().p2phd_launch_count(b"pcm", 0) == 0    # a family of its own
    _count(reset=True)
    null = ctypes.c_void_p(None)
    for over, word in ((dict(K=17), b"K must"), (dict(K=-1), b"K must"), (dict(taps=null), b"null taps"), (dict(chunk=100), b"chunk"),
                       (dict(chunk=4100), b"chunk"), (dict(chunk=1 << 21), b"chunk"), (dict(chunk=0), b"chunk"), (dict(channels=0), b"channels"),
                       (dict(ld=299), b"ld"), (dict(frames=-1), b"frames"), (dict(first_index=-512), b"first_index"), (dict(planar=null), b"null"),
                       (dict(out=null), b"null"), (dict(planar=ctypes.c_void_p(2)), b"aligned"), (dict(gain=ctypes.c_void_p(2)), b"aligned")):
        rc, _, intact = _call(x, taps, 256, over=over)
        text = L_.lib().p2phd_last_error()
        assert rc != 0 and intact and b"pcm_encode_shaped" in text and word in text, (over, text)
    bad = np.array([1.0, np.nan], dtype=np.float32)
    assert _call(x, bad, 256)[0] != 0 and b"finite" in L_.lib().p2phd_last_error()
    assert _count() == 0
    assert L_.lib().p2phd_shaper_tile_len(0, 256) == -1 and L_.lib().p2phd_shaper_tile_len(2, 100) == -1
    assert b"shaper_tile_len" in L_.lib().p2phd_last_error()
