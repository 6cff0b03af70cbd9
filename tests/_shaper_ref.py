"""numpy restatement of the noise-shaped dither of whole-file generation's output stage (csrc/shaper.hip: p2phd_pcm_encode_shaped),
written from the contract of include/p2phd.h.  Every (chunk, channel) is a lane and all lanes step in lockstep, so a step is a
handful of vector operations whatever the clip's length.

fmaf(a, b, c) is emulated as float32(float64(a) * float64(b) + float64(c)).  The product of two float32 is exact in float64; the sum
is rounded to float64 and then to float32, which differs from one rounding only where the float64 sum lands exactly on a float32
tie.  The restatement watches for that (the low 29 bits of the float64 significand are 1000...0; sums in float32's subnormal range
count too) and returns a flag; a test that compares bits of the real tables requires the flag to be clear.

The taps reach an output in the order of the contract -- the oldest error first, the newest last -- but transposed: when e[n] is
known it is added, as tap k, to the pending sum of output n + k for every k at once.  Each pending sum still takes exactly the
fmaf of the contract in the contract's order.

Also here: the Welch estimate the spectral checks share, and the published curves as float64 literals."""
import numpy as np

import _outstage_ref as O

CURVES = {
    'lipshitz9': (2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847),
    'e5': (2.033, -2.165, 1.959, -1.590, 0.6149),
    'light3': (1.623, -0.982, 0.109),
}
CURVE_IDS = {'lipshitz9': 0, 'e5': 1, 'light3': 2}

_TIE_MASK = np.int64((1 << 29) - 1)
_TIE_HALF = np.int64(1 << 28)
_F32_TINY = 2.0 ** -126


def taps_of(curve):
    """The float64 literals of a curve rounded once to float32."""
    return np.array(CURVES[curve], dtype=np.float64).astype(np.float32)


def encode_shaped(planar, taps, chunk, gain=None, seed=0, first_index=0):
    """planar float32 [channels, frames], taps h[1..K] (float32), chunk -> {'bytes': the interleaved little-endian int16 payload,
    'tie': True where an emulated fmaf may have rounded twice, 'e': the error history [channels, frames] float32,
    'v': x * gain * 32768 [channels, frames] float32}."""
    x = np.asarray(planar, dtype=np.float32)
    C, F = x.shape
    h = np.asarray(taps, dtype=np.float32).reshape(-1)
    K = h.size
    chunk = int(chunk)
    first_index = int(first_index)
    if first_index % (chunk * C):
        raise ValueError("first_index %d is not a multiple of chunk * channels = %d" % (first_index, chunk * C))
    nh = -h.astype(np.float64)[:, None]                                    # [K, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        y = x if gain is None else (x * np.float32(gain)).astype(np.float32)
        v = (y * np.float32(32768)).astype(np.float32)
    idx = np.uint64(first_index) + (np.arange(F, dtype=np.uint64)[None, :] * np.uint64(C) + np.arange(C, dtype=np.uint64)[:, None])
    d = O.dither(seed, idx).reshape(C, F) if F else np.zeros((C, 0), dtype=np.float32)
    nchunks = -(-F // chunk) if F else 0
    steps = min(chunk, F)
    lanes = C * nchunks

    def lanes_of(a):                                                        # [C, F] -> [lanes, steps + K], zeros behind a row's end
        p = np.zeros((C, nchunks * chunk), dtype=np.float32)
        p[:, :F] = a
        p = p.reshape(lanes, chunk)[:, :steps]
        return np.concatenate([p, np.zeros((lanes, K), dtype=np.float32)], axis=1)
    V, D = lanes_of(v), lanes_of(d)
    R = np.zeros((lanes, steps), dtype=np.float32)
    W = np.zeros((lanes, steps), dtype=np.float32)
    E = np.zeros((lanes, steps), dtype=np.float32)
    pend = np.ascontiguousarray(V[:, :K].T)                                # pend[k]: the sum of output n + k so far
    tie = False
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(steps):
            u = pend[0] if K else V[:, n]
            w = (u + D[:, n]).astype(np.float32)
            r = np.rint(w)
            e = np.where(np.isfinite(w), r - u, np.float32(0)).astype(np.float32)
            R[:, n], W[:, n], E[:, n] = r, w, e
            if K:
                nxt = np.empty_like(pend)
                nxt[:-1] = pend[1:]
                nxt[-1] = V[:, n + K]
                s = nh * e.astype(np.float64)[None, :] + nxt.astype(np.float64)          # tap k into output n + k
                bits = s.view(np.int64)
                tie = tie or bool(((bits & _TIE_MASK) == _TIE_HALF).any()) or bool(((s != 0) & (np.abs(s) < _F32_TINY)).any())
                pend = s.astype(np.float32)
        q = np.where(np.isnan(W), np.float32(0), np.clip(R, np.float32(-32768), np.float32(32767))).astype(np.int32)

    def rows_of(a, dtype):                                                  # [lanes, steps] -> [C, F]
        p = np.zeros((lanes, chunk), dtype=dtype)
        p[:, :steps] = a
        return p.reshape(C, nchunks * chunk)[:, :F]
    payload = np.ascontiguousarray(rows_of(q, np.int32).T).astype("<i2").tobytes()
    return {'bytes': payload, 'tie': tie, 'e': rows_of(E, np.float32), 'v': v}


def sine(rate, frames=1 << 18, hz=997.0, level=0.25):
    """The test tone of the spectral checks, float32 [1, frames]."""
    n = np.arange(frames, dtype=np.float64)
    return (level * np.sin(2.0 * np.pi * hz * n / rate)).astype(np.float32)[None, :]


def welch(x, n_fft=8192, hop=4096):
    """Welch power spectrum of a 1-D sequence, Hann windows: P[k] = mean over segments of |X[k]|^2 / sum(w^2), so that white noise
    of variance s^2 reads s^2 in every bin."""
    x = np.asarray(x, dtype=np.float64)
    w = np.hanning(n_fft + 1)[:-1]
    starts = range(0, x.size - n_fft + 1, hop)
    acc = np.zeros(n_fft // 2 + 1)
    for s in starts:
        acc += np.abs(np.fft.rfft(x[s:s + n_fft] * w)) ** 2
    return acc / (len(starts) * np.sum(w * w))


def band_db(P, rate, lo, hi):
    """Mean power of the bins in [lo, hi) Hz, in dB."""
    f = np.arange(P.size) * (rate / (2.0 * (P.size - 1)))
    return 10.0 * np.log10(P[(f >= lo) & (f < hi)].mean())


def model_figures(curve, rate, n_fft=8192):
    """What the linear model says: white noise of 1/4 LSB^2 (rounding 1/12 + TPDF 1/6) through 1 - sum_k h[k] z^-k -> the figures of
    noise_figures, in dB re 1 LSB^2.  The sequential recursion follows it; a chunked one leaks the hump into the dip."""
    h = taps_of(curve).astype(np.float64) if curve else np.zeros(0)
    f = np.arange(n_fft // 2 + 1) * (rate / n_fft)
    P = 0.25 * np.abs(1.0 - np.exp(-2j * np.pi * np.outer(f / rate, np.arange(1, h.size + 1))) @ h) ** 2
    return {'mid': band_db(P, rate, 2000.0, 5000.0), 'low': band_db(P, rate, 100.0, 1000.0), 'high': band_db(P, rate, 15000.0, 22000.0),
            'total': 10.0 * np.log10(0.25 * (1.0 + np.sum(h * h)))}


def noise_figures(payload, v, rate):
    """The written int16 samples of a mono payload against v = x * 32768 -> dB re 1 LSB^2 of the noise in 2-5 kHz, 0.1-1 kHz,
    15-22 kHz, and in total."""
    q = np.frombuffer(payload, dtype="<i2").astype(np.float64)
    noise = q - np.asarray(v, dtype=np.float64).reshape(-1)
    P = welch(noise)
    return {'mid': band_db(P, rate, 2000.0, 5000.0), 'low': band_db(P, rate, 100.0, 1000.0), 'high': band_db(P, rate, 15000.0, 22000.0),
            'total': 10.0 * np.log10(np.mean(noise * noise))}
