"""Inputs of the tests of the FLAC encoder's LPC option (tests/test_flac_lpc_host.py, tests/test_gpu_flac_lpc.py): the signals and the
decision cases, each with what the restatement (tests/_flac_lpc_ref.py) must decide for it.  A case is (channels as int64 arrays, bits,
rate, block, M)."""
import functools
import math

import numpy as np

import _flac_enc_cases as K

FORMANTS = (500.0, 1500.0, 2500.0, 3500.0, 4500.0)                          # Hz at 48 kHz: the five pole pairs of the resonant fixture


def poles(x, freqs, radius=0.97, rate=48000.0):
    """x through one pole pair per frequency (float64, the plain recursion)."""
    y = np.asarray(x, dtype=np.float64)
    for fr in freqs:
        a1, a2 = 2.0 * radius * math.cos(2.0 * math.pi * fr / rate), -radius * radius
        out = np.zeros(len(y))
        p1 = p2 = 0.0
        for n in range(len(y)):
            p1, p2 = y[n] + a1 * p1 + a2 * p2, p1
            out[n] = p1
        y = out
    return y


@functools.lru_cache(maxsize=None)
def _resonant(L, seed, bits, freqs, level):
    y = poles(np.random.default_rng(seed).standard_normal(L), freqs)
    a = np.round(y / np.abs(y).max() * level * (1 << (bits - 1))).astype(np.int64)
    a.setflags(write=False)
    return a


def resonant(L, seed, bits=16, freqs=FORMANTS, level=0.5):
    """Seeded noise through the five pole pairs at radius 0.97, its peak at `level` of full scale."""
    return _resonant(L, seed, bits, tuple(freqs), level)


def signal(C, bits, L, seed):
    """Channels of a different kind each: resonant, a tone with noise, full-scale noise, DC, a quiet resonance ..."""
    kinds = (lambda c: resonant(L, seed + c, bits), lambda c: K.tone(L, bits, seed + c), lambda c: K.full_noise(L, bits, seed + c),
             lambda c: np.full(L, 7 - 3 * c, dtype=np.int64), lambda c: resonant(L, seed + c, bits, (900.0, 5000.0), 0.02))
    return [np.array(kinds[(c + seed) % 5](c)) for c in range(C)]


@functools.lru_cache(maxsize=None)
def bound_side(bs=16384, seed=1):
    """A 25-bit side channel on which the fit admits every order and the residual bound of step 4 rejects the higher ones: seeded noise
    through 12 real poles at 0.35 at an rms of a quarter of full scale, clipped, with 14 samples of alternating full scale at either end.
    The window hides the ends from the analysis, the predictor's coefficients sum to more than 16 in size, and at the ends the
    prediction passes 2^28."""
    y = np.random.default_rng(seed).standard_normal(bs)
    for _ in range(12):
        out = np.zeros(bs)
        p = 0.0
        for n in range(bs):
            p = y[n] + 0.35 * p
            out[n] = p
        y = out
    top = (1 << 24) - 1
    x = np.clip(np.round(y / np.sqrt((y * y).mean()) * 0.25 * (1 << 24)), -top, top).astype(np.int64)
    x[:14] = x[-14:] = np.where(np.arange(14) % 2 == 0, top, -top)
    x.setflags(write=False)
    return x


TIE_FIXED = [-2, 2, 2, -2, -10, -18, -10, 11, 39, 45, 24, -4, -16, -21, -33, -29, -10, 22, 35, 28, 17, 4, -13, -20, 1, 22, 27, -1, -33, -34, -19, 1,
             29, 28, 21, 1, -17, -26, -11, 4, 22, 16, 4, -1, -6, -14, -24, -29]
TIE_P = [-2, 2, -1, -1, 3, -3, -3, 8, -11, 15, -11, 5, 3, -16, 20, -16, 5, 4, -11, 14, -11, 4, 4, -10, 15, -16, 13, -8, -3, 13, -21, 11, 1, -13, 20,
         -18, 11, 1, -14, 18, -12, -3, 8, -10, 12, -10, 7, -4]
TIE_O = [14, -29, 30, -4, -27, 46, -23, 2, 29, -41, 29, -5, -28, 50, -46, 12, 27, -38, 27, -15, 4, -9, -1, 20, -22, 27, -17, 20, -23, 28, -11, 6, 16,
         -27, 26, 5, -12, 23, -33, 47, -32, 19, -17, 13, -26, 33, -24, 11, -6, 4, -1, -16, 26, -23, -1, 28, -48, 37, -32, 0, 28, -13, -8, 18]
# the LPC pairs (o, p) of equal, smallest bits of the tie cases at M = 4 (TIE_FIXED: its one cheapest LPC pair costs what FIXED costs)
TIES = {"tie-lpc-fixed": [(2, 0)], "tie-lpc-porder": [(2, 0), (2, 1)], "tie-lpc-order": [(1, 0), (2, 0)]}


@functools.lru_cache(maxsize=None)
def decisions():
    """name -> (case, expect): expect(decisions of the restatement, one (assignment, [(kind, order, porder, ks)]) per frame) -> bool."""
    rng = np.random.default_rng(23)
    kinds = lambda d: [s[0] for _, subs in d for s in subs]                 # noqa: E731
    two_pole = np.round(poles(rng.standard_normal(1024), (3000.0,), 0.98) * 200).astype(np.int64)
    quiet24 = rng.integers(0, 256, 256).astype(np.int64)                    # 24 bit, every sample below 2^8: the analysis signal is silent
    p4 = np.array([0, 20000, 0, -20000] * 64, dtype=np.int64)               # every other sample 0: R[1] = 0, order 1 has no coefficient
    alt = np.where(np.arange(256) % 2 == 0, 20000, -20000).astype(np.int64)
    white = rng.integers(-3000, 3001, 4096).astype(np.int64)
    return {
        "two-pole-lpc": (([two_pole], 16, 48000, 1024, 12), lambda d: kinds(d) == ["lpc"]),
        # the last frame has 5 samples: orders 1 .. 4 alone
        "short-last-frame": (([resonant(21, 3, 16, level=0.9)], 16, 48000, 16, 12), lambda d: all(s[1] < 5 for s in d[1][1])),
        "silent-analysis": (([quiet24], 24, 48000, 256, 12), lambda d: kinds(d)[0] in ("fixed", "verbatim")),
        "period-4": (([p4], 16, 48000, 256, 12), lambda d: True),
        "alternating": (([alt], 16, 48000, 256, 12), lambda d: True),
        "side-full-scale": (([K.full_noise(512, 24, 5), K.full_noise(512, 24, 6)], 24, 96000, 256, 12), lambda d: "lpc" not in kinds(d)),
        "shift-clamp": (([white], 16, 48000, 4096, 2), lambda d: True),
        "tie-lpc-fixed": (([np.array(TIE_FIXED)], 16, 48000, 48, 4), lambda d: d[0][1][0][:3] == ("fixed", 1, 0)),
        "tie-lpc-porder": (([np.array(TIE_P)], 16, 48000, 48, 4), lambda d: d[0][1][0][:3] == ("lpc", 2, 0)),
        "tie-lpc-order": (([np.array(TIE_O)], 16, 48000, 64, 4), lambda d: d[0][1][0][:3] == ("lpc", 1, 0)),
        # left = side >> 1, right = left - side: a legal 24-bit pair whose side channel is bound_side()
        "residual-bound": (([bound_side() >> 1, (bound_side() >> 1) - bound_side()], 24, 48000, 16384, 12),
                           lambda d: d[0][1][1][0] == "lpc" and d[0][1][1][1] < 5),
        "stereo-resonant": (([resonant(3000, 1), (resonant(3000, 1) * 3) // 4 + resonant(3000, 2, level=0.05)], 16, 44100, 1152, 8), lambda d: "lpc" in kinds(d)),
        "resonant-24bit": (([resonant(1500, 4, 24)], 24, 96000, 512, 12), lambda d: "lpc" in kinds(d)),
    }
