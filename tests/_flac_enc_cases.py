"""Inputs of the FLAC encoder's tests (tests/test_flac_enc_host.py, tests/test_gpu_flac_enc.py): the signals of the matrix and the
decision cases, each with what the restatement (tests/_flac_enc_ref.py) must decide for it.  A case is (channels as int64 arrays,
bits, rate, block)."""
import functools

import numpy as np

import _flac_ref as R

RATES = (44100, 12345, 96000, 352800, 100001)                               # table, Hz trailer, table, tens of Hz, from STREAMINFO
BLOCKS = (16, 64, 100, 192, 256, 576, 1000, 4096)


def lengths_of(block):
    return (1, 2, 4, 5, block - 1, block, block + 1, 3 * block + 5)


def tone(L, bits, seed, amp=0.3, noise=1):
    """A 997 Hz tone at 48 kHz with +-`noise` LSB of noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    return (np.round(amp * (1 << (bits - 1)) * np.sin(2 * np.pi * 997 * t / 48000 + seed)) + rng.integers(-noise, noise + 1, L)).astype(np.int64)


def full_noise(L, bits, seed):
    return np.random.default_rng(seed).integers(-(1 << (bits - 1)), 1 << (bits - 1), L).astype(np.int64)


def matrix_signal(C, bits, L, seed):
    """Channels of a different kind each, so that one stream of the matrix holds several subframe types: a tone with noise, DC,
    full-scale noise, a quiet tone ..."""
    kinds = (lambda c: tone(L, bits, seed + c), lambda c: np.full(L, 3 - 5 * c, dtype=np.int64), lambda c: full_noise(L, bits, seed + c),
             lambda c: tone(L, bits, seed + c, amp=0.01, noise=3))
    return [kinds[(c + seed) % 4](c) for c in range(C)]


def matrix_case(C, bits, block, L, index, rate=None):
    """`rate` None: the five rates in turn with the index (the device's sub-matrix; the host matrix crosses all five)."""
    return matrix_signal(C, bits, L, index % 7), bits, RATES[index % 5] if rate is None else rate, block


@functools.lru_cache(maxsize=None)
def decisions():
    """name -> (case, expect): expect(decisions of the restatement, one (assignment, [(kind, order, porder, ks)]) per frame) -> bool."""
    rng = np.random.default_rng(11)
    t1024 = tone(1024, 16, 1, amp=0.5)
    T = tone(4096, 16, 2, amp=0.4, noise=0)
    n1 = rng.integers(-40, 41, 4096).astype(np.int64)
    alt = np.where(np.arange(512) % 2 == 0, -(1 << 23), (1 << 23) - 1).astype(np.int64)
    env = np.repeat(2.0 ** rng.integers(1, 14, 256), 16)
    varying = np.round(env * rng.uniform(-1, 1, 4096)).astype(np.int64)
    kinds = lambda d: [s[0] for _, subs in d for s in subs]                 # noqa: E731
    tie_o = np.array([0, -2, 0, -2, -3, -2, -2, -4, -3, -4, -3, -5, -4, -2, -3, -5])
    tie_p = np.array([3, -3, -1, -3, 2, 0, -2, -3, 2, -2, 2, -1, 0, -3, 0, -3, -2, 3, 3, 0, 3, -2, 1, 1, 3, -3, 1, -2, -1, 3, 1, 3])
    tie_k = np.array([3, -2, -2, -1, -3, 3, 1, -2, 3, 0, -1, -3, 3, -1, -2, -3, -2, 2, -1, 3, -3, -3, 0, -1, -2, 3, -2, -3, -2, 2, 3, -3])
    spike = rng.integers(-1, 2, 65535).astype(np.int64)
    spike[30000] = 8388607
    tie_op = np.array([0, 0, -2, -1, 0, -1, 1, -1, -3, -4, -6, -6, -8, -6, -8, -10])
    return {
        # (0, 1) and (1, 0) cost the same and less than everything else: the smaller partition order goes first
        "tie-order-against-porder": (([tie_op], 16, 48000, 16), lambda d: d[0][1][0][:3] == ("fixed", 1, 0)),
        # a block that cannot be partitioned, quiet but for one full-scale sample: a unary run of more than 2^15 bits (the device
        # encoder's window of the bit stream holds 2^15)
        "long-unary-run": (([spike], 24, 48000, 65535), lambda d: d[0][1][0][:3] == ("fixed", 0, 0) and (2 * 8388607) >> d[0][1][0][3][0] > 1 << 15),
        "silence": (([np.zeros(300, dtype=np.int64)], 16, 48000, 256), lambda d: set(kinds(d)) == {"constant"}),
        "dc-24bit": (([np.full(100, -8388608, dtype=np.int64), np.full(100, 8388607, dtype=np.int64), np.full(100, 5, dtype=np.int64)], 24, 48000, 64),
                     lambda d: set(kinds(d)) == {"constant"}),
        "noise-verbatim": (([full_noise(1024, 16, 3)], 16, 48000, 1024), lambda d: kinds(d) == ["verbatim"]),
        "tone-fixed": (([t1024], 16, 48000, 1024), lambda d: kinds(d) == ["fixed"] and d[0][1][0][1] >= 2),
        "stereo-independent": (([full_noise(4096, 16, 8), full_noise(4096, 16, 9)], 16, 44100, 4096), lambda d: d[0][0] == 1),
        "stereo-equal-left-side": (([T, T.copy()], 16, 44100, 4096), lambda d: d[0][0] == R.LEFT_SIDE and d[0][1][1][0] == "constant"),
        "stereo-side-right": (([T + n1, T], 16, 44100, 4096), lambda d: d[0][0] == R.SIDE_RIGHT),
        "stereo-mid-side": (([T + n1, T - n1], 16, 44100, 4096), lambda d: d[0][0] == R.MID_SIDE),
        "alternating-24bit": (([alt, -1 - alt], 24, 96000, 512), lambda d: True),
        "alternating-24bit-mono": (([alt], 24, 96000, 512), lambda d: kinds(d) == ["verbatim"]),
        "porder-0": (([rng.integers(-20, 21, 4096).astype(np.int64)], 16, 48000, 4096), lambda d: d[0][1][0][:3] == ("fixed", 0, 0)),
        "porder-max": (([varying], 16, 48000, 4096), lambda d: d[0][1][0][0] == "fixed" and d[0][1][0][2] == 8),
        "tie-order": (([tie_o], 16, 48000, 16), lambda d: d[0][1][0][:3] == ("fixed", 0, 0)),
        "tie-porder": (([tie_p], 16, 48000, 32), lambda d: d[0][1][0][:3] == ("fixed", 0, 0)),
        "tie-k": (([tie_k], 16, 48000, 32), lambda d: d[0][1][0] == ("fixed", 0, 0, [1])),
        "five-frames-stereo": (([tone(5 * 4096 - 7, 16, 5), tone(5 * 4096 - 7, 16, 5, amp=0.31, noise=2)], 16, 48000, 4096), lambda d: len(d) == 5),
    }


# the candidates that must tie in the three tie cases: (name, the pairs (o, p) of equal, smallest bits)
TIES = {"tie-order": [(0, 0), (1, 0)], "tie-porder": [(0, 0), (0, 1)], "tie-order-against-porder": [(0, 1), (1, 0)]}
