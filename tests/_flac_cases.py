"""The FLAC fixtures of tests/test_flac_host.py and tests/test_gpu_flac.py: streams built by the restatement (_flac_ref.py), each
with the samples it must decode to.  Built once per process (lru_cache) and never changed."""
import functools
import math
import random

import _flac_ref as R

KINDS = ["constant", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4", "lpc1", "lpc2", "lpc12", "lpc32"]


def signal(T, bits, seed, amp=0.4):
    """A sine plus noise, inside `bits`."""
    rng = random.Random(seed)
    top = (1 << (bits - 1)) - 1
    noise = max(1, top >> 6)
    return [max(-top - 1, min(top, int(amp * top * math.sin(0.07 * n + seed) + rng.randint(-noise, noise)))) for n in range(T)]


def lpc_spec(order, seed, precision=12, shift=10, **more):
    rng = random.Random(seed)
    lim = (1 << (precision - 1)) - 1
    coefs = [rng.randint(-lim // max(order // 2, 1), lim // max(order // 2, 1)) for _ in range(order)]
    coefs[0] = lim if order == 1 else coefs[0]
    return dict(kind="lpc", coefs=coefs, precision=precision, shift=shift, **more)


def spec_of(kind, seed, **more):
    if kind in ("constant", "verbatim"):
        return dict(kind=kind)
    if kind.startswith("fixed"):
        return dict(kind="fixed", order=int(kind[5:]), **more)
    return lpc_spec(int(kind[3:]), seed, **more)


@functools.lru_cache(maxsize=None)
def matrix(nch, bits, block=48, last=40):
    """Every subframe kind in every channel: frame k codes channel c with KINDS[(k + c) % 11]; 4- and 5-bit Rice parameters and
    partition orders 0 .. 2 alternate; a short last frame.  -> (stream bytes, channels)."""
    nk = len(KINDS)
    T = nk * block + last
    chs = [signal(T, bits, 100 * bits + c, 0.25 + 0.05 * c) for c in range(nch)]
    for k in range(nk + 1):
        for c in range(nch):
            if KINDS[(k + c) % nk] == "constant":
                a, b = k * block, min(T, (k + 1) * block)
                chs[c][a:b] = [chs[c][a]] * (b - a)

    def specs(k, c):
        more = {} if KINDS[(k + c) % nk] in ("constant", "verbatim") else dict(method=(k + c) & 1, porder=0 if k == nk else (k + c) % 3 if KINDS[(k + c) % nk] != "lpc32" else 0)
        return spec_of(KINDS[(k + c) % nk], 7 * k + c, **more)
    data, _ = R.make_stream(chs, bits, block, specs=specs)
    return data, chs


@functools.lru_cache(maxsize=None)
def wide_sums():
    """Full-scale 24-bit samples of alternating sign under 32 precision-15 coefficients of alternating sign: every product has one
    sign, the prediction sum reaches 32 * 16383 * 8388607 ~ 2^42 and a 32-bit sum would wrap."""
    A = (1 << 23) - 1
    T = 96
    ch = [A if n % 2 == 0 else -A for n in range(T)]
    coefs = [16383 if i % 2 == 0 else -16383 for i in range(32)]
    spec = dict(kind="lpc", coefs=coefs, precision=15, shift=15, method=1)
    assert abs(sum(c * ch[40 - 1 - i] for i, c in enumerate(coefs))) > 1 << 41
    data, _ = R.make_stream([ch], 24, 48, specs=[spec])
    return data, [ch]


@functools.lru_cache(maxsize=None)
def rice_edges():
    """Rice parameter 0 and the largest of each width (14 and 30), and unary runs of more than 64 zeros (parameter 0 under residuals
    of several hundred) that cross 8-byte boundaries at every alignment."""
    rng = random.Random(5)
    T = 64 * 4
    ch = [rng.randint(-300, 300) for _ in range(T)]
    table = [dict(kind="fixed", order=0, method=0, porder=1, params=[0, 14]), dict(kind="fixed", order=0, method=1, porder=1, params=[30, 0]),
             dict(kind="fixed", order=1, method=0, porder=2, params=[0, 0, 0, 0]), dict(kind="fixed", order=0, method=1, porder=0, params=[0])]
    data, _ = R.make_stream([ch], 16, 64, specs=lambda k, c: table[k])
    return data, [ch]


@functools.lru_cache(maxsize=None)
def escapes(bits):
    """Escape partitions of raw width bits + 1 (steps of full scale under FIXED 1), 0 (a flat stretch), 1 (steps of 0 / -1) and the
    smallest that fits."""
    top = (1 << (bits - 1)) - 1
    rng = random.Random(bits)
    ch = [top if n % 2 == 0 else -top - 1 for n in range(16)]
    ch += [ch[-1]] * 16
    for _ in range(16):
        ch.append(ch[-1] - rng.randint(0, 1))
    ch += [rng.randint(-top // 3, top // 3) for _ in range(16)]
    spec = dict(kind="fixed", order=1, porder=2, escapes={0: bits + 1, 1: 0, 2: 1, 3: None})
    data, _ = R.make_stream([ch], bits, 64, specs=[spec])
    return data, [ch]


@functools.lru_cache(maxsize=None)
def wasted(bits):
    """Wasted bits of 1 and of bits - 1, under VERBATIM, FIXED and CONSTANT."""
    rng = random.Random(bits + 50)
    top = (1 << (bits - 1)) - 1
    a = [2 * rng.randint(-top // 2, top // 2) for _ in range(32)]
    b = [rng.choice((0, -(1 << (bits - 1)))) for _ in range(32)]
    chs = [a + b + [b[0]] * 32, b + a + [2 * 5] * 32]
    table = {(0, 0): dict(kind="verbatim", wasted=1), (0, 1): dict(kind="fixed", order=1, wasted=bits - 1), (1, 0): dict(kind="verbatim", wasted=bits - 1),
             (1, 1): dict(kind="fixed", order=2, wasted=1), (2, 0): dict(kind="constant", wasted=bits - 1 if b[0] else 0), (2, 1): dict(kind="constant", wasted=1)}
    data, _ = R.make_stream(chs, bits, 32, specs=lambda k, c: table[(k, c)])
    return data, chs


@functools.lru_cache(maxsize=None)
def stereo(bits, assign):
    """Left at the top and right at the bottom of the range: the side channel needs bits + 1, and is odd."""
    top = (1 << (bits - 1)) - 1
    rng = random.Random(assign)
    left = [top, top, -top - 1, 3] + [rng.randint(-top - 1, top) for _ in range(44)]
    right = [-top - 1, -top, top, 0] + [rng.randint(-top - 1, top) for _ in range(44)]
    assert (left[0] - right[0]) % 2 == 1 and left[0] - right[0] == (1 << bits) - 1
    specs = lambda k, c: [dict(kind="verbatim"), dict(kind="fixed", order=1)][(k + c) % 2]
    data, _ = R.make_stream([left, right], bits, 16, assign=assign, specs=specs)
    return data, [left, right]


BLOCK_SIZES = [192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 17, 300, 1, 2]


@functools.lru_cache(maxsize=None)
def block_codes():
    """Variable block size: every block-size code once (the table's codes, the 8- and the 16-bit trailer), frames of 1 to 32768
    samples in one stream, CONSTANT subframes in the long frames."""
    chs, specs = [[], []], []
    for k, bs in enumerate(BLOCK_SIZES):
        if bs <= 300:
            chs[0] += signal(bs, 16, k)
            chs[1] += signal(bs, 16, k + 1)
            specs.append([dict(kind="verbatim"), dict(kind="fixed", order=min(2, bs - 1) if bs > 1 else 0)])
        else:
            chs[0] += [37 * k - 200] * bs
            chs[1] += [-k] * bs
            specs.append([dict(kind="constant"), dict(kind="constant")])
    data, _ = R.make_stream(chs, 16, None, variable=True, sizes=list(BLOCK_SIZES), specs=lambda k, c: specs[k][c])
    return data, chs


@functools.lru_cache(maxsize=None)
def variable_small():
    """Variable block size with frames of 1 to 4608 samples in one stream, Rice coded where short."""
    sizes = [1, 2, 16, 17, 255, 256, 257, 4608, 33, 4096, 5]
    chs, specs = [[]], []
    for k, bs in enumerate(sizes):
        if bs <= 300:
            chs[0] += signal(bs, 16, k)
            specs.append(dict(kind="fixed", order=min(bs - 1, k % 5)))
        else:
            chs[0] += signal(bs, 16, k)
            specs.append(dict(kind="verbatim"))
    data, _ = R.make_stream(chs, 16, None, variable=True, sizes=sizes, specs=lambda k, c: specs[k], first_number=(1 << 31) - 300)
    return data, chs


@functools.lru_cache(maxsize=None)
def long_blocks(block):
    """Three frames of `block` (4096 / 4608) samples, FIXED and LPC, Rice coded."""
    ch = signal(3 * block, 16, block, 0.5)
    table = [dict(kind="fixed", order=2, porder=3), lpc_spec(8, 3, porder=4, method=1), dict(kind="fixed", order=4, porder=0)]
    data, _ = R.make_stream([ch], 16, block, specs=lambda k, c: table[k])
    return data, [ch]


RATES = [(88200, None), (176400, None), (192000, None), (8000, None), (16000, None), (22050, None), (24000, None), (32000, None), (44100, None),
         (48000, None), (96000, None), (48000, 12), (44100, 13), (44100, 14), (11025, 0), (655350, 14)]


@functools.lru_cache(maxsize=None)
def rate_code(rate, code):
    ch = signal(40, 16, rate % 97)
    data, _ = R.make_stream([ch], 16, 16, rate=rate, rate_code=code, bits_code=0 if code == 0 else None)
    return data, [ch]


NUMBERS = [(False, 0), (False, 126), (False, 2046), (False, 65534), (False, (1 << 21) - 2), (False, (1 << 26) - 2), (False, (1 << 31) - 3),
           (True, (1 << 31) - 20), (True, (1 << 35) + 5), (True, (1 << 36) - 48)]


@functools.lru_cache(maxsize=None)
def numbers(variable, first):
    """Coded frame / sample numbers of 1 to 7 bytes: three frames whose numbers cross a length boundary."""
    ch = signal(48, 16, first % 89)
    data, _ = R.make_stream([ch], 16, 16, variable=variable, first_number=first)
    return data, [ch]


@functools.lru_cache(maxsize=None)
def with_metadata(id3=None, footer=False):
    ch = signal(70, 16, 9)
    data, _ = R.make_stream([ch, ch[::-1]], 16, 32, blocks=R.every_metadata_kind(), id3=None if id3 is None else R.id3v2(id3, footer))
    return data, [ch, ch[::-1]]


def all_cases():
    """name -> builder of (bytes, channels): every construct of the subset at least once."""
    cases = {}
    for nch in (1, 2, 3, 8):
        for bits in (8, 12, 16, 20, 24):
            cases["matrix-%dch-%dbit" % (nch, bits)] = functools.partial(matrix, nch, bits)
    cases["wide-sums"] = wide_sums
    cases["rice-edges"] = rice_edges
    for bits in (8, 12, 16, 20, 24):
        cases["escapes-%dbit" % bits] = functools.partial(escapes, bits)
        cases["wasted-%dbit" % bits] = functools.partial(wasted, bits)
        for assign in (R.LEFT_SIDE, R.SIDE_RIGHT, R.MID_SIDE):
            cases["stereo-%dbit-%d" % (bits, assign)] = functools.partial(stereo, bits, assign)
    cases["block-codes"] = block_codes
    cases["variable-small"] = variable_small
    cases["long-4096"] = functools.partial(long_blocks, 4096)
    cases["long-4608"] = functools.partial(long_blocks, 4608)
    for rate, code in RATES:
        cases["rate-%d-%s" % (rate, code)] = functools.partial(rate_code, rate, code)
    for variable, first in NUMBERS:
        cases["number-%s-%d" % ("v" if variable else "f", first)] = functools.partial(numbers, variable, first)
    cases["metadata"] = with_metadata
    cases["metadata-id3"] = functools.partial(with_metadata, 37)
    cases["metadata-id3-footer"] = functools.partial(with_metadata, 300, True)
    return cases
