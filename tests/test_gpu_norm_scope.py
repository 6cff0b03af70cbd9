"""The kernels of norm_scope='clip' on the GPU (csrc/spectro.hip: p2phd_spectro_range, p2phd_range_fold,
p2phd_spectro_encode_given) against the encode they extend, p2phd_spectro_encode_ex, bit for bit: the range and the noise
range against that entry's statistics, the fold, the encode under the tensor's own range, the property the feature rests on
-- a batch encoded alone under the range of a larger batch carries the larger batch's rows --, a range of zero, refusals,
canaries and the launch counter."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(B, F, M, C) for B in (1, 3) for F in (9, 40) for M in (64, 80) for C in (1, 2)]   # F: a partial tile / a full and a partial one
ALPHA = 0.6
MIN_VALUE = 1e-7
GUARD = 1024                                                       # floats on either side of an output
GUARD_BITS = 0x7FC0BEEF                                            # a NaN pattern no kernel writes
MODES = (None, 0, 1, 2)                                            # mask modes: None = mask rows without noise (zeros)
INF = float('inf')


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib, _lib.lib()


def _count(reset=False):
    return _L()[1].p2phd_launch_count(b"normscope", 1 if reset else 0)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.int32)


def _mask_rows(M):
    return M // 3                                                  # 21 and 26: neither a multiple of the tile nor of 8


def _spec_host(B, F, M, seed, scale=1.0):
    """Random spectra over six decades, both signs, exact zeros."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, F, M)) * 10.0 ** rng.uniform(-5, 1, (B, F, M))).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = 0.0
    assert (x > 0).any() and (x < 0).any() and (x == 0).any()
    return (np.float32(scale) * x).astype(np.float32)


_OPERANDS = {}


def _operands(B, F, M, C):
    """(spec, noise, noise_sign) on the GPU for a shape; made once."""
    key = (B, F, M, C)
    if key not in _OPERANDS:
        rng = np.random.default_rng(77 + 1000 * B + 100 * F + M + C)
        R = _mask_rows(M)
        noise = rng.standard_normal((B, C, R, F)).astype(np.float32)
        sign = (2.0 * rng.integers(0, 2, noise.shape) - 1.0).astype(np.float32)
        _OPERANDS[key] = tuple(torch.from_numpy(a).to(DEV) for a in (_spec_host(B, F, M, 10 * B + F + M + C), noise, sign))
    return _OPERANDS[key]


def _guarded(n):
    """-> (the whole buffer, its n floats between two guard regions)."""
    buf = torch.full((GUARD + n + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    bits = buf.view(torch.int32).cpu().numpy()
    return bool((bits[:GUARD] == GUARD_BITS).all() and (bits[GUARD + n:] == GUARD_BITS).all())


def _partials(B, F, M):
    _lib, L = _L()
    return torch.empty(max(L.p2phd_spectro_partials_floats(B, F, M), 4096), dtype=torch.float32, device=DEV)


_EX = {}


def _encode_ex(spec, C, rows=0, mode=None, noise=None, sign=None, key=None):
    """p2phd_spectro_encode_ex -> (log_spectro, pha, norm8) on the GPU; kept under `key`."""
    if key is not None and key in _EX:
        return _EX[key]
    _lib, L = _L()
    B, F, M = spec.shape
    log = torch.empty((B, C, M, F), dtype=torch.float32, device=DEV)
    pha = torch.empty((B, 1, M, F), dtype=torch.float32, device=DEV)
    norm8 = torch.zeros(8, dtype=torch.float32, device=DEV)
    _lib.check(L.p2phd_spectro_encode_ex(_lib.ptr(spec), B, F, M, C, ALPHA, MIN_VALUE, rows, 2 if mode is None else mode,
                                         _lib.ptr(None if mode is None else noise), _lib.ptr(sign if mode == 1 else None), _lib.ptr(log),
                                         _lib.ptr(pha), _lib.ptr(norm8), _lib.ptr(_partials(B, F, M)), _lib.stream_ptr()), "encode_ex")
    res = (log, pha, norm8)
    if key is not None:
        _EX[key] = res
    return res


def _given_rc(spec, C, norm8, rows=0, mode=None, noise=None, sign=None, nb=None):
    """p2phd_spectro_encode_given with both outputs between guard regions -> (rc, log_spectro, pha, guards intact)."""
    _lib, L = _L()
    B, F, M = spec.shape
    nb = B if nb is None else nb
    n_log, n_pha = nb * C * M * F, nb * M * F
    (lbuf, log), (pbuf, pha) = _guarded(n_log), _guarded(n_pha)
    before = None if norm8 is None else _bits(norm8).copy()
    rc = L.p2phd_spectro_encode_given(_lib.ptr(spec), nb, F, M, C, ALPHA, MIN_VALUE, rows, 2 if mode is None else mode,
                                      _lib.ptr(None if mode is None else noise), _lib.ptr(sign if mode == 1 else None), _lib.ptr(norm8),
                                      _lib.ptr(log), _lib.ptr(pha), _lib.stream_ptr())
    intact = _intact(lbuf, n_log) and _intact(pbuf, n_pha)
    if before is not None:
        intact = intact and np.array_equal(_bits(norm8), before)   # the entry writes nothing into norm8
    return rc, log.reshape(nb, C, M, F), pha.reshape(nb, 1, M, F), intact


def _given(*a, **kw):
    rc, log, pha, intact = _given_rc(*a, **kw)
    assert rc == 0 and intact, (rc, intact)
    assert not (_bits(log) == GUARD_BITS).any() and not (_bits(pha) == GUARD_BITS).any()      # every element was written
    return log, pha


def _acc(mn=INF, mx=-INF):
    """An accumulator of two floats between guard regions -> (buffer, the two floats)."""
    buf, mm = _guarded(2)
    mm.copy_(torch.tensor([mn, mx], dtype=torch.float32))
    return buf, mm


def _range(spec, C, acc=None):
    _lib, L = _L()
    B, F, M = spec.shape
    buf, mm = _acc() if acc is None else acc
    _lib.check(L.p2phd_spectro_range(_lib.ptr(spec), B, F, M, C, ALPHA, MIN_VALUE, _lib.ptr(mm), _lib.ptr(_partials(B, F, M)),
                                     _lib.stream_ptr()), "spectro_range")
    assert _intact(buf, 2)
    return mm


def _fold(x, acc=None):
    _lib, L = _L()
    buf, mm = _acc() if acc is None else acc
    _lib.check(L.p2phd_range_fold(_lib.ptr(x), x.numel(), _lib.ptr(mm), _lib.ptr(_partials(1, 1, 1)), _lib.stream_ptr()), "range_fold")
    assert _intact(buf, 2)
    return mm


# ------------------------------------------------------------------------------------------
# 1. the range against the encode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,M,C", SHAPES)
def test_range_equals_the_statistics_of_the_encode(B, F, M, C):
    spec, noise, sign = _operands(B, F, M, C)
    _, _, norm8 = _encode_ex(spec, C, _mask_rows(M), 2, noise, key=(B, F, M, C, 2))
    assert np.array_equal(_bits(_range(spec, C)), _bits(norm8[0:2]))
    assert np.array_equal(_bits(_fold(noise)), _bits(norm8[4:6]))
    # a tensor that starts 4 bytes off a 16-byte boundary takes the one-by-one path: the same two floats
    flat = torch.empty(spec.numel() + 1, dtype=torch.float32, device=DEV)
    off = flat[1:].view(spec.shape)
    off.copy_(spec)
    assert off.data_ptr() % 16 == 4
    assert np.array_equal(_bits(_range(off, C)), _bits(norm8[0:2]))
    flat = torch.empty(noise.numel() + 1, dtype=torch.float32, device=DEV)
    flat[1:].copy_(noise.reshape(-1))
    assert np.array_equal(_bits(_fold(flat[1:])), _bits(norm8[4:6]))


# ------------------------------------------------------------------------------------------
# 2. the fold
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,M,C", SHAPES)
def test_fold_behaviour(B, F, M, C):
    spec, noise, _ = _operands(B, F, M, C)
    quiet = (spec * 1e-3).contiguous()
    a, b = _range(spec, C).cpu().numpy(), _range(quiet, C).cpu().numpy()
    assert not np.array_equal(a, b)
    want = np.array([min(a[0], b[0]), max(a[1], b[1])], dtype=np.float32)
    for first, second in ((spec, quiet), (quiet, spec)):
        acc = _acc()
        _range(first, C, acc)
        assert np.array_equal(_bits(_range(second, C, acc)), _bits(want))
    # the pieces of a tensor, one call per row: the tensor's range
    acc = _acc()
    for i in range(B):
        _range(spec[i:i + 1], C, acc)
    assert np.array_equal(_bits(acc[1]), _bits(a))
    # an accumulator that is already wider is left as it is
    wide = np.array([-1000.0, 1000.0], dtype=np.float32)
    assert np.array_equal(_bits(_range(spec, C, _acc(-1000.0, 1000.0))), _bits(wide))
    assert np.array_equal(_bits(_fold(noise, _acc(-1000.0, 1000.0))), _bits(wide))
    na, nb = _fold(noise).cpu().numpy(), _fold(3 * noise + 1).cpu().numpy()
    acc = _acc()
    _fold(3 * noise + 1, acc)
    assert np.array_equal(_bits(_fold(noise, acc)), _bits(np.array([min(na[0], nb[0]), max(na[1], nb[1])], dtype=np.float32)))
    # NaN entries: what the encode gives on the same tensor
    holes = spec.clone()
    holes.view(-1)[::7] = float('nan')
    _, _, norm8 = _encode_ex(holes, C)
    got = _range(holes, C)
    assert np.isfinite(got.cpu().numpy()).all()
    assert np.array_equal(_bits(got), _bits(norm8[0:2]))
    nz = noise.clone()
    nz.view(-1)[::5] = float('nan')
    _, _, norm8 = _encode_ex(spec, C, _mask_rows(M), 2, nz)
    assert np.array_equal(_bits(_fold(nz)), _bits(norm8[4:6]))


# ------------------------------------------------------------------------------------------
# 3. the given range equal to the tensor's own
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,M,C", SHAPES)
def test_given_own_range_is_the_encode(B, F, M, C):
    spec, noise, sign = _operands(B, F, M, C)
    R = _mask_rows(M)
    for mode in MODES:
        want_log, want_pha, norm8 = _encode_ex(spec, C, R, mode, noise, sign, key=(B, F, M, C, mode))
        assert np.isfinite(want_log.cpu().numpy()).all()
        given = norm8.clone()
        given[2:4] = float('nan')                                  # mean and std are not read
        if mode is None:
            given[4:] = float('nan')                               # nor the noise range without noise rows
        log, pha = _given(spec, C, given, R, mode, noise, sign)
        assert np.array_equal(_bits(log), _bits(want_log)), mode
        assert np.array_equal(_bits(pha), _bits(want_pha)), mode
    # no mask rows: the noise range is not read
    want_log, want_pha, norm8 = _encode_ex(spec, C, 0, 2, None, key=(B, F, M, C, 'plain'))
    given = norm8.clone()
    given[2:] = float('nan')
    log, pha = _given(spec, C, given, 0, 2, noise)
    assert np.array_equal(_bits(log), _bits(want_log)) and np.array_equal(_bits(pha), _bits(want_pha))
    assert float(want_log.min()) == 0.0 and abs(float(want_log.max()) - 1.0) <= 2.0 ** -23


# ------------------------------------------------------------------------------------------
# 4. the property itself
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,M,C", SHAPES)
def test_rows_alone_under_the_range_of_the_batch_are_the_rows_of_the_batch(B, F, M, C):
    """[x, y] with y 100 times louder: x encoded alone under the range of [x, y] is rows 0:B of the encode of [x, y], bit for bit.
    The noise statistics have to agree between the two calls.  With noise of all zeros they do, but the encode divides by their
    range of zero and leaves NaN in the noise rows where the new entry leaves 0: there the rows below the noise are compared and
    the noise rows are asserted to be NaN and 0.  With a second noise -- the same rows for x and for y, so that the batch's
    statistics are those of x's rows alone -- every row is compared."""
    x, noise, sign = _operands(B, F, M, C)
    both = torch.cat([x, 100.0 * x])
    R = _mask_rows(M)
    keep = M - R
    acc = _acc()
    _range(x, C, acc)
    _range(both[B:], C, acc)
    # all-zero noise
    zeros = torch.zeros((2 * B, C, R, F), dtype=torch.float32, device=DEV)
    want_log, want_pha, norm8 = _encode_ex(both, C, R, 2, zeros)
    assert np.array_equal(_bits(acc[1]), _bits(norm8[0:2]))
    assert float(norm8[4]) == 0.0 and float(norm8[5]) == 0.0
    log, pha = _given(x, C, norm8, R, 2, zeros[:B])
    assert np.array_equal(_bits(log[:, :, :keep]), _bits(want_log[:B, :, :keep]))
    assert np.array_equal(_bits(pha), _bits(want_pha[:B]))
    assert torch.isnan(want_log[:, :, keep:]).all() and (log[:, :, keep:] == 0).all()
    own, _ = _given(x, C, _encode_ex(x, C)[2], R, None)
    assert not np.array_equal(_bits(own[:, :, :keep]), _bits(log[:, :, :keep]))             # (the range matters)
    # noise whose statistics agree without being degenerate, every mask mode
    for mode in (0, 1, 2):
        n2, s2 = torch.cat([noise, noise]), torch.cat([sign, sign])
        want_log, want_pha, norm8 = _encode_ex(both, C, R, mode, n2, s2)
        given = torch.zeros(8, dtype=torch.float32, device=DEV)
        given[0:2] = acc[1]
        nacc = _acc()
        _fold(noise, nacc)
        given[4:6] = nacc[1]
        log, pha = _given(x, C, given, R, mode, noise, sign)
        assert np.isfinite(want_log.cpu().numpy()).all()
        assert np.array_equal(_bits(log), _bits(want_log[:B])), mode
        assert np.array_equal(_bits(pha), _bits(want_pha[:B])), mode


# ------------------------------------------------------------------------------------------
# 5. a range of zero
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,F,M,C", SHAPES)
def test_zero_range_gives_zeros(B, F, M, C):
    spec = torch.zeros((B, F, M), dtype=torch.float32, device=DEV)
    mm = _range(spec, C).cpu().numpy()
    d = np.float32(20) * np.log10(np.float32(MIN_VALUE)) - np.float32(20)
    assert mm[0] == mm[1] and abs(float(mm[0]) - float(d)) < 1e-3
    norm8 = torch.full((8,), float(mm[0]), dtype=torch.float32, device=DEV)
    R = _mask_rows(M)
    noise = torch.full((B, C, R, F), 0.25, dtype=torch.float32, device=DEV)               # a noise range of zero as well
    norm8[4:6] = 0.25
    for rows, mode in ((0, None), (R, None), (R, 0), (R, 2)):
        log, pha = _given(spec, C, norm8, rows, mode, noise)
        assert torch.isfinite(log).all() and (log == 0).all() and (pha == 0).all()


def test_zero_range_is_nan_in_the_encode_this_extends():
    """The reason for the feature: the encode divides by max - min."""
    B, F, M, C = 1, 9, 64, 2
    log, pha, norm8 = _encode_ex(torch.zeros((B, F, M), dtype=torch.float32, device=DEV), C)
    assert float(norm8[0]) == float(norm8[1])
    assert torch.isnan(log).all() and (pha == 0).all()


# ------------------------------------------------------------------------------------------
# 6. refusals and bookkeeping
# ------------------------------------------------------------------------------------------
def test_empty_batch_bad_arguments_and_the_counter():
    _lib, L = _L()
    B, F, M, C = 3, 9, 80, 2
    spec, noise, sign = _operands(B, F, M, C)
    R = _mask_rows(M)
    _, _, norm8 = _encode_ex(spec, C, R, 2, noise, key=(B, F, M, C, 2))
    part = _partials(B, F, M)
    # the counter: one per call that launches
    _count(reset=True)
    _range(spec, C)
    assert _count() == 1
    _fold(noise)
    assert _count() == 2
    _given(spec, C, norm8, R, 2, noise)
    assert _count() == 3
    # B = 0 and n = 0 launch and write nothing
    rc, log, pha, intact = _given_rc(spec, C, norm8, R, 2, noise, nb=0)
    assert rc == 0 and intact and log.numel() == 0
    one = torch.full((C * M * F,), GUARD_BITS, dtype=torch.int32, device=DEV)
    assert L.p2phd_spectro_encode_given(_lib.ptr(spec), 0, F, M, C, ALPHA, MIN_VALUE, R, 2, _lib.ptr(noise), None, _lib.ptr(norm8),
                                        _lib.ptr(one), _lib.ptr(one), _lib.stream_ptr()) == 0
    assert bool((one == GUARD_BITS).all())
    buf, mm = _acc(1.0, 2.0)
    assert L.p2phd_spectro_range(_lib.ptr(spec), 0, F, M, C, ALPHA, MIN_VALUE, _lib.ptr(mm), _lib.ptr(part), _lib.stream_ptr()) == 0
    assert L.p2phd_range_fold(_lib.ptr(noise), 0, _lib.ptr(mm), _lib.ptr(part), _lib.stream_ptr()) == 0
    assert _intact(buf, 2) and mm.tolist() == [1.0, 2.0]
    assert _count() == 3
    # refusals: the entry's name in the text, nothing written, nothing counted
    einval = L.p2phd_spectro_decode_signed(_lib.ptr(spec), _lib.ptr(spec), _lib.ptr(norm8), B, F, M, 3, 0, MIN_VALUE, 1.0, _lib.ptr(spec),
                                           _lib.stream_ptr())
    assert einval != 0

    def refused(rc, name, word):
        text = L.p2phd_last_error().decode()
        assert rc == einval and name in text and word in text, (rc, text)

    for ch in (0, 3):
        (lbuf, lg), (pbuf, ph) = _guarded(B * C * M * F), _guarded(B * M * F)
        refused(L.p2phd_spectro_encode_given(_lib.ptr(spec), B, F, M, ch, ALPHA, MIN_VALUE, R, 2, _lib.ptr(noise), None, _lib.ptr(norm8),
                                             _lib.ptr(lg), _lib.ptr(ph), _lib.stream_ptr()), "spectro_encode_given", "channels")
        assert (_bits(lg) == GUARD_BITS).all() and (_bits(ph) == GUARD_BITS).all() and _intact(lbuf, lg.numel()) and _intact(pbuf, ph.numel())
        refused(L.p2phd_spectro_range(_lib.ptr(spec), B, F, M, ch, ALPHA, MIN_VALUE, _lib.ptr(mm), _lib.ptr(part), _lib.stream_ptr()),
                "spectro_range", "channels")
    for rows in (-1, M + 1):
        rc, log, pha, intact = _given_rc(spec, C, norm8, rows, 2, noise)
        refused(rc, "spectro_encode_given", "mask_rows")
        assert intact and (_bits(log) == GUARD_BITS).all() and (_bits(pha) == GUARD_BITS).all()
    for mode in (-1, 3):
        rc, log, pha, intact = _given_rc(spec, C, norm8, R, mode, noise)
        refused(rc, "spectro_encode_given", "mask_mode")
        assert intact and (_bits(log) == GUARD_BITS).all() and (_bits(pha) == GUARD_BITS).all()
    rc, log, pha, intact = _given_rc(spec, C, norm8, R, 1, noise, None)                       # mode1 without its signs
    refused(rc, "spectro_encode_given", "sign")
    assert intact and (_bits(log) == GUARD_BITS).all()
    rc, log, pha, intact = _given_rc(spec, C, None, R, 2, noise)
    refused(rc, "spectro_encode_given", "null pointer")
    assert intact and (_bits(log) == GUARD_BITS).all()
    refused(L.p2phd_spectro_encode_given(None, B, F, M, C, ALPHA, MIN_VALUE, R, 2, _lib.ptr(noise), None, _lib.ptr(norm8), _lib.ptr(one),
                                         _lib.ptr(one), _lib.stream_ptr()), "spectro_encode_given", "null pointer")
    assert bool((one == GUARD_BITS).all())
    refused(L.p2phd_spectro_range(None, B, F, M, C, ALPHA, MIN_VALUE, _lib.ptr(mm), _lib.ptr(part), _lib.stream_ptr()), "spectro_range", "null pointer")
    refused(L.p2phd_spectro_range(_lib.ptr(spec), B, F, M, C, ALPHA, MIN_VALUE, None, _lib.ptr(part), _lib.stream_ptr()), "spectro_range", "null pointer")
    refused(L.p2phd_spectro_range(_lib.ptr(spec), B, F, M, C, ALPHA, MIN_VALUE, _lib.ptr(mm), None, _lib.stream_ptr()), "spectro_range", "null pointer")
    refused(L.p2phd_spectro_range(_lib.ptr(spec), B, 0, M, C, ALPHA, MIN_VALUE, _lib.ptr(mm), _lib.ptr(part), _lib.stream_ptr()), "spectro_range", "geometry")
    refused(L.p2phd_range_fold(None, 5, _lib.ptr(mm), _lib.ptr(part), _lib.stream_ptr()), "range_fold", "null pointer")
    refused(L.p2phd_range_fold(_lib.ptr(noise), 5, None, _lib.ptr(part), _lib.stream_ptr()), "range_fold", "null pointer")
    refused(L.p2phd_range_fold(_lib.ptr(noise), -1, _lib.ptr(mm), _lib.ptr(part), _lib.stream_ptr()), "range_fold", "length")
    assert _intact(buf, 2) and mm.tolist() == [1.0, 2.0]
    assert _count() == 3
    with pytest.raises(_lib.P2PHDError, match=r"spectro_encode_given.*mask_mode"):
        _lib.check(L.p2phd_spectro_encode_given(_lib.ptr(spec), B, F, M, C, ALPHA, MIN_VALUE, R, 7, _lib.ptr(noise), None, _lib.ptr(norm8),
                                                _lib.ptr(one), _lib.ptr(one), _lib.stream_ptr()), "spectro_encode_given")
