"""The kernels of segment_norm on the GPU (csrc/spectro.hip: p2phd_spectro_encode_rows, p2phd_spectro_decode_signed_rows,
p2phd_spectro_decode_spliced_rows), bit for bit against the entries they extend applied to one row at a time: row b of the row
encode is p2phd_spectro_encode_ex on spec[b:b + 1] -- statistics, log_spectro and pha --, and p2phd_spectro_encode_given under
that row's statistics; a row of digital silence is zeros where that entry leaves non-finite values; row b of a row decode is the
plain decode of that row under its (min, max).  Outputs lie between canaries, the workspace is poisoned and has exactly the
queried size."""
import numpy as np
import pytest
import torch

from test_gpu_norm_scope import (ALPHA, DEV, GUARD_BITS, MIN_VALUE, _bits, _encode_ex, _given, _guarded, _intact, _spec_host)

pytestmark = pytest.mark.gpu

GEOMETRIES = [(9, 64), (40, 80), (9, 33)]                          # (F, M); F * M = 297: rows 1, 2, ... start off a 16-byte boundary
SHAPES = [(B, F, M, C) for B in (1, 3) for (F, M) in GEOMETRIES for C in (1, 2)]
MODES = (None, 0, 1, 2)                                            # mask modes: None = mask rows without noise (zeros)
INF = float('inf')


def _L():
    from pix2pixhdaudiosr_amd import _lib
    return _lib, _lib.lib()


def _count(family=b"normrows", reset=False):
    return _L()[1].p2phd_launch_count(family, 1 if reset else 0)


def _mask_rows(M):
    return M // 3                                                  # 21, 26 and 11: no multiple of the tile; 11 * 9 * C: odd noise rows


_OPERANDS = {}


def _operands(B, F, M, C):
    """(spec, noise, noise_sign) on the GPU for a shape, every row at a level of its own; made once and left unchanged."""
    key = (B, F, M, C)
    if key not in _OPERANDS:
        rng = np.random.default_rng(99 + 1000 * B + 100 * F + M + C)
        R = _mask_rows(M)
        spec = np.concatenate([_spec_host(1, F, M, 10 * B + F + M + C + 7 * b, scale=10.0 ** -(b % 4)) for b in range(B)])
        noise = (rng.standard_normal((B, C, R, F)) * (1.0 + np.arange(B))[:, None, None, None]).astype(np.float32)
        sign = (2.0 * rng.integers(0, 2, noise.shape) - 1.0).astype(np.float32)
        _OPERANDS[key] = tuple(torch.from_numpy(a).to(DEV) for a in (spec, noise, sign))
    return _OPERANDS[key]


def _workspace(B, F, M):
    """The workspace at exactly the queried size, poisoned, between canaries -> (buffer, the floats, their count)."""
    n = _L()[1].p2phd_spectro_rows_partials_floats(B, F, M)
    assert n >= 4 * B
    buf, ws = _guarded(n)
    return buf, ws, n


def _rows_rc(spec, C, rows=0, mode=None, noise=None, sign=None, nb=None, ws=None, stream=None, norm_null=False, channels=None):
    """p2phd_spectro_encode_rows with every output between canaries -> (rc, log_spectro, pha, norm_rows, canaries intact)."""
    _lib, L = _L()
    B, F, M = spec.shape
    nb = B if nb is None else nb
    n_log, n_pha = nb * C * M * F, nb * M * F
    (lbuf, log), (pbuf, pha), (nbuf, norm) = _guarded(n_log), _guarded(n_pha), _guarded(8 * nb)
    wbuf, wsp, n_ws = _workspace(nb, F, M) if ws is None else ws
    rc = L.p2phd_spectro_encode_rows(_lib.ptr(spec), nb, F, M, C if channels is None else channels, ALPHA, MIN_VALUE, rows,
                                     2 if mode is None else mode, _lib.ptr(None if mode is None else noise),
                                     _lib.ptr(sign if mode == 1 else None), None if norm_null else _lib.ptr(norm), _lib.ptr(log),
                                     _lib.ptr(pha), _lib.ptr(wsp), _lib.stream_ptr() if stream is None else stream)
    torch.cuda.synchronize()
    intact = _intact(lbuf, n_log) and _intact(pbuf, n_pha) and _intact(nbuf, 8 * nb) and _intact(wbuf, n_ws)
    return rc, log.reshape(nb, C, M, F), pha.reshape(nb, 1, M, F), norm.reshape(nb, 8), intact


def _rows(*a, **kw):
    rc, log, pha, norm, intact = _rows_rc(*a, **kw)
    assert rc == 0 and intact, (rc, intact)
    for t in (log, pha, norm):
        assert not (_bits(t) == GUARD_BITS).any()                  # every element was written
    assert (_bits(norm[:, [2, 3, 6, 7]]) == 0).all()               # the entries that are not computed: +0
    return log, pha, norm


def _solo(spec, b, C, rows, mode, noise, sign):
    """p2phd_spectro_encode_ex on row b alone -> (log_spectro, pha, norm8)."""
    return _encode_ex(spec[b:b + 1], C, rows, mode, None if noise is None else noise[b:b + 1], None if sign is None else sign[b:b + 1])


def _assert_row_is_solo(log, pha, norm, b, solo, mode, rows, what=""):
    want_log, want_pha, norm8 = solo
    assert np.array_equal(_bits(log[b]), _bits(want_log[0])), (what, b, mode)
    assert np.array_equal(_bits(pha[b]), _bits(want_pha[0])), (what, b, mode)
    assert np.array_equal(_bits(norm[b, 0:2]), _bits(norm8[0:2])), (what, b, mode)
    if mode is not None and rows > 0:
        assert np.array_equal(_bits(norm[b, 4:6]), _bits(norm8[4:6])), (what, b, mode)
    else:                                                          # (that entry leaves its noise statistics untouched without noise)
        assert norm[b, 4:6].tolist() == [INF, -INF], (what, b, mode)


# ------------------------------------------------------------------------------------------
# 1. every row is its solo encode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=lambda m: "mode%s" % m)
@pytest.mark.parametrize("B,F,M,C", SHAPES)
def test_every_row_is_its_solo_encode(B, F, M, C, mode):
    spec, noise, sign = _operands(B, F, M, C)
    R = _mask_rows(M)
    log, pha, norm = _rows(spec, C, R, mode, noise, sign)
    # the same call on a tensor that starts 4 bytes off a 16-byte boundary: the one-by-one path where the other took quads
    flat = torch.empty(spec.numel() + 1, dtype=torch.float32, device=DEV)
    off = flat[1:].view(spec.shape)
    off.copy_(spec)
    assert off.data_ptr() % 16 == 4
    log_o, pha_o, norm_o = _rows(off, C, R, mode, noise, sign)
    for got, want in ((log_o, log), (pha_o, pha), (norm_o, norm)):
        assert np.array_equal(_bits(got), _bits(want))
    if (F * M) % 4 and B > 1:                                      # row 0 on a 16-byte boundary, the rows behind it off it
        assert spec[0].data_ptr() % 16 == 0 and spec[1].data_ptr() % 16 != 0 and spec[2].data_ptr() % 16 != 0
    for b in range(B):
        solo = _solo(spec, b, C, R, mode, noise, sign)
        assert np.isfinite(solo[0].cpu().numpy()).all()
        _assert_row_is_solo(log, pha, norm, b, solo, mode, R)
        # and the encode under a given range, given that row's statistics
        glog, gpha = _given(spec[b:b + 1], C, norm[b].clone(), R, mode, noise[b:b + 1], sign[b:b + 1])
        assert np.array_equal(_bits(glog[0]), _bits(log[b])) and np.array_equal(_bits(gpha[0]), _bits(pha[b]))
    if B > 1:                                                      # the rows do have ranges of their own
        assert len({tuple(r) for r in norm[:, 0:2].tolist()}) == B
    # no mask rows: the noise is not read
    log, pha, norm = _rows(spec, C, 0, 2, noise, sign)
    for b in range(B):
        _assert_row_is_solo(log, pha, norm, b, _solo(spec, b, C, 0, None, None, None), None, 0, "plain")


@pytest.mark.parametrize("F,M", GEOMETRIES)
def test_a_row_100_times_louder_beside_quiet_rows(F, M):
    C, R = 2, _mask_rows(M)
    spec, noise, sign = (t.clone() for t in _operands(3, F, M, C))
    spec[1] = 100.0 * spec[0]
    spec[2] = spec[0]
    log, pha, norm = _rows(spec, C, R, 2, noise, sign)
    for b in range(3):
        _assert_row_is_solo(log, pha, norm, b, _solo(spec, b, C, R, 2, noise, sign), 2, R, "loud")
    keep = M - R
    assert np.array_equal(_bits(log[0, :, :keep]), _bits(log[2, :, :keep]))          # the loud row between them moved neither
    assert float(norm[1, 1]) > float(norm[0, 1]) + 39.0                              # 40 dB


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("F,M", GEOMETRIES)
def test_a_silent_row_is_zeros_where_the_solo_encode_is_not_finite(F, M, C):
    """Rows 1 is digital silence and nothing else is: it is the one row compared against zeros instead of against the solo encode."""
    R = _mask_rows(M)
    keep = M - R
    spec, noise, sign = (t.clone() for t in _operands(3, F, M, C))
    spec[1] = 0.0
    silent = [b for b in range(3) if not bool(spec[b].any())]
    assert silent == [1]
    for mode in (None, 2):
        log, pha, norm = _rows(spec, C, R, mode, noise, sign)
        for b in range(3):
            solo = _solo(spec, b, C, R, mode, noise, sign)
            if b in silent:
                assert not torch.isfinite(solo[0][:, :, :keep]).any()
                assert float(norm[b, 0]) == float(norm[b, 1])
                assert (_bits(log[b, :, :keep]) == 0).all() and (_bits(pha[b]) == 0).all()
                # its noise rows have a range of their own and are the solo encode's
                assert np.array_equal(_bits(log[b, :, keep:]), _bits(solo[0][0, :, keep:]))
                assert np.array_equal(_bits(norm[b, 0:2]), _bits(solo[2][0:2]))
            else:
                _assert_row_is_solo(log, pha, norm, b, solo, mode, R, "beside silence")
    # a noise range of zero scales by 0 as well
    noise[1] = 0.25
    log, pha, norm = _rows(spec, C, R, 2, noise, sign)
    assert norm[1, 4:6].tolist() == [0.25, 0.25] and (_bits(log[1]) == 0).all()
    _assert_row_is_solo(log, pha, norm, 2, _solo(spec, 2, C, R, 2, noise, sign), 2, R, "beside constant noise")


@pytest.mark.parametrize("F,M", GEOMETRIES)
def test_a_row_with_nan_entries_is_its_solo_encode(F, M):
    C, R = 2, _mask_rows(M)
    spec, noise, sign = (t.clone() for t in _operands(3, F, M, C))
    spec[1].view(-1)[::7] = float('nan')
    noise[2].view(-1)[::5] = float('nan')
    log, pha, norm = _rows(spec, C, R, 2, noise, sign)
    assert np.isfinite(norm[:, [0, 1, 4, 5]].cpu().numpy()).all()
    for b in range(3):
        _assert_row_is_solo(log, pha, norm, b, _solo(spec, b, C, R, 2, noise, sign), 2, R, "nan")


def test_seventy_rows_off_alignment():
    """B = 70 at (9, 33): past any per-row chunk boundary, three rows in four off a 16-byte boundary."""
    B, F, M, C = 70, 9, 33, 2
    R = _mask_rows(M)
    spec, noise, sign = _operands(B, F, M, C)
    assert len({spec[b].data_ptr() % 16 for b in range(B)}) == 4
    log, pha, norm = _rows(spec, C, R, 2, noise, sign)
    for b in range(B):
        _assert_row_is_solo(log, pha, norm, b, _solo(spec, b, C, R, 2, noise, sign), 2, R, "seventy")


def test_rows_past_the_chunk_cap():
    """F * M = 35910 floats a row: 36 workgroups wanted, 32 used, so every workgroup of a row takes a second trip; F * M = 2 mod 4, so
    row 1 starts 8 bytes off."""
    import ctypes
    _lib, L = _L()
    B, F, M, C = 2, 70, 513, 2
    unit, wanted, used = ctypes.c_int64(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.p2phd_stream_grid(b"spectro_rows", 0, F * M, 1, ctypes.byref(unit), ctypes.byref(wanted), ctypes.byref(used)) == 0
    assert (wanted.value, used.value) == (36, 32) and L.p2phd_spectro_rows_partials_floats(B, F, M) == 4 * B * 32
    R = _mask_rows(M)
    spec, noise, sign = _operands(B, F, M, C)
    assert spec[1].data_ptr() % 16 == 8
    log, pha, norm = _rows(spec, C, R, 2, noise, sign)
    for b in range(B):
        _assert_row_is_solo(log, pha, norm, b, _solo(spec, b, C, R, 2, noise, sign), 2, R, "past the cap")


def test_two_runs_a_side_stream_and_one_workspace_twice():
    _lib, L = _L()
    B, F, M, C = 3, 40, 80, 2
    R = _mask_rows(M)
    spec, noise, sign = _operands(B, F, M, C)
    first = _rows(spec, C, R, 1, noise, sign)
    again = _rows(spec, C, R, 1, noise, sign)
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _rows(spec, C, R, 1, noise, sign, stream=_lib.stream_ptr())
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(first, other):
        assert np.array_equal(_bits(a), _bits(b))
    # two calls back to back on one workspace, the second on other rows: nothing of the first is left in it
    ws = _workspace(B, F, M)
    quiet = (spec * 1e-3).contiguous()
    _rows(quiet, C, R, 1, noise, sign, ws=ws)
    second = _rows(spec, C, R, 1, noise, sign, ws=ws)
    for a, b in zip(first, second):
        assert np.array_equal(_bits(a), _bits(b))
    assert not (_bits(ws[1]) == GUARD_BITS).any()                  # the workspace is written before it is read, all of it


# ------------------------------------------------------------------------------------------
# 2. the decodes
# ------------------------------------------------------------------------------------------
def _decode(entry, args_front, table, B, F, M, C, tail):
    _lib, L = _L()
    buf, spec = _guarded(B * F * M)
    rc = getattr(L, entry)(*[_lib.ptr(t) for t in args_front], _lib.ptr(table), B, F, M, C, *tail, _lib.ptr(spec), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(buf, B * F * M) and not (_bits(spec) == GUARD_BITS).any(), (entry, rc)
    return spec.reshape(B, F, M)


@pytest.mark.parametrize("B,F,M,C", SHAPES)
def test_row_decodes_are_the_plain_decodes_row_by_row(B, F, M, C):
    spec, noise, sign = _operands(B, F, M, C)
    R = _mask_rows(M)
    log, pha, norm = _rows(spec, C, R, 2, noise, sign)
    rng = np.random.default_rng(B + F + M + C)
    sr = torch.from_numpy(rng.random((B, C, M, F)).astype(np.float32)).to(DEV)       # a generator's output in [0, 1]
    pha = pha.reshape(B, M, F).contiguous()
    keep = M - R
    got = _decode("p2phd_spectro_decode_signed_rows", (sr, pha), norm, B, F, M, C, (keep, MIN_VALUE, 1.0))
    for b in range(B):
        want = _decode("p2phd_spectro_decode_signed", (sr[b:b + 1], pha[b:b + 1]), norm[b, 0:2].clone(), 1, F, M, C, (keep, MIN_VALUE, 1.0))
        assert np.array_equal(_bits(got[b]), _bits(want[0])), b
    if B > 1:
        one = _decode("p2phd_spectro_decode_signed", (sr, pha), norm[0, 0:2].clone(), B, F, M, C, (keep, MIN_VALUE, 1.0))
        assert not np.array_equal(_bits(got[1]), _bits(one[1]))                      # (the range matters)
    for fade in (0, 5):
        got = _decode("p2phd_spectro_decode_spliced_rows", (sr, log, pha), norm, B, F, M, C, (keep, fade, MIN_VALUE, 1.0))
        for b in range(B):
            want = _decode("p2phd_spectro_decode_spliced", (sr[b:b + 1], log[b:b + 1].contiguous(), pha[b:b + 1]), norm[b, 0:2].clone(), 1, F,
                           M, C, (keep, fade, MIN_VALUE, 1.0))
            assert np.array_equal(_bits(got[b]), _bits(want[0])), (b, fade)


# ------------------------------------------------------------------------------------------
# 3. counters, empty batches and refusals
# ------------------------------------------------------------------------------------------
def test_counters_empty_batch_and_refusals():
    _lib, L = _L()
    B, F, M, C = 3, 9, 33, 2
    spec, noise, sign = _operands(B, F, M, C)
    R = _mask_rows(M)
    _count(reset=True)
    _count(b"normscope", reset=True)
    log, pha, norm = _rows(spec, C, R, 2, noise, sign)
    assert _count() == 1
    p = pha.reshape(B, M, F).contiguous()
    _decode("p2phd_spectro_decode_signed_rows", (log, p), norm, B, F, M, C, (M - R, MIN_VALUE, 1.0))
    assert _count() == 2
    _decode("p2phd_spectro_decode_spliced_rows", (log, log, p), norm, B, F, M, C, (M - R, 3, MIN_VALUE, 1.0))
    assert _count() == 3 and _count(b"normscope") == 0
    _decode("p2phd_spectro_decode_signed", (log, p), norm[0, 0:2].clone(), B, F, M, C, (M - R, MIN_VALUE, 1.0))
    assert _count() == 3                                           # the plain entries count nothing here
    # B = 0 launches and writes nothing
    rc, l0, p0, n0, intact = _rows_rc(spec, C, R, 2, noise, sign, nb=0, ws=_workspace(1, F, M))
    assert rc == 0 and intact and l0.numel() == 0 and _count() == 3
    assert L.p2phd_spectro_rows_partials_floats(0, F, M) == 0 and L.p2phd_spectro_rows_partials_floats(B, 0, M) == 0
    einval = L.p2phd_spectro_decode_signed(_lib.ptr(spec), _lib.ptr(spec), _lib.ptr(norm), B, F, M, 3, 0, MIN_VALUE, 1.0, _lib.ptr(spec),
                                           _lib.stream_ptr())
    assert einval != 0

    def refused(res, word, name="spectro_encode_rows"):
        rc, lg, ph, nr, intact = res
        text = L.p2phd_last_error().decode()
        assert rc == einval and name in text and word in text, (rc, text)
        assert intact and all((_bits(t) == GUARD_BITS).all() for t in (lg, ph, nr))   # nothing written

    refused(_rows_rc(spec, C, R, 2, noise, sign, channels=3), "channels")
    refused(_rows_rc(spec, C, R, 3, noise, sign), "mask_mode")
    refused(_rows_rc(spec, C, R, 1, noise, None), "sign")
    refused(_rows_rc(spec, C, M + 1, 2, noise, sign), "mask_rows")
    refused(_rows_rc(spec, C, R, 2, noise, sign, norm_null=True), "null pointer")
    one = torch.full((8,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    args = (F, M, C, ALPHA, MIN_VALUE, R, 2, _lib.ptr(noise), None)
    for k in range(4):                                             # spec, log_spectro, pha, workspace in turn
        ptrs = [_lib.ptr(one)] * 5
        ptrs[(0, 2, 3, 4)[k]] = None
        rc = L.p2phd_spectro_encode_rows(ptrs[0], 1, *args, ptrs[1], ptrs[2], ptrs[3], ptrs[4], _lib.stream_ptr())
        assert rc == einval and "null pointer" in L.p2phd_last_error().decode()
    rc = L.p2phd_spectro_encode_rows(_lib.ptr(one), 65536, *args, _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), _lib.stream_ptr())
    assert rc == einval and "grid too large" in L.p2phd_last_error().decode()
    for entry, front in (("p2phd_spectro_decode_signed_rows", 2), ("p2phd_spectro_decode_spliced_rows", 3)):
        tail = (M - R, MIN_VALUE, 1.0) if front == 2 else (M - R, 0, MIN_VALUE, 1.0)
        name = entry[len("p2phd_"):]
        rc = getattr(L, entry)(*[_lib.ptr(one)] * front, None, 1, F, M, C, *tail, _lib.ptr(one), _lib.stream_ptr())
        assert rc == einval and name in L.p2phd_last_error().decode() and "null pointer" in L.p2phd_last_error().decode()
        rc = getattr(L, entry)(*[_lib.ptr(one)] * front, _lib.ptr(one), 1, F, M, 3, *tail, _lib.ptr(one), _lib.stream_ptr())
        assert rc == einval and "channels" in L.p2phd_last_error().decode()
        rc = getattr(L, entry)(*[_lib.ptr(one)] * front, _lib.ptr(one), 65536, F, M, C, *tail, _lib.ptr(one), _lib.stream_ptr())
        assert rc == einval and "grid too large" in L.p2phd_last_error().decode()
    torch.cuda.synchronize()
    assert bool((one.view(torch.int32) == GUARD_BITS).all())
    assert _count() == 3 and _count(b"normscope") == 0
