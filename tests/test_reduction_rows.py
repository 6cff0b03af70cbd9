"""p2phd_reduction_rows on the host: which grid the launches take that size themselves by a region of the library's reduction
scratch (csrc/norm.hip: instnorm_bwd_rows, act_bwd_db_rows -- the functions the launchers themselves call).  Nothing is launched
and no device is needed.

Pinned here: every listed case of the per-element suite (K.IN_CASES, K.ACT_DB_CASES) runs UNCLAMPED; the cases that
tests/test_gpu_companions.py and tests/test_gpu_reductions.py run as "the clamped path" ARE clamped, in every storage type, with a
grid stride that stays a multiple of the pieces per pixel; and the query refuses, with a text, exactly where the launchers do."""
import pytest

import _companions as K

LIBS = ("bf16", "f16")
CODES = ((1, 8), (0, 4))                                        # (dtype code, elements per 16-byte piece): 16-bit storage, f32
EINVAL = -1


def _lib(kind):
    from pix2pixhdaudiosr_amd import _lib
    return _lib.lib(kind)


@pytest.mark.parametrize("kind", LIBS)
def test_listed_cases_are_not_clamped(kind):
    L = _lib(kind)
    for code, _ in CODES:
        for case in K.IN_CASES:
            N, HW, Cc, two_pass = case[:4]
            rc, wanted, used = K.reduction_rows(L, "instnorm_bwd", code, N, HW, Cc)
            assert rc == 0, (case, L.p2phd_last_error())
            assert L.p2phd_instnorm_act_bwd_two_pass(code, N, HW, Cc) == two_pass
            assert used == wanted and (wanted >= 1) == bool(two_pass), (case[:3], code, wanted, used)
        for P, Cc in K.ACT_DB_CASES:
            rc, wanted, used = K.reduction_rows(L, "act_bwd_db", code, 1, P, Cc)
            assert rc == 0, ((P, Cc), L.p2phd_last_error())
            assert used == wanted >= 1, ((P, Cc), code, wanted, used)


@pytest.mark.parametrize("kind", LIBS)
def test_clamp_cases_are_clamped_to_a_multiple_of_the_grid_unit(kind):
    L = _lib(kind)
    for code, epp in CODES:
        for case in K.IN_CLAMP_CASES:
            N, HW, Cc = case[:3]
            assert L.p2phd_instnorm_act_bwd_two_pass(code, N, HW, Cc) == 1
            wanted, used = K.clamped_rows(L, "instnorm_bwd", code, N, HW, Cc, epp)
            assert 2 * K.cpitch(Cc) * N * used <= 4 << 20, (case[:3], used)        # the rows fit the region (csrc/core.hip, kFoldFloats)
        for P, Cc in K.ACT_DB_CLAMP_CASES:
            wanted, used = K.clamped_rows(L, "act_bwd_db", code, 1, P, Cc, epp)
            assert K.cpitch(Cc) * used <= 1 << 20, ((P, Cc), used)


@pytest.mark.parametrize("kind", LIBS)
def test_nothing_to_launch_answers_zero_rows(kind):
    L = _lib(kind)
    for family, N, P in (("instnorm_bwd", 0, 700), ("instnorm_bwd", 2, 0), ("act_bwd_db", 1, 0)):
        assert K.reduction_rows(L, family, 1, N, P, 8) == (0, 0, 0), (family, N, P)


@pytest.mark.parametrize("kind", LIBS)
@pytest.mark.parametrize("family,N,P,Cc,text", [
    ("instnorm_bwd", 2049, 700, 8, b"samples"),                 # more samples than the region has tickets
    ("instnorm_bwd", 2048, 700, 4096, b"scratch"),              # rows_max = 2^21 / (4096 * 2048) = 0: not one grid unit of rows
    ("instnorm_bwd", 2, 700, 4097, b"channels"),
    ("act_bwd_db", 1, 700, 4097, b"channels"),
    ("act_bwd_db", 2, 700, 8, b"N = 1"),
    ("colsum", 1, 700, 8, b"colsum"),
])
def test_refusals(kind, family, N, P, Cc, text):
    """By the query alone: the launchers refuse in the same function, and are never called here on buffers of these sizes."""
    L = _lib(kind)
    for code, _ in CODES:
        assert K.reduction_rows(L, "act_bwd_db", code, 1, 40, 40)[0] == 0       # (a good call in front: the text below is this call's)
        rc, wanted, used = K.reduction_rows(L, family, code, N, P, Cc)
        assert rc == EINVAL and (wanted, used) == (0, 0), (family, N, P, Cc, rc, wanted, used)
        err = L.p2phd_last_error()
        assert err and text in err, err
