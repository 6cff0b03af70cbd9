"""norm_scope without a GPU: the option's validation, the parser, and the premise of the feature on a numpy restatement
(tests/_norm_scope_ref.py) -- a silent group under its own range is NaN, under its clip's range it is zeros."""
import itertools

import numpy as np
import pytest

import _norm_scope_ref as NR


def test_check_norm_scope():
    from pix2pixhdaudiosr_amd.generate import NORM_SCOPES, check_norm_scope
    assert NORM_SCOPES == ('group', 'clip')
    assert check_norm_scope() == 'group'
    for scope in NORM_SCOPES:
        assert check_norm_scope(scope) == scope
    for bad in ('file', 'Clip', '', None, 1, 'folder'):
        with pytest.raises(ValueError, match=r"norm_scope must be 'group' or 'clip'"):
            check_norm_scope(bad)
    with pytest.raises(ValueError, match=r"^generate: norm_scope"):
        check_norm_scope('x', who="generate")


def test_parser_default_and_choices(capsys):
    from pix2pixhdaudiosr_amd.generate import _parser
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]
    assert _parser().parse_args(base).norm_scope == 'group'
    assert _parser().parse_args(base + ["--norm_scope", "clip"]).norm_scope == 'clip'
    with pytest.raises(SystemExit):
        _parser().parse_args(base + ["--norm_scope", "file"])
    assert "--norm_scope" in capsys.readouterr().err


def test_super_resolver_refuses_a_bad_scope_before_it_touches_the_model():
    from types import SimpleNamespace
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    opt = SimpleNamespace(segment_length=31 * 32, batchSize=2, hr_sampling_rate=48000, lr_sampling_rate=8000, n_fft=64, hop_length=32,
                          win_length=64, center=True, mdct_type='mdct4')
    with pytest.raises(ValueError, match=r"norm_scope must be"):
        SuperResolver(SimpleNamespace(device='cpu', mdct_type='mdct4'), opt, norm_scope='file')


@pytest.mark.parametrize("channels", [1, 2])
def test_silent_group_under_its_own_and_under_a_wider_range(channels):
    rng = np.random.default_rng(5)
    loud = rng.standard_normal((2, 9, 16)).astype(np.float32)
    silent = np.zeros((2, 9, 16), dtype=np.float32)
    d_silent, d_loud = NR.db_encode(silent, channels=channels), NR.db_encode(loud, channels=channels)
    floor = np.float32(20) * np.log10(np.float32(1e-7)) - np.float32(20)
    assert d_silent.shape == (2, channels, 16, 9) and (d_silent == floor).all()
    own = NR.own_range(d_silent)
    assert own[0] == own[1] == floor
    # group scope: the group's own range has no width
    assert np.isnan(NR.normalise(d_silent, own)).all()
    # clip scope: the clip's range, which a louder group widened, puts silence at the bottom
    clip = NR.fold(own, NR.own_range(d_loud))
    assert clip[0] == floor and clip[1] > floor
    got = NR.normalise(d_silent, clip)
    assert np.isfinite(got).all() and (got == 0).all()
    # a clip that is silence throughout: the guard
    guarded = NR.normalise(d_silent, own, guard=True)
    assert np.isfinite(guarded).all() and (guarded == 0).all()
    # the guard moves nothing where the range has a width
    assert np.array_equal(NR.normalise(d_loud, clip, guard=True), NR.normalise(d_loud, clip))
    both = NR.normalise(d_loud, clip)
    assert both.min() >= 0 and both.max() == 1


def test_fold_is_associative_and_commutative():
    rng = np.random.default_rng(6)
    ranges = [NR.own_range(NR.db_encode(a * rng.standard_normal((1, 5, 8)).astype(np.float32))) for a in (1e-3, 1.0, 30.0)]
    ranges.append(NR.own_range(NR.db_encode(np.zeros((1, 5, 8), dtype=np.float32))))
    whole = NR.own_range(np.concatenate([NR.db_encode(a * np.ones((1, 1, 1), dtype=np.float32)) for a in (1,)]))  # (a range of one value)
    ranges.append(whole)
    for a, b in itertools.permutations(ranges, 2):
        assert NR.fold(a, b) == NR.fold(b, a)
        assert NR.fold(a, NR.EMPTY) == a and NR.fold(NR.EMPTY, a) == a
    for a, b, c in itertools.permutations(ranges, 3):
        assert NR.fold(NR.fold(a, b), c) == NR.fold(a, NR.fold(b, c))
    # the fold of the pieces is the range of the whole
    pieces = [a * rng.standard_normal((1, 5, 8)).astype(np.float32) for a in (1e-3, 1.0, 30.0)]
    acc = NR.EMPTY
    for p in pieces:
        acc = NR.fold(acc, NR.own_range(NR.db_encode(p)))
    assert acc == NR.own_range(NR.db_encode(np.concatenate(pieces)))
