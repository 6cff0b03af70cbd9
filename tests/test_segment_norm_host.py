"""segment_norm without a GPU: the premise on a numpy restatement (tests/_norm_rows_ref.py) -- every row of a batch under its own
range, a silent row zeros and not NaN --, the grouping of a clip's rows (plans.group_rows_plan), every refusal of the option and
of the command line, and the walk itself on a SuperResolver built without a device."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _norm_rows_ref as RR
import _norm_scope_ref as NR


# ------------------------------------------------------------------------------------------
# the premise
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_every_row_gets_its_own_range_and_silence_stays_silence(channels):
    rng = np.random.default_rng(11)
    loud = rng.standard_normal((9, 16)).astype(np.float32)
    batch = np.stack([loud, np.zeros_like(loud), loud / np.float32(100)])
    log, table = RR.encode_rows(batch, channels=channels)
    assert log.shape == (3, channels, 16, 9) and table.shape == (3, 8)
    floor = np.float32(20) * np.log10(np.float32(1e-7)) - np.float32(20)
    # the silent row: a range of zero, zeros and not NaN; under the batch's range, as 'group' takes it, it is NaN only when alone
    assert table[1, 0] == table[1, 1] == floor
    assert np.isfinite(log).all() and (log[1] == 0).all()
    alone = NR.db_encode(batch[1:2], channels=channels)
    assert np.isnan(NR.normalise(alone, NR.own_range(alone))).all()
    # the loud and the quiet row: each spans [0, 1] under its own range, 40 dB apart
    for b in (0, 2):
        assert log[b].min() == 0 and abs(float(log[b].max()) - 1.0) <= 2.0 ** -23      # (x * (1 / x): two roundings)
        assert table[b, 0] < table[b, 1]
        solo, solo_table = RR.encode_rows(batch[b:b + 1], channels=channels)
        assert np.array_equal(solo[0], log[b]) and np.array_equal(solo_table[0], table[b])
    assert abs(float(table[0, 1] - table[2, 1]) - 40.0) < 1e-3
    # under one range for the batch the quiet row would sit 40 dB down in it, never reaching 1
    db = NR.db_encode(batch, channels=channels)
    shared = NR.normalise(db, NR.own_range(db))
    assert shared[2].max() < 0.9 and abs(float(shared[0].max()) - 1.0) <= 2.0 ** -23
    # entries that are not computed
    assert (table[:, [2, 3, 6, 7]] == 0).all() and (table[:, 4] == np.inf).all() and (table[:, 5] == -np.inf).all()


def test_row_stats_pass_over_nan_and_take_the_noise_per_row():
    rng = np.random.default_rng(12)
    spec = rng.standard_normal((2, 5, 8)).astype(np.float32)
    noise = rng.standard_normal((2, 2, 3, 5)).astype(np.float32)
    noise[1] *= 7
    want = RR.row_stats(spec, noise)
    holes = spec.copy()
    holes[0, 0, 0] = np.nan
    got = RR.row_stats(holes, noise)
    assert np.isfinite(got[:, [0, 1, 4, 5]]).all() and np.array_equal(got[1], want[1])
    for b in range(2):
        assert want[b, 4] == noise[b].min() and want[b, 5] == noise[b].max()
    assert RR.encode_rows(np.zeros((0, 5, 8), dtype=np.float32))[0].shape == (0, 2, 8, 5)


# ------------------------------------------------------------------------------------------
# the grouping
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 2, 4, 5])
@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5, 8, 9, 30])
def test_group_rows_plan_covers_every_row_once(rows, batch):
    from pix2pixhdaudiosr_amd.generate import group_rows_plan
    plan = group_rows_plan(rows, batch)
    assert len(plan) == math.ceil(rows / batch)
    seen = [r for r0, n in plan for r in range(r0, r0 + n)]
    assert seen == list(range(rows))
    assert all(n == batch for _, n in plan[:-1])                   # only the last group has fillers
    if plan:
        assert 1 <= plan[-1][1] <= batch and plan[-1][1] == rows - batch * (len(plan) - 1)
    if rows == 0:
        assert plan == []


def test_group_rows_plan_refusals():
    from pix2pixhdaudiosr_amd.generate import group_rows_plan
    for rows, batch, word in ((-1, 2, "rows"), (3, 0, "batch"), (3, -1, "batch"), (2.0, 2, "rows"), (3, 2.5, "batch"), (True, 2, "rows"),
                              (None, 2, "rows")):
        with pytest.raises(ValueError, match=r"group_rows_plan: %s" % word):
            group_rows_plan(rows, batch)


def test_workspace_query_is_the_grid_of_the_statistics():
    """Host arithmetic of the library: p2phd_spectro_rows_partials_floats is four floats per workgroup of the (chunk, row) grid, whose
    chunks are the stream family "spectro_rows": a float4 per thread, at most 32 workgroups a row."""
    import ctypes
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    for F, M in ((9, 33), (9, 64), (40, 80), (128, 512), (32, 1024), (33, 1024), (1, 1), (128, 2048)):
        unit, wanted, used = ctypes.c_int64(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        assert L.p2phd_stream_grid(b"spectro_rows", 0, F * M, 1, ctypes.byref(unit), ctypes.byref(wanted), ctypes.byref(used)) == 0
        want = max(1, math.ceil(math.ceil(F * M / 4) / 256))
        assert (wanted.value, used.value, unit.value) == (want, min(want, 32), min(want, 32) * 1024), (F, M)
        for B in (1, 3, 70):
            assert L.p2phd_spectro_rows_partials_floats(B, F, M) == 4 * B * min(want, 32)
    assert L.p2phd_spectro_rows_partials_floats(0, 9, 33) == 0
    for B, F, M in ((-1, 9, 33), (2, 0, 33), (2, 9, 0)):
        assert L.p2phd_spectro_rows_partials_floats(B, F, M) == 0


# ------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------
def test_check_segment_norm():
    from pix2pixhdaudiosr_amd.generate import NORM_SCOPES, check_segment_norm
    assert NORM_SCOPES == ('group', 'clip')                        # the option is no third scope
    assert check_segment_norm() is False
    assert check_segment_norm(False, 'group') is False and check_segment_norm(False, 'clip') is False
    assert check_segment_norm(True) is True and check_segment_norm(True, 'group') is True
    with pytest.raises(ValueError, match=r"^SuperResolver: segment_norm gives every segment its own range and norm_scope 'clip'"):
        check_segment_norm(True, 'clip')
    with pytest.raises(ValueError, match=r"^generate: segment_norm"):
        check_segment_norm(True, 'clip', who="generate")
    for bad in (1, 0, None, 'yes', 'rows', 1.0):
        with pytest.raises(ValueError, match=r"segment_norm must be a bool"):
            check_segment_norm(bad)
    for flag in (False, True):
        with pytest.raises(ValueError, match=r"norm_scope must be 'group' or 'clip'"):
            check_segment_norm(flag, 'segment')


def _opt():
    return SimpleNamespace(segment_length=31 * 32, batchSize=2, hr_sampling_rate=48000, lr_sampling_rate=8000, n_fft=64, hop_length=32,
                           win_length=64, center=True, mdct_type='mdct4')


def test_super_resolver_refuses_before_it_touches_the_model():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    model = SimpleNamespace(device='cpu', mdct_type='mdct4')
    with pytest.raises(ValueError, match=r"segment_norm gives every segment its own range"):
        SuperResolver(model, _opt(), norm_scope='clip', segment_norm=True)
    with pytest.raises(ValueError, match=r"segment_norm must be a bool"):
        SuperResolver(model, _opt(), segment_norm='rows')
    with pytest.raises(ValueError, match=r"norm_scope must be"):
        SuperResolver(model, _opt(), norm_scope='segment', segment_norm=True)
    assert SuperResolver.segment_norm is False                     # what an object built without __init__ runs with


def test_command_line(capsys, tmp_path):
    from pix2pixhdaudiosr_amd.generate import _parser, main
    base = ["--input", str(tmp_path / "a.wav"), "--output", str(tmp_path / "b.wav"), "--load_pretrain", str(tmp_path / "no_such_checkpoint")]
    assert _parser().parse_args(base).segment_norm is False
    a = _parser().parse_args(base + ["--segment_norm"])
    assert a.segment_norm is True and a.norm_scope == 'group'
    with pytest.raises(SystemExit):
        _parser().parse_args(base + ["--segment_norm", "1"])
    capsys.readouterr()
    # with --norm_scope clip: refused before the options file, the checkpoint or the input is opened (none of them exists)
    with pytest.raises(SystemExit) as e:
        main(base + ["--segment_norm", "--norm_scope", "clip"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "generate: segment_norm gives every segment its own range" in err and "norm_scope 'clip'" in err
    assert "--segment_norm" in _parser().format_help()


# ------------------------------------------------------------------------------------------
# the walk, on an object built without a device
# ------------------------------------------------------------------------------------------
def _stub(batch, T=6, noise_shape=None):
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    sr = SuperResolver.__new__(SuperResolver)
    sr.device, sr.batch, sr.T, sr.graph, sr.segment_norm = torch.device('cpu'), batch, T, False, True
    sr.model = SimpleNamespace(mask_noise_shape=None if noise_shape is None else (lambda b, t: (b,) + noise_shape))
    sr.calls = []

    def group(seg, noise):                                         # the rows back, doubled; a row's range: (its first sample, its sum)
        sr.calls.append((seg.clone(), None if noise is None else noise.clone()))
        table = torch.zeros((seg.shape[0], 8))
        table[:, 0], table[:, 1] = seg[:, 0], seg.sum(dim=1)
        return 2 * seg, table

    sr._group_rows = group
    return sr


@pytest.mark.parametrize("C,S,batch", [(1, 3, 4), (1, 4, 4), (2, 5, 4), (2, 3, 2), (3, 3, 1), (1, 0, 3), (2, 0, 3), (1, 1, 5)])
def test_walk_calls_the_group_function_with_full_groups(C, S, batch):
    T = 6
    sr = _stub(batch, T)
    seg = 1.0 + torch.arange(C * S * T, dtype=torch.float32).reshape(C * S, T)
    out = torch.full_like(seg, float('nan'))
    sr._walk_rows(seg, out, None, C, S)
    assert len(sr.calls) == math.ceil(C * S / batch)
    got = torch.cat([rows for rows, _ in sr.calls]) if sr.calls else seg[:0]
    assert all(rows.shape == (batch, T) and nz is None for rows, nz in sr.calls)
    assert torch.equal(got[:C * S], seg) and (got[C * S:] == 0).all() and got.shape[0] - C * S < batch     # fillers: zeros, the last group's
    assert torch.equal(out, 2 * seg)                               # every row's output back in its place, the fillers' dropped
    assert sr.last_norm.shape == (C, S, 2)
    assert torch.equal(sr.last_norm.reshape(-1, 2), torch.stack([seg[:, 0], seg.sum(dim=1)], dim=1))


def test_walk_slices_given_noise_and_draws_full_groups():
    C, S, batch, T, shape = 2, 3, 4, 6, (2, 3, 5)
    sr = _stub(batch, T, shape)
    seg = torch.ones((C * S, T))
    noise = 1.0 + torch.arange(C * S * 30, dtype=torch.float32).reshape((C * S,) + shape)
    sr._walk_rows(seg, torch.empty_like(seg), noise, C, S)
    assert [nz.shape for _, nz in sr.calls] == [(batch,) + shape] * 2
    assert torch.equal(torch.cat([nz for _, nz in sr.calls])[:C * S], noise)
    assert (sr.calls[1][1][2:] == 0).all()                          # the fillers' noise: zeros
    # without a given noise: one draw of the full group's shape per group
    sr.calls.clear()
    torch.manual_seed(3)
    sr._walk_rows(seg, torch.empty_like(seg), None, C, S)
    torch.manual_seed(3)
    want = [torch.randn((batch,) + shape) for _ in range(2)]
    assert all(torch.equal(nz, w) for (_, nz), w in zip(sr.calls, want))
    with pytest.raises(ValueError, match=r"enhance_lr: noise for rows 0\.\.3 has shape"):
        sr._walk_rows(seg, torch.empty_like(seg), noise[:, :1], C, S)
