"""Host side of the look-ahead true-peak limiter of whole-file generation (csrc/limiter.hip): the window the library fills against
the restatement of tests/_limiter_ref.py, limiter_plan and check_limiter, the invariants of the curve on random r, and the
plumbing -- result keys, CSV columns and printed lines do not move without the option, and with it the option's arguments reach the
output stage.  No GPU; the stub resolver is the pattern of tests/test_outstage_host.py."""
import csv
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _limiter_ref as LR


# ------------------------------------------------------------------------------------------
# the window
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", (1, 2, 7, 72, 240, 1023, 1024))
def test_window_is_the_restatement_rounded_once_and_symmetric(A):
    from pix2pixhdaudiosr_amd.generate import limiter_window
    w = limiter_window(A).numpy()
    want = LR.window(A)
    assert w.dtype == np.float32 and w.shape == (A + 1,)
    # float64 values that differ in the last place or two (another cos, another order of the sum) round to the same fp32 number
    # or to its neighbour: half an ulp of slack beside the rounding itself
    assert (np.abs(w.astype(np.float64) - want) <= 0.75 * np.spacing(want.astype(np.float32)).astype(np.float64)).all()
    assert np.array_equal(w.view(np.int32), w[::-1].copy().view(np.int32))                  # symmetric bit for bit
    assert (w > 0).all()
    # sum 1 within one fp32 rounding per term
    assert abs(w.astype(np.float64).sum() - 1.0) <= (A + 1) * 2.0 ** -25 * w.max()


def test_window_of_one_sample_and_refusals():
    from pix2pixhdaudiosr_amd.generate import limiter_window
    assert limiter_window(1).tolist() == [0.5, 0.5]
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="lookahead"):
            limiter_window(bad)


# ------------------------------------------------------------------------------------------
# limiter_plan, check_limiter
# ------------------------------------------------------------------------------------------
def test_limiter_plan():
    from pix2pixhdaudiosr_amd import generate as G
    assert (G.LIMITER_LOOKAHEAD_MS, G.LIMITER_HOLD_MS, G.LIMITER_MAX_LOOKAHEAD, G.LIMITER_MAX_HOLD) == (5.0, 20.0, 1024, 4096)
    assert G.limiter_plan(48000) == {'lookahead': 240, 'hold': 960}
    assert G.limiter_plan(44100) == {'lookahead': 220, 'hold': 882}                         # round(220.5) -> 220 (ties to even), 882
    assert G.limiter_plan(48000, 1.5, 0) == {'lookahead': 72, 'hold': 0}
    assert G.limiter_plan(48000, 0.0, 0.0) == {'lookahead': 1, 'hold': 0}                    # at least one sample ahead
    assert G.limiter_plan(8000, 0.01, 0.07) == {'lookahead': 1, 'hold': 1}
    assert G.limiter_plan(48000, 1024 / 48.0, 4096 / 48.0) == {'lookahead': 1024, 'hold': 4096}
    with pytest.raises(ValueError, match=r"lookahead_ms 30 is 1440 samples at 48000 Hz, more than 1024: at most 21\.3333 ms"):
        G.limiter_plan(48000, 30)
    with pytest.raises(ValueError, match=r"hold_ms 100 is 4800 samples at 48000 Hz, more than 4096: at most 85\.3333 ms"):
        G.limiter_plan(48000, None, 100)
    for kw in (dict(lookahead_ms=-1.0), dict(hold_ms=float('nan')), dict(lookahead_ms=True), dict(hold_ms='20'), dict(lookahead_ms=float('inf'))):
        with pytest.raises(ValueError, match="_ms must be"):
            G.limiter_plan(48000, **kw)
    for rate in (0, -48000, float('inf'), True, '48000'):
        with pytest.raises(ValueError, match="rate"):
            G.limiter_plan(rate)


def test_check_limiter():
    from pix2pixhdaudiosr_amd.generate import CLIP_MODES, check_limiter, check_output_options
    assert CLIP_MODES == ('clamp', 'guard', 'error')                                        # the limiter is no clip mode
    guard = check_output_options('float32', clip='guard', ceiling_dbfs=-1.0)
    assert check_limiter(False, None, None, None, 'pcm16', 48000) is None
    assert check_limiter(False, None, None, guard, 'float32', 48000) is None
    assert check_limiter(True, None, None, guard, 'float32', 48000) == {'lookahead': 240, 'hold': 960, 'lookahead_ms': None, 'hold_ms': None}
    assert check_limiter(True, 1.5, 0, guard, 'float32', 48000) == {'lookahead': 72, 'hold': 0, 'lookahead_ms': 1.5, 'hold_ms': 0}
    for value in (1, 0, None, 'yes'):
        with pytest.raises(ValueError, match="limiter must be a bool"):
            check_limiter(value, None, None, guard, 'float32', 48000)
    for kw in (dict(lookahead_ms=5.0), dict(hold_ms=0.0)):
        with pytest.raises(ValueError, match="options of limiter=True"):
            check_limiter(False, kw.get('lookahead_ms'), kw.get('hold_ms'), guard, 'float32', 48000)
    for stage in (None, check_output_options('pcm16', report_peaks=True), check_output_options('pcm16', clip='error')):
        with pytest.raises(ValueError, match="limiter is an option of clip='guard'"):
            check_limiter(True, None, None, stage, 'pcm16', 48000)
    with pytest.raises(ValueError, match="enhance_folder: limiter_plan: lookahead_ms 30 .* at most 21.3333 ms"):
        check_limiter(True, 30, None, guard, 'float32', 48000, "enhance_folder")


# ------------------------------------------------------------------------------------------
# the curve's invariants (the restatement; tests/test_gpu_limiter.py holds the kernel to it)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,H", ((1, 0), (7, 3), (72, 0), (240, 960)))
def test_curve_never_asks_for_less_than_a_sample_needs_and_is_one_out_of_reach(A, H):
    rng = np.random.default_rng(100 * A + H)
    L = 12000
    r = np.ones(L, dtype=np.float32)
    at = rng.choice(L, 40, replace=False)
    r[at] = rng.uniform(0.05, 1.0, 40).astype(np.float32)
    r[4000:8000] = 1.0                                             # a stretch nothing reaches from inside
    r[0], r[L - 1] = 0.5, 0.25                                     # both ends
    w = LR.window(A).astype(np.float32)
    for g in (LR.curve(r, w, A, H)[0], LR.curve32(r, w, A, H)):
        assert (g <= r).all() and (g > 0).all()
        out = ~LR.reach(r, A, H)
        assert out.any() and (g[out] == 1.0).all()
        assert (g[LR.reach(r, A, H)] <= 1.0).all()
    # the two orders agree within the bound of the fp32 sum
    g64, a = LR.curve(r, w, A, H)
    assert (np.abs(LR.curve32(r, w, A, H).astype(np.float64) - g64) <= (A + 1) * 2.0 ** -24 * a + 2.0 ** -25).all()


def test_sliding_minimum_of_the_restatement_on_a_hand_case():
    r = np.array([1, 1, 0.5, 1, 1, 1, 0.25, 1], dtype=np.float32)
    # A = 1, H = 2: h[j] = min r[j - 2 .. j + 1], j = -1 .. 7
    assert LR.sliding_min(r, 1, 2).tolist() == [1, 1, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25]
    g = LR.curve32(r, np.array([0.5, 0.5], dtype=np.float32), 1, 2)
    assert g.tolist() == [1, 0.75, 0.5, 0.5, 0.5, 0.375, 0.25, 0.25]


# ------------------------------------------------------------------------------------------
# plumbing
# ------------------------------------------------------------------------------------------
def _stub_resolver():
    from pix2pixhdaudiosr_amd.generate import SuperResolver

    class Stub(SuperResolver):
        def __init__(self):
            self.opt = SimpleNamespace(lr_sampling_rate=12000, hr_sampling_rate=48000)
            self.device = torch.device("cpu")
            self.calls = []

        def _read(self, path, slot='in0'):
            from pix2pixhdaudiosr_amd.data import wavio
            self.calls.append(('read', path))
            return torch.zeros(0, dtype=torch.uint8), wavio.info(path), slot

        def _decode(self, host, meta, slot):
            return torch.linspace(-1, 1, meta.num_frames)[None].repeat(meta.num_channels, 1)

        def enhance_lr(self, lr_audio, noise=None):
            return 1.7 * lr_audio

        def _write(self, path_out, sr, encoding, stage=None, **extra):
            self.calls.append(('write', path_out, encoding, stage, extra))
            if stage is None:
                return None
            C = sr.shape[0]
            out = {'peak': [0.8] * C, 'peak_dbfs': [-1.9] * C, 'clipped': [0] * C, 'nonfinite': [0] * C, 'gain': 0.999}
            if 'true_peak' in extra:
                out.update(true_peak=[0.9] * C, true_peak_dbtp=[-0.9] * C)
            if 'limiter' in extra:
                out['limiter'] = {'lookahead': extra['limiter']['lookahead'], 'hold': extra['limiter']['hold'], 'max_reduction_db': -3.8,
                                  'limited_samples': 16, 'input_true_peak_dbtp': 2.8}
            return out
    return Stub()


@pytest.fixture
def stub(tmp_path, monkeypatch):
    from pix2pixhdaudiosr_amd.data import audio_dataset, wavio
    monkeypatch.setattr(audio_dataset, "lr_round_trip", lambda raw, *a, **k: raw)
    src = tmp_path / "in"
    src.mkdir()
    for name, C in (("a.wav", 1), ("b.wav", 2)):
        wavio.save(str(src / name), torch.zeros(C, 64), 16000)
    return _stub_resolver(), src


def test_nothing_moves_without_the_option(stub, tmp_path):
    """The stub of tests/test_outstage_host.py takes _write(path_out, sr, encoding, stage=None) and no keyword: ours records any
    keyword it is given, and without the option there is none, by position or by name."""
    sr, src = stub
    for kw in ({}, dict(limiter=False), dict(limiter=False, limiter_lookahead_ms=None, limiter_hold_ms=None)):
        res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', **kw)
        assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'sr']
        assert sr.calls[-1] == ('write', str(tmp_path / "o.wav"), 'pcm16', None, {})
        res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', clip='guard', ceiling_dbfs=-1.0, **kw)
        assert sorted(res['output']) == ['clipped', 'gain', 'nonfinite', 'peak', 'peak_dbfs'] and sr.calls[-1][4] == {}
        recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all', **kw)
        assert [sorted(r) for r in recs] == [['channels', 'error', 'frames', 'metrics', 'out_frames', 'path', 'rate', 'written_channels']] * 2
        assert [c[3:] for c in sr.calls if c[0] == 'write'][-2:] == [(None, {})] * 2


def test_the_option_reaches_the_output_stage(stub, tmp_path):
    from pix2pixhdaudiosr_amd.generate import encoding_limit
    sr, src = stub
    ceiling = 10.0 ** (-1.0 / 20.0)
    res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', encoding='float32', clip='guard',
                          ceiling_dbfs=-1.0, limiter=True)
    assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'output', 'sr'] and torch.equal(res['sr'], 1.7 * res['lr'])
    assert sorted(res['output']) == ['clipped', 'gain', 'limiter', 'nonfinite', 'peak', 'peak_dbfs', 'true_peak', 'true_peak_dbtp']
    assert sorted(res['output']['limiter']) == ['hold', 'input_true_peak_dbtp', 'limited_samples', 'lookahead', 'max_reduction_db']
    _, path, encoding, stage, extra = sr.calls[-1]
    assert stage['clip'] == 'guard' and stage['ceiling'] == ceiling
    assert extra == {'true_peak': {'rate': 48000, 'ceiling': ceiling, 'limit': 1.0},       # the measurement is switched on with it
                     'limiter': {'lookahead': 240, 'hold': 960, 'rate': 48000, 'ceiling': ceiling}}
    # the ms options; the ceiling defaults to the encoding's limit; true_peak=True beside it changes nothing
    sr.enhance_file(str(src / "a.wav"), None, is_lr_input=True, encoding='pcm16', clip='guard', limiter=True, limiter_lookahead_ms=1.5,
                    limiter_hold_ms=0, true_peak=True)
    assert sr.calls[-1][4]['limiter'] == {'lookahead': 72, 'hold': 0, 'rate': 48000, 'ceiling': encoding_limit('pcm16')}
    assert sr.calls[-1][4]['true_peak']['ceiling'] == encoding_limit('pcm16')
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all', clip='guard', ceiling_dbfs=-1.0, limiter=True,
                             limiter_hold_ms=10.0)
    assert all(r['output']['limiter']['hold'] == 480 for r in recs)
    writes = [c for c in sr.calls if c[0] == 'write'][-2:]
    assert all(c[4]['limiter'] == {'lookahead': 240, 'hold': 480, 'rate': 48000, 'ceiling': ceiling} for c in writes)
    assert writes[0][4]['limiter'] is not writes[1][4]['limiter']                           # one file's: it takes the file's buffers


def test_refusals_come_before_a_file_is_read(stub, tmp_path):
    sr, src = stub
    n = len(sr.calls)
    for kw, word in ((dict(limiter=True), "clip='guard'"), (dict(limiter=True, clip='clamp'), "clip='guard'"),
                     (dict(limiter=True, clip='error'), "clip='guard'"), (dict(limiter=True, report_peaks=True), "clip='guard'"),
                     (dict(limiter=True, clip='limit'), "clip must be one of"),
                     (dict(limiter=1, clip='guard'), "limiter must be a bool"),
                     (dict(limiter_lookahead_ms=5.0, clip='guard'), "options of limiter=True"),
                     (dict(limiter_hold_ms=5.0), "options of limiter=True"),
                     (dict(limiter=True, clip='guard', limiter_lookahead_ms=30.0), "at most 21.3333 ms"),
                     (dict(limiter=True, clip='guard', limiter_hold_ms=-1.0), "hold_ms must be"),
                     (dict(limiter=True, clip='guard', true_peak='yes'), "true_peak must be a bool")):
        with pytest.raises(ValueError, match=word):
            sr.enhance_file(str(src / "a.wav"), str(tmp_path / "x.wav"), is_lr_input=True, **kw)
        with pytest.raises(ValueError, match=word):
            sr.enhance_folder(str(src), str(tmp_path / "out2"), is_lr_input=True, **kw)
    assert len(sr.calls) == n and not (tmp_path / "x.wav").exists() and not (tmp_path / "out2").exists()


def test_cli_options_and_refusals(capsys):
    from pix2pixhdaudiosr_amd.generate import _parser, main
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]
    a = _parser().parse_args(base)
    assert (a.limiter, a.limiter_lookahead_ms, a.limiter_hold_ms) == (False, None, None)
    b = _parser().parse_args(base + ["--clip", "guard", "--limiter", "--limiter_lookahead_ms", "1.5", "--limiter_hold_ms", "0"])
    assert (b.limiter, b.limiter_lookahead_ms, b.limiter_hold_ms) == (True, 1.5, 0.0)
    for extra, word in ((["--limiter"], "clip='guard'"), (["--limiter", "--clip", "error"], "clip='guard'"),
                        (["--limiter_hold_ms", "3"], "options of limiter=True"),
                        (["--clip", "guard", "--limiter", "--limiter_lookahead_ms", "30"], "at most 21.3333 ms")):
        with pytest.raises(SystemExit) as e:                      # ("ck" does not exist: loading anything would raise another error)
            main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_prints_one_line_per_file_and_adds_the_columns(stub, tmp_path, capsys):
    """The part of main() behind the model's construction, on the stub: --limiter prints the peak line and one limiter line per file
    and adds two columns; without it not a word about it and the table as it was."""
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_LIMITER, _parser, _run
    assert METRICS_COLUMNS_LIMITER == ("limiter_reduction_db", "limited_samples")
    sr, src = stub
    lines, tables = {}, {}
    for flag in ([], ["--limiter"]):
        for folder_mode, inp, out in ((False, src / "b.wav", tmp_path / "o.wav"), (True, src, tmp_path / "outdir")):
            csv_path = tmp_path / "m.csv"
            a = _parser().parse_args(["--input", str(inp), "--output", str(out), "--load_pretrain", "ck", "--is_lr_input", "--clip", "guard",
                                      "--metrics_csv", str(csv_path)] + flag)
            stage = dict(clip=a.clip, ceiling_dbfs=a.ceiling_dbfs, dither=a.dither, dither_seed=a.dither_seed, report_peaks=a.report_peaks)
            if flag:
                stage.update(limiter=True, limiter_lookahead_ms=a.limiter_lookahead_ms, limiter_hold_ms=a.limiter_hold_ms)
            assert _run(a, sr, stage, None, 48000, folder_mode) == 0
            lines[(bool(flag), folder_mode)] = capsys.readouterr().out.splitlines()
            with open(csv_path, newline="") as f:
                tables[(bool(flag), folder_mode)] = list(csv.reader(f))
    for folder_mode, files in ((False, 1), (True, 2)):
        plain, on = lines[(False, folder_mode)], lines[(True, folder_mode)]
        assert not any("limiter" in l or "peak" in l for l in plain)
        extra = [l for l in on if l not in plain]
        assert [l for l in on if l in plain] == plain and len(extra) == 2 * files
        # 16 of the 64 samples of a file: 25.0 %
        assert [l for l in extra if l.startswith("limiter")] == ["limiter: -3.80 dB at most, 25.0 % of the samples, true peak in +2.80 dBTP"] * files
        assert sum("true peak -0.90 dBTP" in l and "gain 0.999000" in l for l in extra) == files
        off_rows, on_rows = tables[(False, folder_mode)], tables[(True, folder_mode)]
        assert tuple(off_rows[0]) == METRICS_COLUMNS and tuple(on_rows[0]) == METRICS_COLUMNS + METRICS_COLUMNS_LIMITER
        assert [r[:-2] for r in on_rows] == off_rows


def test_metrics_rows_with_the_limiter_columns():
    from pix2pixhdaudiosr_amd.generate import metrics_rows
    m = lambda v: (v, v + 1, v + 2, 0, 0, 0, v + 3)
    lim = lambda db, n: {'limiter': {'lookahead': 240, 'hold': 960, 'max_reduction_db': db, 'limited_samples': n, 'input_true_peak_dbtp': 1.0},
                         'true_peak_dbtp': [0.5, 0.25]}
    recs = [{'path': 'a.wav', 'out_frames': 10, 'metrics': [m(1.0)], 'output': lim(-3.0, 5)},
            {'path': 'b.wav', 'out_frames': 20, 'metrics': [m(2.0), m(3.0)], 'output': lim(0.0, 0)},
            {'path': 'bad.wav', 'out_frames': 0, 'metrics': None, 'output': None}]
    old = metrics_rows(recs)
    assert old == metrics_rows(recs, limiter=False)
    new = metrics_rows(recs, limiter=True)
    assert [r[:-2] for r in new] == old and [r[-2:] for r in new] == [(-3.0, 5), (0.0, 0), (0.0, 0), (-1.0, 5 / 3)]
    both = metrics_rows(recs, true_peak=True, limiter=True)
    assert [r[-3:] for r in both[:3]] == [(0.5, -3.0, 5), (0.5, 0.0, 0), (0.25, 0.0, 0)]
