"""Host side of the output stage of whole-file generation (peak report, clip guard, dither): the numpy restatement
(tests/_outstage_ref.py) against the hash's known answers, the plain encoder's restatement (tests/_pcm_ref.py) and the ideal
triangular law; the validation of the new arguments in the API and on the command line; the peak columns of the metrics
table; and the result's keys when none of the new arguments is given."""
import numpy as np
import pytest
import torch

import _outstage_ref as O
import _pcm_ref as P

BASE = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]

# (seed, index) -> (h, d * 2^16): computed by hand from the recipe of include/p2phd.h
KNOWN = [(0, 0, 0xaa3e5b61, -20189), (0, 1, 0x6f0b28e6, -17957), (1, 0, 0x9941cd2d, 13292),
         (0x123456789abcdef0, 0, 0x13aaa200, 36438), (0, 2 ** 32 - 1, 0x82f01567, -28041), (0, 2 ** 32, 0x9941cd2d, 13292),
         (0x123456789abcdef0, 2 ** 40 + 12345, 0x5fbe1a37, -17799)]


@pytest.mark.parametrize("seed,index,h,d16", KNOWN)
def test_hash_known_answers(seed, index, h, d16):
    assert int(O.dither_hash(seed, index)) == h
    assert int(O.dither_lsb16(seed, index)) == d16
    d = O.dither(seed, np.array([index], dtype=np.uint64))
    assert d.dtype == np.float32 and float(d[0]) * 65536.0 == d16 and -1.0 < float(d[0]) < 1.0


def _edge_values():
    """+-1, hi, hi +- 1 ulp, -1 -+ 1 ulp, +-inf, NaN, denormals, zeros and every .5 tie around both limits, per format."""
    v = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-40, 3.4028235e38, -3.4028235e38]
    for bits in (16, 24):
        scale = np.float32(2 ** (bits - 1))
        hi = (scale - np.float32(1)) / scale
        for x in (hi, np.float32(-1)):
            v += [x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-2))]
        k = np.concatenate([np.arange(-scale - 4, -scale + 4), np.arange(-4, 4), np.arange(scale - 5, scale + 3)])
        v += list(((k + 0.5) / float(scale)).astype(np.float32)) + list((k / float(scale)).astype(np.float32))
    return np.array(v, dtype=np.float32)


@pytest.mark.parametrize("encoding", ["pcm16", "pcm24", "float32"])
def test_plain_restatements_agree(encoding):
    """No gain, no dither: clamping after the rounding gives the codes of clamping before it."""
    edge = _edge_values()
    rng = np.random.default_rng(3)
    x = np.concatenate([edge, rng.uniform(-1.5, 1.5, 4096).astype(np.float32)])
    x = x[:len(x) // 2 * 2].reshape(2, -1)
    assert O.encode_ex(x, encoding) == P.encode(x, encoding)
    assert O.encode_ex(P.encode_input(500, 3), encoding) == P.encode(P.encode_input(500, 3), encoding)


def test_peaks_restatement_on_a_hand_case():
    hi = O.hi_of("pcm16")
    x = np.array([[0.5, -1.0, hi, np.nan, 0.0], [1.5, -1.25, np.inf, -np.inf, np.nextafter(hi, np.float32(2))]], dtype=np.float32)
    peak, over, nonfinite, gain = O.peaks(x, "pcm16")
    assert peak.tolist() == [1.0, 1.5] and over.tolist() == [0, 5] and nonfinite.tolist() == [1, 2]
    assert gain == hi / np.float32(1.5) and gain.dtype == np.float32
    assert O.peaks(x, "float32")[1].tolist() == [0, 4] and O.peaks(x, "float32")[3] == np.float32(1) / np.float32(1.5)
    assert O.peaks(x, "pcm16", ceiling=0.5)[3] == np.float32(0.5) / np.float32(1.5)
    assert O.peaks(x[:1], "pcm16", ceiling=2.0)[3] == 1.0
    empty = O.peaks(np.zeros((2, 0), dtype=np.float32), "pcm24")
    assert empty[0].tolist() == [0, 0] and empty[1].tolist() == [0, 0] and empty[3] == 1.0
    assert O.peaks(np.full((1, 4), np.nan, dtype=np.float32), "pcm16")[0].tolist() == [0.0]


def test_tpdf_statistics():
    """2^20 consecutive indices against the ideal triangular law on (-1, 1): mean 0, variance 1/6, fourth moment 1/15, white.
    Bounds at 5 sigma of the estimators."""
    N = 1 << 20
    d = O.dither(0, np.arange(N, dtype=np.uint64)).astype(np.float64)
    assert d.min() > -1.0 and d.max() < 1.0
    mean, var = d.mean(), d.var()
    lag1 = np.mean((d[:-1] - mean) * (d[1:] - mean)) / var
    print(f"TPDF N = 2^20: mean {mean:.3e}, var {var:.6f}, lag-1 {lag1:.3e}")
    assert abs(mean) < 5 * np.sqrt(1 / (6 * N))
    assert abs(var - 1 / 6) < 5 * np.sqrt((1 / 15 - 1 / 36) / N)
    assert abs(lag1) < 5 / np.sqrt(N)
    # another seed is another stream
    other = O.dither(2 ** 63 + 5, np.arange(4096, dtype=np.uint64)).astype(np.float64)
    assert abs(np.corrcoef(other, d[:4096])[0, 1]) < 5 / np.sqrt(4096)


def test_dither_flips_ties_and_keeps_pieces():
    k = np.arange(-50, 50)
    x = ((k + 0.5) / 32768.0).astype(np.float32)[None]
    plain = np.frombuffer(O.encode_ex(x, "pcm16"), dtype="<i2")
    dith = np.frombuffer(O.encode_ex(x, "pcm16", tpdf=True, seed=7), dtype="<i2")
    assert np.abs(dith.astype(int) - plain).max() == 1 and 20 < np.count_nonzero(dith != plain) < 80
    y = P.encode_input(301, 2)
    whole = O.encode_ex(y, "pcm16", tpdf=True, seed=9, first_index=2 ** 32 - 100)
    parts = O.encode_ex(y[:, :100], "pcm16", tpdf=True, seed=9, first_index=2 ** 32 - 100) + \
        O.encode_ex(y[:, 100:], "pcm16", tpdf=True, seed=9, first_index=2 ** 32 - 100 + 200)
    assert whole == parts
    with pytest.raises(ValueError):
        O.encode_ex(y, "pcm24", tpdf=True)


# ------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------
def test_check_output_options():
    from pix2pixhdaudiosr_amd.generate import ceiling_from_dbfs, check_output_options, encoding_limit
    assert check_output_options("pcm16") is None and check_output_options("float32", "clamp", None, None, 0, False) is None
    st = check_output_options("pcm16", clip="guard", ceiling_dbfs=-1.0, dither="tpdf", dither_seed=3, report_peaks=True)
    assert st == {'clip': 'guard', 'ceiling': 10.0 ** (-1.0 / 20.0), 'dither': 'tpdf', 'seed': 3, 'report': True}
    assert check_output_options("pcm24", report_peaks=True) == {'clip': 'clamp', 'ceiling': None, 'dither': None, 'seed': 0, 'report': True}
    assert check_output_options("pcm16", dither_seed=5) is not None
    assert encoding_limit("pcm16") == 32767 / 32768 and encoding_limit("pcm24") == 8388607 / 8388608 and encoding_limit("float32") == 1.0
    # a level at or above the encoding's limit is the limit itself
    assert ceiling_from_dbfs(0.0, "pcm16") is None and ceiling_from_dbfs(0, "float32") is None and ceiling_from_dbfs(None, "pcm16") is None
    assert ceiling_from_dbfs(-6.0, "float32") == 10.0 ** (-6.0 / 20.0)
    for kw, word in ((dict(encoding="pcm24", dither="tpdf"), "pcm16"), (dict(encoding="float32", dither="tpdf"), "pcm16"),
                     (dict(encoding="pcm16", dither="rect"), "dither"), (dict(encoding="pcm16", clip="limit"), "clip"),
                     (dict(encoding="pcm16", clip="guard", ceiling_dbfs=0.5), "ceiling_dbfs"),
                     (dict(encoding="pcm16", clip="guard", ceiling_dbfs=float("nan")), "ceiling_dbfs"),
                     (dict(encoding="pcm16", ceiling_dbfs=-1.0), "guard"), (dict(encoding="pcm16", clip="error", ceiling_dbfs=-1.0), "guard"),
                     (dict(encoding="pcm16", dither_seed=1.5), "dither_seed"), (dict(encoding="pcm8"), "encoding")):
        with pytest.raises(ValueError, match=word):
            check_output_options(**kw)


def _stub_resolver():
    """SuperResolver with every device step replaced: the clip is 'decoded' from a tensor, 'enhanced' by a factor and the
    output stage records its arguments -- what is left is the plumbing of the arguments and of the result's keys."""
    from types import SimpleNamespace
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

        def _write(self, path_out, sr, encoding, stage=None):
            self.calls.append(('write', path_out, encoding, stage))
            return None if stage is None else {'peak': [1.7] * sr.shape[0], 'peak_dbfs': [4.6] * sr.shape[0],
                                               'clipped': [3] * sr.shape[0], 'nonfinite': [0] * sr.shape[0], 'gain': 0.5}
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


def test_result_keys_do_not_move_without_the_new_arguments(stub, tmp_path):
    sr, src = stub
    res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all')
    assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'sr']
    assert sr.calls[-1] == ('write', str(tmp_path / "o.wav"), 'pcm16', None)
    assert sorted(sr.enhance_file(str(src / "b.wav"), None, is_lr_input=True)) == ['hr', 'info', 'lr', 'metrics', 'sr']
    assert sr.calls[-1][0] == 'read'                              # no output file, no stage: nothing is encoded
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all')
    assert [sorted(r) for r in recs] == [['channels', 'error', 'frames', 'metrics', 'out_frames', 'path', 'rate', 'written_channels']] * 2
    assert [c[3] for c in sr.calls if c[0] == 'write'][-2:] == [None, None]


def test_new_arguments_reach_the_output_stage(stub, tmp_path):
    sr, src = stub
    res = sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, channels='all', clip='guard',
                          ceiling_dbfs=-1.0, dither='tpdf', dither_seed=11, report_peaks=True)
    assert sorted(res) == ['hr', 'info', 'lr', 'metrics', 'output', 'sr']
    assert res['output']['gain'] == 0.5 and len(res['output']['peak']) == 2
    assert sr.calls[-1][3] == {'clip': 'guard', 'ceiling': 10.0 ** (-1.0 / 20.0), 'dither': 'tpdf', 'seed': 11, 'report': True}
    assert torch.equal(res['sr'], 1.7 * res['lr'])               # the returned clip is the unscaled one
    # measuring without a file to write
    only = sr.enhance_file(str(src / "a.wav"), None, is_lr_input=True, report_peaks=True)
    assert 'output' in only and sr.calls[-1][:2] == ('write', None)
    # a folder: file k of the plan is dithered with seed + k
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, dither='tpdf', dither_seed=100)
    assert all('output' in r for r in recs)
    assert [c[3]['seed'] for c in sr.calls if c[0] == 'write'][-2:] == [100, 101]
    # bad combinations are refused before the file is read
    n = len(sr.calls)
    for kw in (dict(encoding='pcm24', dither='tpdf'), dict(encoding='float32', dither='tpdf'), dict(clip='guard', ceiling_dbfs=3.0),
               dict(ceiling_dbfs=-3.0), dict(clip='soft')):
        with pytest.raises(ValueError):
            sr.enhance_file(str(src / "a.wav"), str(tmp_path / "x.wav"), is_lr_input=True, **kw)
        with pytest.raises(ValueError):
            sr.enhance_folder(str(src), str(tmp_path / "out2"), is_lr_input=True, **kw)
    assert len(sr.calls) == n and not (tmp_path / "x.wav").exists() and not (tmp_path / "out2").exists()


def test_clip_error_is_a_value_error_and_passes_through(stub, tmp_path):
    from pix2pixhdaudiosr_amd.generate import ClipError
    assert issubclass(ClipError, ValueError)
    sr, src = stub
    raised = ClipError("o.wav: 3 samples would clip")

    def refuse(path_out, clip, encoding, stage=None):
        raise raised
    sr._write = refuse
    with pytest.raises(ClipError) as e:
        sr.enhance_file(str(src / "b.wav"), str(tmp_path / "o.wav"), is_lr_input=True, clip='error')
    assert e.value is raised
    with pytest.raises(ClipError) as e:
        sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, clip='error')
    assert e.value is raised


def test_cli_options():
    from pix2pixhdaudiosr_amd.generate import _parser, main
    a = _parser().parse_args(BASE)
    assert (a.clip, a.ceiling_dbfs, a.dither, a.dither_seed, a.report_peaks) == ("clamp", None, None, 0, False)
    b = _parser().parse_args(BASE + ["--clip", "guard", "--ceiling_dbfs", "-1.5", "--dither", "tpdf", "--dither_seed", "42", "--report_peaks"])
    assert (b.clip, b.ceiling_dbfs, b.dither, b.dither_seed, b.report_peaks) == ("guard", -1.5, "tpdf", 42, True)


@pytest.mark.parametrize("extra,word", [(["--dither", "tpdf", "--encoding", "pcm24"], "pcm16"),
                                        (["--dither", "tpdf", "--encoding", "float32"], "pcm16"),
                                        (["--clip", "guard", "--ceiling_dbfs", "0.5"], "ceiling_dbfs"),
                                        (["--ceiling_dbfs", "-1"], "guard"),
                                        (["--clip", "error", "--ceiling_dbfs", "-1"], "guard"),
                                        (["--clip", "soft"], "--clip"), (["--dither", "rect"], "--dither")])
def test_cli_rejects_bad_combinations_before_the_model_loads(extra, word, capsys):
    from pix2pixhdaudiosr_amd.generate import main
    with pytest.raises(SystemExit) as e:                          # ("ck" does not exist: loading anything would raise another error)
        main(BASE + extra)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_cli_prints_one_line_per_file_and_adds_the_columns(stub, tmp_path, capsys):
    """The part of main() behind the model's construction, on the stub: --report_peaks prints a line per file and adds the
    three columns; without it not a word about peaks."""
    import csv
    from pix2pixhdaudiosr_amd.generate import _parser, _run
    sr, src = stub
    lines = {}
    for flag in ([], ["--report_peaks"]):
        for folder_mode, inp, out in ((False, src / "b.wav", tmp_path / "o.wav"), (True, src, tmp_path / "outdir")):
            csv_path = tmp_path / "m.csv"
            a = _parser().parse_args(["--input", str(inp), "--output", str(out), "--load_pretrain", "ck", "--is_lr_input",
                                      "--metrics_csv", str(csv_path)] + flag)
            stage = dict(clip=a.clip, ceiling_dbfs=a.ceiling_dbfs, dither=a.dither, dither_seed=a.dither_seed, report_peaks=a.report_peaks)
            assert _run(a, sr, stage, None, 48000, folder_mode) == 0
            lines[(bool(flag), folder_mode)] = capsys.readouterr().out.splitlines()
            with open(csv_path, newline="") as f:
                header = next(csv.reader(f))
            assert header[-3:] == (["peak_dbfs", "clipped", "gain"] if flag else ["snr_sr", "snr_lr", "lsd"])
    for folder_mode, files in ((False, 1), (True, 2)):
        plain, rep = lines[(False, folder_mode)], lines[(True, folder_mode)]
        assert not any("peak" in l or "clipped" in l for l in plain)
        extra = [l for l in rep if l not in plain]
        assert len(extra) == files and all("peak +4.60 dBFS" in l and "clipped" in l and "gain 0.500000" in l for l in extra)
        assert [l for l in rep if l in plain] == plain


# ------------------------------------------------------------------------------------------
# the metrics table
# ------------------------------------------------------------------------------------------
def _records():
    m = lambda v: (v, v + 1, v + 2, 0, 0, 0, v + 3)
    e = lambda v: dict(mse=v, snr_sr=v + 1, snr_lr=v + 2, lsd=v + 3, lsd_lf=v + 4, lsd_hf=v + 5, ssnr_sr=v + 6, ssnr_lr=v + 7)
    return [{'path': 'a.wav', 'out_frames': 10, 'metrics': [m(1.0)], 'metrics_ext': [e(1.0)],
             'output': {'peak': [0.5], 'peak_dbfs': [-6.0], 'clipped': [0], 'nonfinite': [0], 'gain': 1.0}},
            {'path': 'b.wav', 'out_frames': 20, 'metrics': [m(2.0), m(3.0)], 'metrics_ext': [e(2.0), e(3.0)],
             'output': {'peak': [1.7, 1.0], 'peak_dbfs': [4.5, 0.0], 'clipped': [7, 1], 'nonfinite': [0, 0], 'gain': 0.5}},
            {'path': 'c.wav', 'out_frames': 30, 'metrics': None, 'metrics_ext': None,
             'output': {'peak': [0.1], 'peak_dbfs': [-20.0], 'clipped': [0], 'nonfinite': [0], 'gain': 1.0}},
            {'path': 'bad.wav', 'out_frames': 0, 'metrics': None, 'metrics_ext': None, 'output': None}]


@pytest.mark.parametrize("extended", [False, True])
def test_metrics_rows_with_peaks(extended, tmp_path):
    import csv
    from pix2pixhdaudiosr_amd.generate import METRICS_COLUMNS, METRICS_COLUMNS_EXT, METRICS_COLUMNS_PEAKS, metrics_rows, write_metrics_csv
    recs = _records()
    assert METRICS_COLUMNS_PEAKS == ("peak_dbfs", "clipped", "gain")
    old = metrics_rows(recs, extended)
    assert old == metrics_rows(recs, extended, peaks=False)
    new = metrics_rows(recs, extended, peaks=True)
    assert [r[:-3] for r in new] == old and len(new) == 4
    assert [r[-3:] for r in new] == [(-6.0, 0, 1.0), (4.5, 7, 0.5), (0.0, 1, 0.5), (-1.5 / 3, 8 / 3, 2.0 / 3)]
    assert metrics_rows(recs[2:], extended, peaks=True) == []
    base = METRICS_COLUMNS_EXT if extended else METRICS_COLUMNS
    for peaks in (False, True):
        path = str(tmp_path / f"m{int(peaks)}.csv")
        write_metrics_csv(path, recs, extended, peaks) if peaks else write_metrics_csv(path, recs, extended)
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        assert tuple(rows[0]) == base + (METRICS_COLUMNS_PEAKS if peaks else ())
        assert all(len(r) == len(rows[0]) for r in rows) and len(rows) == 5


ROWS = [('a.wav', 0, 10, 1.0, 2.0, 3.0, 4.0), ('b.wav', 0, 20, 2.0, 3.0, 4.0, 5.0), ('b.wav', 1, 20, 3.0, 4.0, 5.0, 6.0),
        ('mean', '', '', 2.0, 3.0, 4.0, 5.0)]
ROWS_EXT = [(5.0, 6.0, 7.0, 8.0), (6.0, 7.0, 8.0, 9.0), (7.0, 8.0, 9.0, 10.0), (6.0, 7.0, 8.0, 9.0)]
ROWS_PEAKS = [(-6.0, 0, 1.0), (4.5, 7, 0.5), (0.0, 1, 0.5), (-0.5, 2.6666666666666665, 0.6666666666666666)]


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("peaks", [False, True])
def test_metrics_rows_fixed_table(extended, peaks):
    """The rows of _records() as the table was before metrics_rows became one loop over its columns, value for value."""
    from pix2pixhdaudiosr_amd.generate import metrics_rows
    want = [r + (e if extended else ()) + (p if peaks else ()) for r, e, p in zip(ROWS, ROWS_EXT, ROWS_PEAKS)]
    got = metrics_rows(_records(), extended, peaks)
    assert got == want and [[type(v) for v in r] for r in got] == [[type(v) for v in r] for r in want]
    # the means of the two tables differ on a NaN: it propagates in the basic one and is left out in the extended one
    recs = _records()
    recs[0]['metrics'] = [(float('nan'),) + recs[0]['metrics'][0][1:]]
    recs[0]['metrics_ext'][0]['mse'] = float('nan')
    mean = metrics_rows(recs, extended, peaks)[-1]
    assert (mean[3] == 2.5) if extended else (mean[3] != mean[3])
    assert mean[4:] == want[-1][4:]
