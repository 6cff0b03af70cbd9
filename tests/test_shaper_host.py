"""The host side of the noise-shaped dither (csrc/shaper.hip: p2phd_shaper_taps_fill, p2phd_shaper_tile_len; generate.check_dither,
check_output_options, shaper_coefficients, the command line) and the contract itself, on its numpy restatement
tests/_shaper_ref.py, without a GPU: the tables, zero taps = TPDF, the bound on the error while a passage clips, non-finite samples,
every refusal, and the spectral figures of the issue -- a 997 Hz sine at 0.25 of full scale, 2^18 samples, Welch with 8192-point
Hann windows at hop 4096, mean noise power per band in dB re 1 LSB^2."""
import ctypes

import numpy as np
import pytest
import torch

import _outstage_ref as O
import _shaper_ref as R

BASE = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]


# ------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------
def test_tables_are_the_literals_rounded_once():
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.generate import DITHER_CHUNK, DITHER_CURVES, DITHERS, SHAPED_RATES, shaper_coefficients
    assert DITHERS == (None, 'tpdf', 'shaped') and DITHER_CHUNK == 4096 and SHAPED_RATES == (44100, 48000)
    assert DITHER_CURVES == R.CURVE_IDS and next(iter(DITHER_CURVES)) == 'lipshitz9'
    for name, lits in R.CURVES.items():
        h = shaper_coefficients(name)
        assert h.dtype == torch.float32 and not h.is_cuda and h.numel() == len(lits)
        assert np.array_equal(h.numpy(), np.array([np.float32(v) for v in lits]))
    with pytest.raises(ValueError, match="curve"):
        shaper_coefficients('f9')
    L = _lib.lib()
    buf = np.zeros(16, dtype=np.float32)
    K = ctypes.c_int32(0)
    einval = L.p2phd_shaper_taps_fill(3, ctypes.c_void_p(buf.ctypes.data), ctypes.byref(K))
    assert einval != 0 and b"shaper_taps_fill" in L.p2phd_last_error()
    assert L.p2phd_shaper_taps_fill(-1, ctypes.c_void_p(buf.ctypes.data), ctypes.byref(K)) == einval
    assert L.p2phd_shaper_taps_fill(0, None, ctypes.byref(K)) == einval and L.p2phd_shaper_taps_fill(0, ctypes.c_void_p(buf.ctypes.data), None) == einval
    assert L.p2phd_shaper_taps_fill(1, ctypes.c_void_p(buf.ctypes.data), ctypes.byref(K)) == 0 and K.value == 5 and not buf[5:].any()
    assert L.p2phd_shaper_tile_len(1, 4096) > 0 and L.p2phd_shaper_tile_len(65535, 1 << 20) > 0
    for bad in ((0, 4096), (65536, 4096), (1, 100), (1, 4100), (1, 1 << 21), (1, 0)):
        assert L.p2phd_shaper_tile_len(*bad) == -1 and b"shaper_tile_len" in L.p2phd_last_error(), bad


# ------------------------------------------------------------------------------------------
# the contract, on the restatement
# ------------------------------------------------------------------------------------------
def _clip(C, F, seed=1, level=0.5):
    return np.random.default_rng(seed).uniform(-level, level, (C, F)).astype(np.float32)


def test_zero_taps_are_the_tpdf_encoder():
    x = _clip(3, 700, level=1.2)
    x[0, 5], x[1, 300], x[2, 699], x[2, 0] = np.float32("nan"), np.float32("inf"), np.float32("-inf"), np.float32(-0.0)
    for chunk in (256, 320, 1024):
        for seed, first in ((0, 0), ((1 << 40) + 3, 5 * chunk * 3)):
            for gain in (None, 0.37):
                want = O.encode_ex(x, "pcm16", gain=gain, tpdf=True, seed=seed, first_index=first)
                for taps in ((), (0.0,) * 9):
                    got = R.encode_shaped(x, taps, chunk, gain=gain, seed=seed, first_index=first)
                    assert got['bytes'] == want and not got['tie'], (chunk, seed, gain, len(taps))
    assert R.encode_shaped(x[:, :0], (), 256)['bytes'] == b""
    with pytest.raises(ValueError, match="first_index"):
        R.encode_shaped(x, (), 256, first_index=3)


@pytest.mark.parametrize("curve", sorted(R.CURVES))
def test_the_error_stays_bounded_while_a_passage_clips(curve):
    """e comes from the unclamped r: |e| <= 0.5 + |d| < 1.5 whatever the signal does, so a passage that clips winds nothing up."""
    x = _clip(1, 3000, seed=4, level=0.3)
    x[0, 700:1700] = 3.0                                           # 1000 samples far beyond full scale, across a chunk boundary
    x[0, 2000:2100] = -3.0
    o = R.encode_shaped(x, R.taps_of(curve), 1024, seed=3)
    q = np.frombuffer(o['bytes'], dtype="<i2")
    assert np.abs(o['e']).max() <= 1.5
    assert (q[700:1700] == 32767).all() and (q[2000:2100] == -32768).all()
    bound = 1.5 * (1.0 + np.abs(R.taps_of(curve)).sum())          # |stored - v| <= |e| + sum |h| |e|
    for lo, hi in ((0, 700), (1700, 2000), (2100, 3000)):          # the first sample behind the passage is as close as any other
        assert np.abs(q[lo:hi] - o['v'][0, lo:hi]).max() <= bound


def test_non_finite_samples_store_what_the_contract_says_and_the_history_recovers():
    taps = R.taps_of('lipshitz9')
    x = _clip(1, 1024, seed=6, level=0.3)
    clean = R.encode_shaped(x, taps, 512, seed=1)
    x[0, 100], x[0, 200], x[0, 300] = np.float32("nan"), np.float32("inf"), np.float32("-inf")
    o = R.encode_shaped(x, taps, 512, seed=1)
    q, q0 = np.frombuffer(o['bytes'], dtype="<i2"), np.frombuffer(clean['bytes'], dtype="<i2")
    assert (q[100], q[200], q[300]) == (0, 32767, -32768)
    assert np.isfinite(o['e']).all() and np.abs(o['e']).max() <= 1.5 and (o['e'][0, [100, 200, 300]] == 0).all()
    assert np.array_equal(q[:100], q0[:100]) and np.array_equal(q[512:], q0[512:])          # the samples before it, and the next chunk
    bound = 1.5 * (1.0 + np.abs(taps).sum())
    rest = np.ones(512, dtype=bool)
    rest[[100, 200, 300]] = False
    assert np.abs(q[:512][rest] - o['v'][0, :512][rest]).max() <= bound


# ------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------
def test_check_dither_and_the_stage():
    from pix2pixhdaudiosr_amd.generate import check_dither, check_output_options
    assert check_dither(None, "pcm24", "who") is None and check_dither('tpdf', "pcm16", "who") is None
    assert check_dither('shaped', "pcm16", "who") is None and check_dither('shaped', "pcm16", "who", 44100, 'e5', 256) is None
    assert check_dither('shaped', "pcm16", "who", 48000, None, 1 << 20) is None and check_dither('tpdf', "pcm16", "who", 16000) is None
    for args, word in ((('shaped', "pcm24", "who"), "pcm16"), (('shaped', "float32", "who"), "pcm16"),
                       (('shaped', "pcm16", "who", 32000), "44100 or 48000"), (('shaped', "pcm16", "who", 16000), "44100 or 48000"),
                       (('shaped', "pcm16", "who", 48000, 'f9'), "dither_curve"), (('shaped', "pcm16", "who", 48000, None, 100), "dither_chunk"),
                       (('shaped', "pcm16", "who", 48000, None, 4100), "dither_chunk"), (('shaped', "pcm16", "who", 48000, None, 1 << 21), "dither_chunk"),
                       (('shaped', "pcm16", "who", None, None, 4096.0), "dither_chunk"), (('shaped', "pcm16", "who", None, None, True), "dither_chunk"),
                       (('tpdf', "pcm16", "who", None, 'e5'), "dither='shaped'"), ((None, "pcm16", "who", None, None, 4096), "dither='shaped'"),
                       (('rect', "pcm16", "who"), "dither must")):
        with pytest.raises(ValueError, match="who: .*" + word):
            check_dither(*args)
    # the stage carries the two values only with 'shaped'
    assert check_output_options("pcm16", dither='tpdf') == {'clip': 'clamp', 'ceiling': None, 'dither': 'tpdf', 'seed': 0, 'report': False}
    assert check_output_options("pcm16", dither='shaped') == {'clip': 'clamp', 'ceiling': None, 'dither': 'shaped', 'seed': 0, 'report': False,
                                                             'curve': 'lipshitz9', 'chunk': 4096}
    st = check_output_options("pcm16", 'guard', -1.0, 'shaped', 7, True, "who", 'light3', 512)
    assert (st['curve'], st['chunk'], st['seed'], st['clip']) == ('light3', 512, 7, 'guard')
    for kw, word in ((dict(dither='shaped', dither_curve='x'), "dither_curve"), (dict(dither='shaped', dither_chunk=100), "dither_chunk"),
                     (dict(dither='tpdf', dither_curve='e5'), "shaped"), (dict(dither_chunk=4096), "shaped"),
                     (dict(dither='shaped', encoding="pcm24"), "pcm16")):
        with pytest.raises(ValueError, match=word):
            check_output_options(**dict(dict(encoding="pcm16"), **kw))


def _stub_resolver(rate):
    from types import SimpleNamespace
    from pix2pixhdaudiosr_amd.generate import SuperResolver

    class Stub(SuperResolver):
        def __init__(self):
            self.opt = SimpleNamespace(lr_sampling_rate=rate // 4, hr_sampling_rate=rate)
            self.device = torch.device("cpu")
            self.calls = []

        def _read(self, path, slot='in0'):
            from pix2pixhdaudiosr_amd.data import wavio
            self.calls.append(('read', path))
            return torch.zeros(0, dtype=torch.uint8), wavio.info(path), slot

        def _decode(self, host, meta, slot):
            return torch.linspace(-1, 1, meta.num_frames)[None].repeat(meta.num_channels, 1)

        def enhance_lr(self, lr_audio, noise=None):
            return 0.5 * lr_audio

        def _write(self, path_out, sr, encoding, stage=None):
            self.calls.append(('write', path_out, encoding, stage))
            return None if stage is None else {'peak': [0.5], 'peak_dbfs': [-6.0], 'clipped': [0], 'nonfinite': [0], 'gain': 1.0}
    return Stub()


@pytest.fixture
def folder(tmp_path, monkeypatch):
    from pix2pixhdaudiosr_amd.data import audio_dataset, wavio
    monkeypatch.setattr(audio_dataset, "lr_round_trip", lambda raw, *a, **k: raw)
    src = tmp_path / "in"
    src.mkdir()
    for name in ("a.wav", "b.wav"):
        wavio.save(str(src / name), torch.zeros(1, 64), 16000)
    return src


def test_the_options_reach_the_output_stage_and_bad_ones_open_no_file(folder, tmp_path):
    sr = _stub_resolver(48000)
    sr.enhance_file(str(folder / "a.wav"), str(tmp_path / "o.wav"), is_lr_input=True, dither='shaped', dither_seed=5)
    assert sr.calls[-1][3] == {'clip': 'clamp', 'ceiling': None, 'dither': 'shaped', 'seed': 5, 'report': False, 'curve': 'lipshitz9', 'chunk': 4096}
    sr.enhance_file(str(folder / "a.wav"), str(tmp_path / "o.wav"), is_lr_input=True, dither='shaped', dither_curve='e5', dither_chunk=1024)
    assert (sr.calls[-1][3]['curve'], sr.calls[-1][3]['chunk']) == ('e5', 1024)
    sr.enhance_file(str(folder / "a.wav"), str(tmp_path / "o.wav"), is_lr_input=True, dither='tpdf')
    assert sorted(sr.calls[-1][3]) == ['ceiling', 'clip', 'dither', 'report', 'seed']
    # a folder: file k of the plan is dithered with seed + k, curve and chunk alike for all
    sr.enhance_folder(str(folder), str(tmp_path / "out"), is_lr_input=True, dither='shaped', dither_seed=100, dither_chunk=512)
    assert [(c[3]['seed'], c[3]['chunk'], c[3]['curve']) for c in [c for c in sr.calls if c[0] == 'write'][-2:]] == [(100, 512, 'lipshitz9'), (101, 512, 'lipshitz9')]
    n = len(sr.calls)
    bad = (dict(dither='shaped', encoding='pcm24'), dict(dither='shaped', dither_curve='f9'), dict(dither='shaped', dither_chunk=100),
           dict(dither='shaped', dither_chunk=4100), dict(dither='shaped', dither_chunk=1 << 21), dict(dither='tpdf', dither_curve='e5'),
           dict(dither_chunk=4096), dict(dither='shaped', output_rate=32000), dict(dither='shaped', output_rate=16000))
    for kw in bad:
        with pytest.raises(ValueError):
            sr.enhance_file(str(folder / "a.wav"), str(tmp_path / "x.wav"), is_lr_input=True, **kw)
        with pytest.raises(ValueError):
            sr.enhance_folder(str(folder), str(tmp_path / "out2"), is_lr_input=True, **kw)
    assert len(sr.calls) == n and not (tmp_path / "x.wav").exists() and not (tmp_path / "out2").exists()
    # the rate that counts is the written one: a model at 16 kHz is refused, the same model written at 44100 Hz is not
    low = _stub_resolver(16000)
    with pytest.raises(ValueError, match="44100 or 48000"):
        low.enhance_file(str(folder / "a.wav"), str(tmp_path / "x.wav"), is_lr_input=True, dither='shaped')
    with pytest.raises(ValueError, match="44100 or 48000"):
        low.enhance_folder(str(folder), str(tmp_path / "out2"), is_lr_input=True, dither='shaped')
    assert low.calls == [] and not (tmp_path / "x.wav").exists() and not (tmp_path / "out2").exists()
    low.enhance_file(str(folder / "a.wav"), str(tmp_path / "x.wav"), is_lr_input=True, dither='tpdf')      # (tpdf: any rate, as before)


def test_cli_options():
    from pix2pixhdaudiosr_amd.generate import _parser
    a = _parser().parse_args(BASE)
    assert (a.dither, a.dither_curve, a.dither_chunk) == (None, None, None)
    b = _parser().parse_args(BASE + ["--dither", "shaped", "--dither_curve", "e5", "--dither_chunk", "1024"])
    assert (b.dither, b.dither_curve, b.dither_chunk) == ("shaped", "e5", 1024)
    assert _parser().parse_args(BASE + ["--dither", "tpdf"]).dither == "tpdf"


@pytest.mark.parametrize("extra,word", [(["--dither", "shaped", "--encoding", "pcm24"], "pcm16"),
                                        (["--dither", "shaped", "--encoding", "float32"], "pcm16"),
                                        (["--dither", "shaped", "--output_rate", "32000"], "44100 or 48000"),
                                        (["--dither", "shaped", "--output_rate", "16000"], "44100 or 48000"),
                                        (["--dither", "shaped", "--dither_curve", "f9"], "--dither_curve"),
                                        (["--dither", "shaped", "--dither_chunk", "100"], "dither_chunk"),
                                        (["--dither", "shaped", "--dither_chunk", "4100"], "dither_chunk"),
                                        (["--dither", "shaped", "--dither_chunk", "2097152"], "dither_chunk"),
                                        (["--dither", "tpdf", "--dither_curve", "e5"], "shaped"),
                                        (["--dither_chunk", "4096"], "shaped"), (["--dither", "shape"], "--dither")])
def test_cli_rejects_bad_combinations_before_the_model_loads(extra, word, capsys):
    from pix2pixhdaudiosr_amd.generate import main
    with pytest.raises(SystemExit) as e:                          # ("ck" does not exist: loading anything would raise another error)
        main(BASE + extra)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_start_up_line():
    from pix2pixhdaudiosr_amd.generate import check_output_options, dither_line, shaper_coefficients
    st = check_output_options("pcm16", dither='shaped')
    assert dither_line(st, shaper_coefficients(st['curve']).numel()) == 'dither: shaped (lipshitz9, 9 taps, chunks of 4096)'


# ------------------------------------------------------------------------------------------
# the spectral figures
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def figures():
    """One run per row of the table, each at one seed, shared by the checks below."""
    cache = {}

    def get(curve, rate, chunk):
        key = (curve, rate, chunk)
        if key not in cache:
            x = R.sine(rate)
            o = R.encode_shaped(x, R.taps_of(curve) if curve else (), chunk, seed=0)
            cache[key] = dict(R.noise_figures(o['bytes'], o['v'], rate), emax=float(np.abs(o['e']).max()))
            print("%s %d Hz chunk %d: %s" % (curve, rate, chunk, ", ".join("%s %+.2f" % kv for kv in sorted(cache[key].items()))))
        return cache[key]
    return get


def test_tpdf_floor_is_flat(figures):
    f = figures(None, 48000, 4096)
    for band in ('mid', 'low', 'high', 'total'):
        assert abs(f[band] - 10.0 * np.log10(0.25)) < 0.25, (band, f)       # 1/12 + 1/6 LSB^2: -6.02 dB in every band


def test_lipshitz9_at_the_default_chunk(figures):
    """Measured with this restatement at seed 0: 2-5 kHz -25.23 dB (19.2 dB under TPDF; -25.00 .. -25.66 over seeds 0 .. 7), 0.1-1 kHz
    -17.99, 15-22 kHz +14.25, total +12.39 (18.4 dB over TPDF)."""
    f, z = figures('lipshitz9', 48000, 4096), figures(None, 48000, 4096)
    assert f['mid'] <= z['mid'] - 18.0, (f, z)
    assert z['total'] + 17.0 <= f['total'] <= z['total'] + 20.0, (f, z)
    assert f['high'] > 10.0 and f['emax'] <= 1.5


def test_lipshitz9_sequential(figures):
    """A chunk as long as the clip is the plain recursion.  Measured at seed 0: 2-5 kHz -28.05 dB, 22.0 dB under TPDF."""
    f, z = figures('lipshitz9', 48000, 1 << 18), figures(None, 48000, 4096)
    assert f['mid'] <= z['mid'] - 20.0, (f, z)
    assert z['total'] + 17.0 <= f['total'] <= z['total'] + 20.0, (f, z)
    assert f['mid'] < figures('lipshitz9', 48000, 4096)['mid'] and f['emax'] <= 1.5       # chunking costs depth, never stability


def test_lipshitz9_at_44100(figures):
    f, z = figures('lipshitz9', 44100, 4096), figures(None, 44100, 4096)
    assert f['mid'] <= z['mid'] - 18.0 and z['total'] + 17.0 <= f['total'] <= z['total'] + 20.0, (f, z)


def test_light3(figures):
    """Measured at seed 0, chunk 4096: 2-5 kHz -22.56 dB (16.5 dB under TPDF), total +0.63 dB (6.6 dB over)."""
    f, z = figures('light3', 48000, 4096), figures(None, 48000, 4096)
    assert f['mid'] <= z['mid'] - 15.0 and f['total'] <= z['total'] + 8.0 and f['emax'] <= 1.5, (f, z)


def test_e5(figures):
    """The issue sets no figure for this curve, so it is held to the linear model (R.model_figures: 2-5 kHz -24.58 dB, 15-22 kHz +9.03,
    total +6.17): the total and the hump within 0.5 dB (the estimator's spread over seeds is 0.2 - 0.4 dB), the dip no deeper than
    that and at most 2.0 dB shallower -- a chunk of 4096 leaks the hump into it at -36 dB re the hump, here
    -27 dB beside the model's -24.6.  Measured at seed 0: -24.06, +9.05, +6.17."""
    f, m = figures('e5', 48000, 4096), R.model_figures('e5', 48000)
    assert abs(f['total'] - m['total']) <= 0.5 and abs(f['high'] - m['high']) <= 0.5, (f, m)
    assert m['mid'] - 0.5 <= f['mid'] <= m['mid'] + 2.0 and f['emax'] <= 1.5, (f, m)


def test_the_sequential_recursion_follows_the_linear_model(figures):
    """Every band of the unchunked run within 0.5 dB of white noise of 1/4 LSB^2 through 1 - sum h[k] z^-k: the sign convention and the
    tap order of the contract, checked against the published shape."""
    f, m = figures('lipshitz9', 48000, 1 << 18), R.model_figures('lipshitz9', 48000)
    for band in ('mid', 'low', 'high', 'total'):
        assert abs(f[band] - m[band]) <= 0.5, (band, f, m)
    assert abs(m['total'] - figures(None, 48000, 4096)['total'] - 18.4) < 0.1          # 10 log10(1 + sum h^2)
