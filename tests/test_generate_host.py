"""Host side of whole-file generation (pix2pixhdaudiosr_amd/generate.py): segment arithmetic against the numpy
restatement (tests/_generate_ref.py) and the reference's seg_pad_audio count, the options-dump parser on the reference's
own four dumps (tests/golden/opt_*.txt), and the two image helpers the reference's Visualizer needs from util.util."""
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import _generate_ref as R
from conftest import GOLDEN

T = 992                                     # 31 * 32: the segment of the tiny geometry


@pytest.mark.parametrize("overlap", [0, 0.1, 0.25, 0.5])
@pytest.mark.parametrize("L", [1, T - 1, T, T + 1, 3 * T, 3 * T + 5])
def test_segment_plan(L, overlap):
    from pix2pixhdaudiosr_amd.generate import segment_plan
    S, stride, V = segment_plan(L, T, overlap)
    assert V == int(overlap * T) and stride == T - V
    assert S == max(1, math.ceil((L - V) / stride))
    assert (S, stride, V) == R.plan(L, T, overlap)
    assert (S - 1) * stride + T >= L                              # every sample of [0, L) lies in a segment
    covered = np.zeros(L, dtype=bool)
    for s in range(S):
        covered[s * stride: s * stride + T] = True
    assert covered.all()
    assert S == 1 or (S - 2) * stride + T < L                     # and no segment is spare


@pytest.mark.parametrize("L", [1, T - 1, T, T + 1, 3 * T, 3 * T + 5])
def test_no_overlap_is_the_datasets_count(L):
    from pix2pixhdaudiosr_amd.data.audio_dataset import AudioTestDataset
    from pix2pixhdaudiosr_amd.generate import segment_plan
    ds = AudioTestDataset.__new__(AudioTestDataset)
    ds.segment_length = T
    x = torch.arange(L, dtype=torch.float32)
    seg = ds.seg_pad_audio(x[None])
    S, stride, V = segment_plan(L, T, 0)
    assert (S, stride, V) == (seg.shape[0], T, 0)
    np.testing.assert_array_equal(R.gather(x.numpy(), T, stride, S), seg.numpy())


def test_plan_rejects_bad_arguments():
    from pix2pixhdaudiosr_amd.generate import segment_plan
    for bad in (-0.1, 0.51):
        with pytest.raises(ValueError):
            segment_plan(100, T, bad)
    with pytest.raises(ValueError):
        segment_plan(100, 0, 0.25)


@pytest.mark.parametrize("V", [0, 1, 7, T // 2])
def test_weights_sum_to_one(V):
    """A property of the restatement alone (tests/_generate_ref.py): the kernel's weights are tied to it on the GPU, by
    tests/test_gpu_generate.py::test_gather_and_stitch_match_restatement.  The span comes from the product's segment_plan."""
    from pix2pixhdaudiosr_amd.generate import segment_plan
    assert segment_plan(5 * (T - V) + V, T, V / T)[:2] == (5, T - V)
    for S in (1, 2, 5):
        total = R.weight_sum(S, T, T - V)
        assert np.abs(total - 1.0).max() <= np.spacing(1.0)      # 1 ulp
    f = R.fade_in(V)
    assert np.all(f > 0) and np.all(f < 1) and np.all(np.diff(f) > 0)
    np.testing.assert_allclose(f + f[::-1], 1.0, rtol=0, atol=4 * np.spacing(1.0))      # the fade is symmetric


def test_restated_stitch_inverts_gather():
    """The restatement is self-consistent on the product's segment arithmetic (the kernels meet it on the GPU)."""
    from pix2pixhdaudiosr_amd.generate import segment_plan
    x = np.random.default_rng(5).standard_normal(3 * T + 5)
    for overlap in (0, 0.1, 0.25, 0.5):
        S, stride, V = segment_plan(len(x), T, overlap)
        y = R.stitch(R.gather(x, T, stride, S), stride, 1.0, len(x))
        np.testing.assert_allclose(y, x, rtol=0, atol=4 * np.spacing(np.abs(x).max()))


# ------------------------------------------------------------------------------------------
# options dump
# ------------------------------------------------------------------------------------------
OPT_FILES = sorted(glob.glob(os.path.join(GOLDEN, "opt_*.txt")))
EXPECTED = dict(ngf=48, n_blocks_global=3, n_blocks_local=2, netG="local", n_fft=512, hop_length=256, segment_length=32512,
                explicit_encoding=True, mask_mode="mode2", lr_sampling_rate=8000)


def test_four_reference_dumps_are_present():
    assert len(OPT_FILES) == 4


@pytest.mark.parametrize("path", OPT_FILES, ids=[os.path.basename(p) for p in OPT_FILES])
def test_parse_reference_dump(path):
    from pix2pixhdaudiosr_amd.generate import opt_from_file, parse_opt_file
    d = parse_opt_file(path)
    for k, v in EXPECTED.items():
        assert d[k] == v and type(d[k]) is type(v), (k, d[k])
    assert d["use_time_D"] is False                               # (the generation runs: an inference model has no discriminator)
    assert d["max_dataset_size"] == float("inf") and isinstance(d["max_dataset_size"], float)
    assert d["alpha"] == 0.6 and d["min_value"] == 1e-7 and d["phase_encoding_mode"] is None
    assert isinstance(d["checkpoints_dir"], str) and isinstance(d["name"], str)
    assert isinstance(d["gpu_ids"], list) and d["isTrain"] is True            # what the run wrote (one of them on GPU 3) ...
    o = opt_from_file(path, batchSize=2)
    # ... and what generation overrides; explicit overrides win over the file (batchSize: 4 there)
    assert o.isTrain is False and o.gpu_ids == [0] and o.batchSize == 2 and o.ngf == 48 and d["batchSize"] == 4


def test_parse_errors(tmp_path):
    from pix2pixhdaudiosr_amd.generate import parse_opt_file
    with pytest.raises(FileNotFoundError, match="opt.txt"):
        parse_opt_file(str(tmp_path / "opt.txt"))
    bad = tmp_path / "bad.txt"
    bad.write_text("------------ Options -------------\nngf: 48\nthis line has no separator\n-------------- End ----------------\n")
    with pytest.raises(ValueError, match=r"bad\.txt:3"):
        parse_opt_file(str(bad))
    empty = tmp_path / "empty.txt"
    empty.write_text("------------ Options -------------\n-------------- End ----------------\n")
    with pytest.raises(ValueError, match="no `key: value`"):
        parse_opt_file(str(empty))


def test_cli_parser_flags():
    from pix2pixhdaudiosr_amd.generate import _parser
    a = _parser().parse_args(["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck", "--overlap", "0.1",
                              "--batchSize", "2", "--which_epoch", "20", "--is_lr_input", "--no_graph", "--fp16"])
    assert (a.overlap, a.batchSize, a.which_epoch, a.is_lr_input, a.no_graph, a.fp16, a.opt_file) == (0.1, 2, "20", True, True, True, None)
    assert a.reference_amplitude is None and a.mdct_type is None
    b = _parser().parse_args(["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck", "--reference_amplitude", "0"])
    assert b.reference_amplitude == 0 and b.overlap == 0.25
    assert "6 dB" in _parser().format_help()


# ------------------------------------------------------------------------------------------
# util.util names of the reference's Visualizer
# ------------------------------------------------------------------------------------------
def test_visualizer_names_resolve():
    from pix2pixhdaudiosr_amd.util import util as U
    with open(os.path.join(GOLDEN, "visualizer_util_names.json")) as f:
        names = json.load(f)
    assert "save_image" in names
    for n in names:
        assert callable(getattr(U, n)), n


def test_tensor2im_formula():
    from pix2pixhdaudiosr_amd.util.util import tensor2im
    t = torch.randn(3, 5, 7, generator=torch.Generator().manual_seed(3))
    want = np.clip((np.transpose(t.numpy(), (1, 2, 0)) + 1) / 2.0 * 255.0, 0, 255).astype(np.uint8)
    got = tensor2im(t)
    assert got.dtype == np.uint8 and got.shape == (5, 7, 3)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(tensor2im(t, normalize=False), np.clip(np.transpose(t.numpy(), (1, 2, 0)) * 255.0, 0, 255).astype(np.uint8))
    assert tensor2im(t[:1]).shape == (5, 7)                       # one channel: 2-D
    assert [a.shape for a in tensor2im([t, t[:1]])] == [(5, 7, 3), (5, 7)]


@pytest.mark.parametrize("ext", ["jpg", "png"])
def test_save_image_both_kinds(tmp_path, ext):
    from PIL import Image
    from pix2pixhdaudiosr_amd.util.util import save_image
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, size=(12, 20, 3), dtype=np.uint8)                # what the reference's Visualizer passes
    flt = rng.standard_normal((32, 16)).astype(np.float32)                      # what get_current_visuals returns here
    for name, a in (("rgb", rgb), ("flt", flt), ("const", np.zeros((4, 6), dtype=np.float64))):
        path = str(tmp_path / f"{name}.{ext}")
        save_image(a, path)
        back = np.asarray(Image.open(path))
        assert back.shape == a.shape and back.dtype == np.uint8
    if ext == "png":                                                            # lossless: the values themselves
        np.testing.assert_array_equal(np.asarray(Image.open(str(tmp_path / "rgb.png"))), rgb)
        back = np.asarray(Image.open(str(tmp_path / "flt.png")))
        want = np.round((flt.astype(np.float64) - flt.min()) * (255.0 / (float(flt.max()) - float(flt.min()))))
        np.testing.assert_array_equal(back, want.astype(np.uint8))
        assert back.min() == 0 and back.max() == 255


# ------------------------------------------------------------------------------------------
# the package: what pix2pixhdaudiosr_amd.generate exports, and python -m
# ------------------------------------------------------------------------------------------
PUBLIC = ["CROSSOVERS", "LOWBANDS", "METRICS_COLUMNS", "METRICS_COLUMNS_EXT", "METRICS_COLUMNS_PEAKS", "PCM_ENCODINGS", "PCM_FORMATS",
          "CLIP_MODES", "DITHERS", "CROSSOVER_BETA", "CROSSOVER_ATTEN_DB", "CROSSOVER_MAX_TAPS", "SuperResolver", "_parser", "_run",
          "ceiling_from_dbfs", "check_crossover", "check_dither", "check_lowband", "check_output_options", "check_paths", "crossover",
          "crossover_coefficients", "crossover_plan", "crossover_width_hz", "encoding_limit", "main", "metrics_rows", "opt_from_file",
          "parse_opt_file", "pcm_decode", "pcm_encode", "pcm_peaks", "plan_folder", "segment_plan", "segments_gather",
          "segments_gather_planar", "segments_stitch", "segments_stitch_planar", "select_channels", "write_metrics_csv"]


def test_public_names_resolve_to_the_submodules():
    import importlib
    import inspect
    G = importlib.import_module("pix2pixhdaudiosr_amd.generate")
    parts = {"pix2pixhdaudiosr_amd.generate." + m for m in ("ops", "plans", "resolver", "report", "cli")}
    for name in PUBLIC:
        obj = getattr(G, name)
        if inspect.isfunction(obj) or inspect.isclass(obj):
            assert obj.__module__ in parts, (name, obj.__module__)
            assert getattr(importlib.import_module(obj.__module__), name) is obj
    assert G.__doc__.startswith(G._parser().description)


def test_python_m_prints_the_parser_help():
    import subprocess
    import sys
    from pix2pixhdaudiosr_amd.generate import _parser
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.generate", "--help"], cwd=root, capture_output=True, text=True,
                       env=dict(os.environ, COLUMNS="200"))
    assert p.returncode == 0, p.stderr
    options = lambda text: [w for w in text.split() if w.startswith("--")]
    assert options(p.stdout) == options(_parser().format_help()) and "--crossover_taps" in options(p.stdout)
