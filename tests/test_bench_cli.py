"""bench.py command-line contract: the rank launcher and its argument checks, --dump-outputs (no GPU needed), and one
plain run on the GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env(**kw):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(kw)
    return env


def test_bench_refuses_mismatched_world():
    """Under a launcher (WORLD_SIZE set) --gpus must agree with it: a silent n_gpus != N line is what round 1 printed."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "1"], cwd=ROOT, capture_output=True, text=True,
                       env=_clean_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stdout + r.stderr)


def test_bench_gpus_n_starts_n_ranks_and_propagates_failure():
    """`bench.py --gpus 2` without a launcher starts torch.distributed.run with two ranks as CHILD processes (the parent
    never touches the GPU); without a GPU both ranks fail at set_device and the parent must exit non-zero, not print a
    1-GPU line."""
    import torch
    if torch.cuda.is_available():
        return                                                      # covered by tests/test_gpu_dp.py on the GPU box
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"], cwd=ROOT,
                       capture_output=True, text=True, env=_clean_env(), timeout=600)
    assert r.returncode != 0
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())
    err = r.stdout + r.stderr
    assert "local_rank: 1" in err or "rank: 1" in err or "rank      : 1" in err, err[-3000:]


def test_bench_refuses_zero_steps():
    """--steps sets the number of timed steps and ms_per_step divides by it: 0 is refused before anything runs."""
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], cwd=ROOT, capture_output=True, text=True, env=_clean_env(),
                       timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_outputs_writes_float32_within_64_mb_and_samples_the_same_elements(tmp_path):
    """--dump-outputs on stand-in tensors (CPU): one float32 .npy per output, small arrays whole, arrays beyond DUMP_SAMPLE
    elements as a seeded sample that picks the same elements on every call."""
    from types import SimpleNamespace
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    sr = torch.randn(4, 2, 64, 32, generator=g)
    wG = torch.randn(3 * bench.DUMP_SAMPLE, generator=g)
    model = SimpleNamespace(_visual=(None, sr, None, None), optimizer_G=SimpleNamespace(flat_p=wG),
                            optimizer_D=SimpleNamespace(flat_p=torch.arange(1000, dtype=torch.float32)))
    losses = {"G_GAN": torch.tensor(1.5), "D_real": torch.tensor(0.25), "G_GAN_Feat": 0}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, losses)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["loss_D_real.npy", "loss_G_GAN.npy", "netD_weights.npy", "netG_weights.npy", "sr_spectro.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    got = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype == np.float32 for v in got.values())
    assert float(got["loss_G_GAN.npy"]) == 1.5
    assert np.array_equal(got["sr_spectro.npy"], sr.numpy()) and np.array_equal(got["netD_weights.npy"], np.arange(1000))
    s = got["netG_weights.npy"]
    assert bench.DUMP_SAMPLE // 2 < s.size <= bench.DUMP_SAMPLE and np.isin(s, wG.numpy()).all()
    assert all(np.array_equal(v, np.load(tmp_path / "b" / f)) for f, v in got.items())


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain run: --steps timed steps, the contract fields, none of --full's extra measurements.  --dump-outputs writes the
    last timed step's outputs (finite float32, at most 64 MB); that step starts from the initial state, so a second run
    repeats its losses and spectrogram bit for bit and its weights up to the atomically summed noise biases."""
    import json
    import numpy as np
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--steps", "3", "--warmup", "1", "--batch", "2", "--dump-outputs", str(tmp_path / d)],
                           cwd=ROOT, capture_output=True, text=True, env=_clean_env(), timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "frames/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert not {"roofline", "mdct", "cpu_baseline"} & set(out) and "G_fwd_bwd_ms" not in out["config"]
    files = sorted(os.listdir(tmp_path / "a"))
    assert {"loss_G_GAN.npy", "loss_D_real.npy", "loss_D_fake.npy", "sr_spectro.npy", "netG_weights.npy"} <= set(files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    assert np.load(tmp_path / "a" / "sr_spectro.npy").shape == (2, 2, 512, 256)
    for f in files:
        va, vb = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert va.dtype == np.float32 and np.isfinite(va).all(), f
        if f.endswith("_weights.npy"):
            assert np.linalg.norm(va - vb) <= 1e-4 * np.linalg.norm(vb), f
        else:
            assert np.array_equal(va, vb), f
