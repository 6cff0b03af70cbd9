"""--metrics_ext / extended_metrics of whole-file generation (pix2pixhdaudiosr_amd/generate.py): the per-row metrics of every
written channel from one device call, in the result, the printout and four more columns of --metrics_csv; nothing changes
without the flag."""
import csv
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

OLD_HEADER = ["file", "channel", "frames", "mse", "snr_sr", "snr_lr", "lsd"]
NEW_COLUMNS = ["lsd_lf", "lsd_hf", "ssnr_sr", "ssnr_lr"]


def _make_opt(**kw):
    o = dict(gpu_ids=[0], isTrain=True, checkpoints_dir="/tmp/p2phd_test_ckpt", name="t", model="pix2pixHD",
             input_nc=2, output_nc=2, label_nc=0, hr_sampling_rate=48000, lr_sampling_rate=8000,
             n_fft=64, hop_length=32, win_length=64, center=True, no_instance=True, ngf=8, netG="global",
             n_downsample_global=2, n_blocks_global=2, n_local_enhancers=1, n_blocks_local=1, norm="instance",
             no_lsgan=False, ndf=8, n_layers_D=3, num_D=2, no_ganFeat_loss=False, use_hifigan_D=False, use_time_D=False,
             verbose=False, continue_train=False, load_pretrain="", which_epoch="latest", pool_size=0, lr=0.0002,
             beta1=0.5, no_vgg_loss=True, use_match_loss=False, niter_fix_global=0, explicit_encoding=True, alpha=0.6,
             min_value=1e-7, mask=True, mask_mode="mode2", phase_encoding_mode=None, lambda_feat=10.0, fp16=False, niter_decay=100,
             instance_feat=False, label_feat=False)
    o.update(kw)
    return SimpleNamespace(**o)


def _checkpoint(tmp_path):
    """A tiny seeded generator saved as a run folder with its opt.txt, and the model / options loaded back from it."""
    from pix2pixhdaudiosr_amd.generate import opt_from_file
    from pix2pixhdaudiosr_amd.models.models import create_model
    common = dict(mdct_type="mdct4", segment_length=127 * 32, batchSize=2, checkpoints_dir=str(tmp_path), name="run", seed=1234)
    torch.manual_seed(1234)
    create_model(_make_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_make_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    opt = opt_from_file(str(folder / "opt.txt"))
    model = create_model(opt)
    model.eval()
    return folder, model, opt


def _clip(n, start=0):
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    return torch.from_numpy(F["test_wav_excerpt_i16"][start:start + n].astype(np.float32) / 32768.0)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.generate"] + [str(a) for a in args], cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)


def test_folder_cli_extended_metrics(tmp_path):
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.data import wavio
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    from pix2pixhdaudiosr_amd.util import util as U
    folder, model, opt = _checkpoint(tmp_path)
    src = tmp_path / "in"
    src.mkdir()
    n = 2 * opt.segment_length - 300                              # two segments; 6 segmental-SNR hops and more at 48 kHz
    wavio.save(str(src / "a_mono.wav"), _clip(n, 0), 48000)
    wavio.save(str(src / "b_stereo.wav"), torch.stack([_clip(n + 50, 2000), -0.5 * _clip(n + 50, 7000)]), 48000)
    files = ["a_mono.wav", "b_stereo.wav"]

    # the API: one call of the per-row entry per file, whatever its channels; the figures are those of the returned tensors
    sr = SuperResolver(model, opt)
    lib = _lib.lib()
    want, per_call = [], None
    for rel, C in zip(files, (1, 2)):
        torch.manual_seed(opt.seed)
        lib.p2phd_launch_count(b"metrics_rows", 1)
        res = sr.enhance_file(str(src / rel), None, channels='all', extended_metrics=True)
        launches = lib.p2phd_launch_count(b"metrics_rows", 1)
        assert launches > 0 and per_call in (None, launches)
        per_call = launches
        ext = res['metrics_ext']
        assert isinstance(ext, list) and len(ext) == C and all(tuple(e) == U.METRIC_ROW_NAMES for e in ext)
        assert ext == U.compute_matrics_ext(res['hr'], res['lr'], res['sr'], opt)
        assert [tuple(m) for m in res['metrics']] == [(e['mse'], e['snr_sr'], e['snr_lr'], 0, 0, 0, e['lsd']) for e in ext]
        assert all(np.isfinite(list(e.values())).all() for e in ext)
        assert all(-10.0 <= e[k] <= 35.0 for e in ext for k in ('ssnr_sr', 'ssnr_lr'))
        # the existing figures, measured the existing way on the same tensors
        for c, e in enumerate(ext):
            old = U.compute_matrics(res['hr'][c:c + 1], res['lr'][c:c + 1], res['sr'][c:c + 1], opt)
            np.testing.assert_allclose([e['mse'], e['snr_sr'], e['snr_lr'], e['lsd']], [old[0], old[1], old[2], old[6]], rtol=1e-4)
        want += [(rel, c, e) for c, e in enumerate(ext)]
    # 'first' keeps the 7-tuple and carries a one-entry list; without the option there is no such key
    torch.manual_seed(opt.seed)
    first = sr.enhance_file(str(src / "b_stereo.wav"), None, extended_metrics=True)
    assert isinstance(first['metrics'], tuple) and len(first['metrics']) == 7 and len(first['metrics_ext']) == 1
    assert first['metrics'] == tuple(first['metrics_ext'][0][k] if k else 0 for k in ('mse', 'snr_sr', 'snr_lr', 0, 0, 0, 'lsd'))
    assert 'metrics_ext' not in sr.enhance_file(str(src / "a_mono.wav"), None)

    # the command line with the flag
    csv_path = str(tmp_path / "ext.csv")
    p = _cli("--input", src, "--output", tmp_path / "out", "--load_pretrain", folder, "--channels", "all", "--metrics_csv", csv_path,
             "--metrics_ext")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "LSD_LF" in p.stdout and "LSD_HF" in p.stdout and "SSNR_SR" in p.stdout and "SSNR_LR" in p.stdout
    with open(csv_path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == OLD_HEADER + NEW_COLUMNS
    assert [(r[0], r[1]) for r in rows[1:]] == [("a_mono.wav", "0"), ("b_stereo.wav", "0"), ("b_stereo.wav", "1"), ("mean", "")]
    body = [[float(v) for v in r[3:]] for r in rows[1:]]
    names = rows[0][3:]
    for got, (rel, c, e) in zip(body[:-1], want):
        assert got == [e[k] for k in names], (rel, c)
    for k in range(len(names)):
        assert body[-1][k] == sum(r[k] for r in body[:-1]) / 3, names[k]

    # ... and without it: today's table and printout
    old_path = str(tmp_path / "old.csv")
    p = _cli("--input", src, "--output", tmp_path / "out_old", "--load_pretrain", folder, "--channels", "all", "--metrics_csv", old_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "LSD_HF" not in p.stdout and "SSNR" not in p.stdout
    with open(old_path, newline="") as f:
        old_rows = list(csv.reader(f))
    assert old_rows[0] == OLD_HEADER and all(len(r) == 7 for r in old_rows) and len(old_rows) == 5
    for a, b in zip(old_rows[1:-1], body[:-1]):
        np.testing.assert_allclose([float(v) for v in a[3:]], b[:4], rtol=1e-4)
    for rel in files:
        assert open(str(tmp_path / "out" / rel), "rb").read() == open(str(tmp_path / "out_old" / rel), "rb").read()
