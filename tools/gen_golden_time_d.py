#!/usr/bin/env python3
"""Generate tests/golden/time_d_step{,_grads,_after}.npz: one training step of the REFERENCE model on CPU with --use_time_D.

The reference's own MDCT2 / IMDCT2 (what the shipped model hard-codes), the tiny geometry of gen_golden.gen_model
(n_fft 64, hop 32, ngf 8, ndf 8, num_D 2, B 2, 16 frames), recorded mask noise.  Written: inputs, the windowed frames of
both clips, `sr`, `sr_frames`, the three inputs of time_D (in call order: dB fake, dB real, raw fake), loss names and
values, initial G_ / D_ / T_ weights, the gradients of all three networks for loss_G then loss_D (train.py:155-184), the
weights after one Adam step, and `loss_values_f64`: the losses of a float64 copy of the same model on the same inputs
(the reference's own fp32 rounding error, which the parity test's loss bounds are derived from).

Needs the reference checkout (gen_golden.REF); third-party imports are stubbed as in gen_golden.py.

Usage:  python tools/gen_golden_time_d.py [--out tests/golden]
"""
import argparse
import contextlib
import io
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402
from gen_golden import _np, _stub_modules  # noqa: E402


def _opt():
    return SimpleNamespace(
        gpu_ids=[], isTrain=True, checkpoints_dir="/tmp/p2phd_golden", name="g", resize_or_crop="none",
        instance_feat=False, label_feat=False, load_features=False, label_nc=0, input_nc=2, output_nc=2,
        hr_sampling_rate=48000, lr_sampling_rate=8000, n_fft=64, hop_length=32, win_length=64, center=True,
        no_instance=True, feat_num=3, ngf=8, netG="global", n_downsample_global=2, n_blocks_global=2,
        n_local_enhancers=1, n_blocks_local=1, norm="instance", no_lsgan=False, ndf=8, n_layers_D=3, num_D=2,
        no_ganFeat_loss=False, use_hifigan_D=False, use_time_D=True, verbose=False, continue_train=False,
        load_pretrain="", which_epoch="latest", pool_size=0, lr=0.0002, beta1=0.5, no_vgg_loss=True,
        use_match_loss=False, niter_fix_global=0, explicit_encoding=True, alpha=0.6, min_value=1e-7, mask=True,
        mask_mode="mode2", phase_encoding_mode=None, lambda_feat=10.0, lambda_mat=10.0, lambda_time=0.4,
        abs_spectro=True, fp16=False, nef=16, n_downsample_E=4)


def _build(opt):
    from models.pix2pixHD_model import Pix2PixHDModel
    with contextlib.redirect_stdout(io.StringIO()):
        model = Pix2PixHDModel()
        model.initialize(opt)
    return model


def _forward(model, lr, hr, noise):
    """model.forward with the recorded mask noise handed to the torch.randn of pix2pixHD_model.py:202."""
    _randn = torch.randn
    torch.randn = lambda *a, **k: noise.clone()
    try:
        return model.forward(lr, None, hr, None, infer=True)
    finally:
        torch.randn = _randn


def gen_time_d(out):
    from models.mdct import MDCT2, IMDCT2
    from dct.dct_native import DCT_2N_native, IDCT_2N_native
    d = {}
    opt = _opt()
    torch.manual_seed(1234)
    model = _build(opt)
    frames, B = 16, 2
    T = (frames - 1) * opt.hop_length
    g = torch.Generator().manual_seed(77)
    hr = 0.1 * torch.randn(B, T, generator=g)
    lr = 0.1 * torch.randn(B, T, generator=g)
    # exact zeros inside a frame, besides those of the centre padding: dB must clamp them to min_value
    hr[0, 100:140] = 0.0
    lr[1, 200:230] = 0.0
    d["hr"] = _np(hr); d["lr"] = _np(lr)
    d["window"] = _np(model.window)
    mask_size = int(opt.n_fft * (1 - 1 / (opt.hr_sampling_rate / opt.lr_sampling_rate)))
    noise = torch.randn(B, 2, mask_size, frames, generator=torch.Generator().manual_seed(4321))
    d["mask_noise"] = _np(noise)

    for k, v in model.netG.state_dict().items():
        d[f"G_p_{k}"] = _np(v)
    for k, v in model.netD.state_dict().items():
        d[f"D_p_{k}"] = _np(v)
    for k, v in model.time_D.state_dict().items():
        d[f"T_p_{k}"] = _np(v)
    d["T_keys"] = np.array(list(model.time_D.state_dict().keys()))

    seen = []
    time_fwd = model.time_D.forward                   # the reference calls .forward directly: hooks would not see it

    def recording_forward(x):
        seen.append(_np(x))
        return time_fwd(x)
    model.time_D.forward = recording_forward
    losses, sr = _forward(model, lr, hr, noise)
    del model.time_D.forward
    assert len(seen) == 3
    d["time_in_fake_db"], d["time_in_real_db"], d["time_in_g_raw"] = seen
    names = model.loss_names
    d["loss_names"] = np.array(names)
    d["loss_values"] = np.array([float(l) for l in losses], dtype=np.float64)
    d["sr"] = _np(sr)
    d["lambda_time"] = np.array(opt.lambda_time)

    with torch.no_grad():
        _, _, hnorm = model.to_spectro(hr, mask=False)
        torch_randn = torch.randn
        torch.randn = lambda *a, **k: noise.clone()
        try:
            _, _, lnorm = model.to_spectro(lr, mask=True)
        finally:
            torch.randn = torch_randn
        d["hr_frames"] = _np(hnorm["frames"]); d["lr_frames"] = _np(lnorm["frames"])
        d["lr_max"] = _np(lnorm["max"]); d["lr_min"] = _np(lnorm["min"])
        d["sr_frames"] = _np(np.sqrt(model.up_ratio - 1) * model.window * model.to_frames(sr, lnorm))

    ld = dict(zip(names, losses))
    loss_D = (ld["D_fake"] + ld["D_real"]) * 0.5 + (ld["D_fake_t"] + ld["D_real_t"]) * 0.5
    loss_G = ld["G_GAN"] + ld.get("G_GAN_Feat", 0) + ld["G_GAN_t"]
    model.optimizer_G.zero_grad(); loss_G.backward(retain_graph=True)
    for k, v in model.netG.named_parameters():
        d[f"G_g_{k}"] = _np(v.grad)
    model.optimizer_G.step()
    model.optimizer_D.zero_grad(); loss_D.backward()
    for k, v in model.netD.named_parameters():
        d[f"D_g_{k}"] = _np(v.grad)
    for k, v in model.time_D.named_parameters():
        d[f"T_g_{k}"] = _np(v.grad)
    model.optimizer_D.step()
    for k, v in model.netG.state_dict().items():
        d[f"G_p1_{k}"] = _np(v)
    for k, v in model.netD.state_dict().items():
        d[f"D_p1_{k}"] = _np(v)
    for k, v in model.time_D.state_dict().items():
        d[f"T_p1_{k}"] = _np(v)

    # the same step in float64: same weights, same inputs
    m64 = _build(opt)
    for name in ("netG", "netD", "time_D"):
        net = getattr(m64, name)
        net.load_state_dict({k[len(p) + 3:]: torch.from_numpy(v) for p in (dict(netG="G", netD="D", time_D="T")[name],)
                             for k, v in d.items() if k.startswith(p + "_p_")})
        net.double()
    m64.window = model.window.double()
    kw = dict(n_fft=opt.n_fft, hop_length=opt.hop_length, win_length=opt.win_length, window=m64.window, device="cpu")
    m64._dct, m64._idct = DCT_2N_native(), IDCT_2N_native()
    m64._mdct = MDCT2(dct_op=m64._dct, **kw)
    m64._imdct = IMDCT2(idct_op=m64._idct, **kw)
    with torch.no_grad():
        l64, _ = _forward(m64, lr.double(), hr.double(), noise.double())
    assert all(l.dtype == torch.float64 for l in l64)
    d["loss_values_f64"] = np.array([float(l) for l in l64], dtype=np.float64)

    d["torch_version"] = np.array(torch.__version__)
    # three files, each below the repository's size limit for one committed file: the step itself with the initial weights,
    # the gradients, the weights after the step
    grads = {k: d.pop(k) for k in list(d) if k[:4] in ("G_g_", "D_g_", "T_g_")}
    after = {k: d.pop(k) for k in list(d) if k[:5] in ("G_p1_", "D_p1_", "T_p1_")}
    np.savez_compressed(os.path.join(out, "time_d_step.npz"), **d)
    np.savez_compressed(os.path.join(out, "time_d_step_grads.npz"), **grads)
    np.savez_compressed(os.path.join(out, "time_d_step_after.npz"), **after)
    print("time_d_step.npz", len(d), "arrays; losses", dict(zip(names, d["loss_values"])))
    print("fp32 - fp64:", dict(zip(names, d["loss_values"] - d["loss_values_f64"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    _stub_modules()
    sys.path.insert(0, gg.REF)
    torch.set_num_threads(4)
    gen_time_d(a.out)


if __name__ == "__main__":
    main()
