"""Step time of --use_time_D at the published run's geometry (n_fft 512, hop 256, win 512, segment 32512, netG local,
ngf 48, num_D 2), bf16, graphed step, flag off and on, and the new kernels alone with their HBM traffic.

    python tools/time_time_d.py [batch] [replays]        (GPU)

Also the two discriminators alone (forward + both backward passes as the step runs them), whose ratio is the yardstick of
DESIGN 6; P2PHD_TIME_D_TRACE=1 adds a per-kernel table of the time-domain passes.  Per configuration: warm-up (two eager steps, capture, 3 replays), then two runs of `replays` graph replays each between
device synchronisations; prints ms/step of both runs.  Kernels alone: 50 launches between two events after 5 warm-up launches.
"""
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_opt(use_time_D):
    return SimpleNamespace(
        gpu_ids=[0], isTrain=True, checkpoints_dir="/tmp/p2phd_time_d", name="t", model="pix2pixHD", input_nc=2, output_nc=2,
        label_nc=0, hr_sampling_rate=48000, lr_sampling_rate=8000, n_fft=512, hop_length=256, win_length=512, center=True,
        no_instance=True, ngf=48, netG="local", n_downsample_global=4, n_blocks_global=9, n_local_enhancers=1, n_blocks_local=3,
        norm="instance", no_lsgan=False, ndf=64, n_layers_D=3, num_D=2, no_ganFeat_loss=False, use_hifigan_D=False,
        use_time_D=use_time_D, mdct_type="mdct2", verbose=False, continue_train=False, load_pretrain="", which_epoch="latest",
        pool_size=0, lr=0.0002, beta1=0.5, no_vgg_loss=True, use_match_loss=False, niter_fix_global=0, explicit_encoding=True,
        alpha=0.6, min_value=1e-7, mask=True, mask_mode="mode2", phase_encoding_mode=None, lambda_feat=10.0, lambda_time=0.4,
        fp16=True, niter_decay=100, instance_feat=False, label_feat=False)


def time_step(use_time_D, B, replays):
    from pix2pixhdaudiosr_amd.models.models import create_model
    torch.manual_seed(1234)
    m = create_model(make_opt(use_time_D))
    hr = 0.1 * torch.randn(B, 32512, device="cuda")
    lr = 0.1 * torch.randn(B, 32512, device="cuda")
    for _ in range(6):
        m.train_step_graphed(lr, hr)
    runs = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(replays):
            m.train_step_graphed(lr, hr)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / replays * 1e3)
    print(f"use_time_D={use_time_D} B={B}: {runs[0]:.3f} / {runs[1]:.3f} ms per graphed bf16 step ({replays} replays per run)")
    return min(runs)


def time_kernel(name, fn, nbytes):
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(50):
        fn()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / 50 * 1e3
    print(f"{name}: {us:.1f} us, {nbytes / us / 1e6:.2f} TB/s of {nbytes / 1e6:.1f} MB")


def kernels(B):
    from pix2pixhdaudiosr_amd import _ops
    from pix2pixhdaudiosr_amd.models.mdct import MDCT2, _DctTables
    from pix2pixhdaudiosr_amd.util.util import kbdwin
    N, F = 512, 128
    w = kbdwin(N).cuda()
    x = 0.1 * torch.randn(B, 32512, device="cuda")
    m = MDCT2(n_fft=N, hop_length=256, win_length=N, window=w, device="cuda")
    time_kernel("mdct2 (spectrogram only)", lambda: m(x), B * (32512 + F * N) * 4)
    time_kernel("mdct2 + frames", lambda: m(x, return_ola=True), B * (32512 + 2 * F * N) * 4)
    fr = torch.randn(B, F, N, device="cuda")
    for dt, eb in ((torch.bfloat16, 2), (torch.float32, 4)):
        for db in (True, False):
            time_kernel(f"pack {'dB' if db else 'raw'} {dt}", lambda: _ops.pack_frame_pair(dt, fr, fr, db, 1e-7), B * F * N * (8 + 8 * eb))
    sr = (torch.rand(B, 2, N, F, device="cuda") * 2 - 1).requires_grad_(True)
    mm = torch.tensor([-150.0, -20.0], device="cuda")
    tb = _DctTables.get(N, sr.device)
    args = (sr, mm, w, tb, 0.6, 1e-7, float(np.sqrt(5.0)))
    time_kernel("spectrogram -> frames", lambda: _ops.SpectroToFrames.apply(*args), B * F * N * 12)
    y = _ops.SpectroToFrames.apply(*args)
    g = torch.randn_like(y)
    time_kernel("frames adjoint", lambda: torch.autograd.grad(y, sr, g, retain_graph=True), B * F * N * 20)


def time_d_parts(B, reps=10):
    """Forward + both backward passes of the spectral discriminator alone and of the time-domain branch alone, as the training
    step runs them (pair pass / three passes, generator-loss backward down to the generated spectrogram without D weight
    gradients, then the discriminator-loss backward), eager, between two events."""
    from pix2pixhdaudiosr_amd import _ops
    from pix2pixhdaudiosr_amd.models.models import create_model
    torch.manual_seed(1234)
    m = create_model(make_opt(True))
    dev = m.device
    hr = 0.1 * torch.randn(B, 32512, device="cuda")
    lr = 0.1 * torch.randn(B, 32512, device="cuda")
    for _ in range(2):
        m.train_step(lr, hr)
    with torch.no_grad():
        lr_s, _, hr_s, _, _, _, hn, ln = m.encode_input(lr, None, hr, None)
    sr0 = torch.rand(B, 2, 512, 128, device="cuda") * 2 - 1
    optD = m.optimizer_D
    firsts = [net._scale_steps(d)[0][0].spec for net in (m.netD, m.time_D) for d in range(m.opt.num_D)]

    def run(which):
        _ops.begin_step(dev)
        sr = sr0.clone().requires_grad_(True)
        if which == "spectral":
            g_gan, g_feat, d_real, d_fake = m._spectral_losses(lr_s, hr_s, sr, True)
            loss_G, net = g_gan + g_feat, m.netD
        else:
            loss_G, d_real, d_fake = m._time_losses(sr, ln, hn)
            net = m.time_D
        _ops.end_arena(dev)
        optD.zero_grad(lazy=True)
        with _ops.backward_without_weight_grads(optD._params), m._fake_half():
            loss_G.backward(inputs=[sr], retain_graph=True)
        with _ops.backward_without_input_grads(firsts):
            ((d_fake + d_real) * 0.5).backward(inputs=list(net.parameters()))

    out = {}
    for which in ("spectral", "time"):
        for _ in range(3):
            run(which)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(reps):
            run(which)
        b.record()
        host = (time.perf_counter() - t0) / reps * 1e3           # host time to ISSUE the work: below the device time = GPU-bound
        torch.cuda.synchronize()
        out[which] = a.elapsed_time(b) / reps
        print(f"{which} discriminator fwd + bwd alone, B={B}: {out[which]:.3f} ms (host issue time {host:.3f} ms)")
    print(f"time-domain branch / spectral discriminator: {out['time'] / out['spectral']:.3f} x")
    if os.environ.get("P2PHD_TIME_D_TRACE", "0") == "1":           # per-kernel device time of one time-domain pass set
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            run("time")
            torch.cuda.synchronize()
        print(prof.key_averages().table(sort_by="cuda_time_total", row_limit=14, max_name_column_width=70))


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    replays = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    torch.cuda.set_device(0)
    kernels(B)
    time_d_parts(B)
    off = time_step(False, B, replays)
    on = time_step(True, B, replays)
    print(f"flag on - off: {on - off:.3f} ms per step ({on / off:.3f} x)")


if __name__ == "__main__":
    main()
