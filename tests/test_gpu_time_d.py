"""GPU tests of the time-domain discriminator (--use_time_D): the frame output of MDCT2, the pair pack, the
spectrogram <-> frames kernels, and the whole step against the reference's own step on CPU
(tests/golden/time_d_step*.npz from tools/gen_golden_time_d.py) and against tests/_time_d_ref.py at sizes a fixture
cannot hold.

Loss bound (tests 4, 5, 8): 1e-4 relative (the project's bound) for every term whose reference fp32-vs-fp64 gap in the
fixture is below 1e-5; for a term above that, 4 x that recorded gap, never below 1e-4.  Computed here from
`loss_values` and `loss_values_f64`: dB of generated frames near zero amplifies fp32 rounding in the reference as much as
in this code, and the fixture records by how much."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _time_d_ref as R
from conftest import GOLDEN, rel_err, assert_grad_close, noise_bias_keys

pytestmark = pytest.mark.gpu

MINV, ALPHA, UP = 1e-7, 0.6, 6.0


@pytest.fixture(scope="module")
def g():
    d = {}
    for f in ("time_d_step.npz", "time_d_step_grads.npz", "time_d_step_after.npz"):
        z = np.load(os.path.join(GOLDEN, f))
        d.update({k: z[k] for k in z.files})
    return d


def make_opt(**kw):
    o = dict(gpu_ids=[0], isTrain=True, checkpoints_dir="/tmp/p2phd_test_ckpt", name="time_d", model="pix2pixHD",
             input_nc=2, output_nc=2, label_nc=0, hr_sampling_rate=48000, lr_sampling_rate=8000,
             n_fft=64, hop_length=32, win_length=64, center=True, no_instance=True, ngf=8, netG="global",
             n_downsample_global=2, n_blocks_global=2, n_local_enhancers=1, n_blocks_local=1, norm="instance",
             no_lsgan=False, ndf=8, n_layers_D=3, num_D=2, no_ganFeat_loss=False, use_hifigan_D=False, use_time_D=True,
             mdct_type="mdct2", verbose=False, continue_train=False, load_pretrain="", which_epoch="latest", pool_size=0,
             lr=0.0002, beta1=0.5, no_vgg_loss=True, use_match_loss=False, niter_fix_global=0, explicit_encoding=True,
             alpha=ALPHA, min_value=MINV, mask=True, mask_mode="mode2", phase_encoding_mode=None, lambda_feat=10.0,
             lambda_time=0.4, fp16=False, niter_decay=100, instance_feat=False, label_feat=False)
    o.update(kw)
    return SimpleNamespace(**o)


NETS = (("netG", "G"), ("netD", "D"), ("time_D", "T"))


def _model(g, **kw):
    from pix2pixhdaudiosr_amd import _ops
    from pix2pixhdaudiosr_amd.models.models import create_model
    model = create_model(make_opt(**kw))
    for name, tag in NETS:
        net = getattr(model, name)
        net.load_state_dict({k: torch.from_numpy(g[f"{tag}_p_{k}"]) for k in net.state_dict().keys()})
    _ops.bump_weight_epoch()
    return model


def _inputs(g):
    return tuple(torch.from_numpy(g[k]) for k in ("lr", "hr", "mask_noise"))


def loss_bounds(g):
    """name -> relative bound, from the fixture's own fp32-vs-fp64 gap (module docstring)."""
    out = {}
    for n, v32, v64 in zip(g["loss_names"], g["loss_values"], g["loss_values_f64"]):
        gap = abs(float(v32) - float(v64)) / max(1.0, abs(float(v64)))
        out[str(n)] = 1e-4 if gap < 1e-5 else max(1e-4, 4.0 * gap)
    return out


def _check_losses(got, ref, bounds, what=""):
    for k, r in ref.items():
        v = float(got[k])
        print(f"{what}{k}: got {v:.9g} ref {float(r):.9g} rel {abs(v - float(r)) / max(1.0, abs(float(r))):.3e} bound {bounds[k]:.1e}")
    for k, r in ref.items():
        assert abs(float(got[k]) - float(r)) <= bounds[k] * max(1.0, abs(float(r))), (what, k, float(got[k]), float(r))


# ------------------------------------------------------------------------------------------ 1
def test_mdct2_return_ola_frames(g):
    from pix2pixhdaudiosr_amd.models.mdct import MDCT2
    w = torch.from_numpy(g["window"])
    m = MDCT2(n_fft=64, hop_length=32, win_length=64, window=w, device="cuda")
    for clip in ("lr", "hr"):
        x = torch.from_numpy(g[clip]).cuda()
        spec, frames = m(x, return_ola=True)
        assert tuple(frames.shape) == g[clip + "_frames"].shape and not frames.requires_grad
        assert rel_err(frames.cpu().numpy(), g[clip + "_frames"]) < 1e-6
        assert torch.equal(spec, m(x))                             # the spectrogram is the one return_ola=False gives
    # n_fft 512 / hop 256 / B 32: the len(signal) quirk at a batch below hop (padding follows the batch size)
    from pix2pixhdaudiosr_amd.util.util import kbdwin
    w = kbdwin(512)
    x = 0.1 * torch.randn(32, 32512, generator=torch.Generator().manual_seed(3))
    m = MDCT2(n_fft=512, hop_length=256, win_length=512, window=w, device="cuda")
    spec, frames = m(x.cuda(), return_ola=True)
    ref = R.mdct2_frames(x, 256, 512, w)
    assert tuple(frames.shape) == tuple(ref.shape)
    assert rel_err(frames.cpu().numpy(), ref.numpy()) < 1e-6
    assert torch.equal(spec, m(x.cuda()))


# ------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("db", [True, False])
def test_pair_pack(g, dtype, db):
    from pix2pixhdaudiosr_amd import _ops
    lr_f, hr_f = torch.from_numpy(g["lr_frames"]), torch.from_numpy(g["hr_frames"])
    assert (lr_f == 0).any() and (hr_f == 0).any()
    out = _ops.pack_frame_pair(dtype, lr_f.cuda(), hr_f.cuda(), db, MINV)
    assert out.dtype == dtype and tuple(out.shape) == (*lr_f.shape, 8)
    out = out.float().cpu()
    assert torch.isfinite(out).all()
    assert (out[..., 2:] == 0).all()                               # pad channels
    ref = torch.stack((lr_f, hr_f), dim=-1)
    if db:
        ref = R.to_db(ref, MINV)
        floor = 20 * np.log10(MINV) - 20
        assert float(out[..., 0][lr_f == 0].max()) == pytest.approx(floor, abs=1e-3 if dtype == torch.float32 else 1.0)
    if dtype == torch.float32:
        # raw: exact.  dB: values reach 160 in magnitude, where one fp32 ulp is 2^-16; log10 (its last-bit error times 20), the
        # multiply and the subtraction each round once in either implementation -> 4 ulp
        assert float((out[..., :2] - ref).abs().max()) <= (4 * 2.0 ** -16 if db else 0.0)
    else:
        assert float(((out[..., :2] - ref).abs() / ref.abs().clamp(min=1e-30)).max()) <= 2.0 ** -8     # bf16 rounding
    # sources one float off a 16-byte boundary (views such as frames.reshape(-1)[1:]): the element-wise path
    n_el = lr_f.numel() - 4
    a1, b1 = lr_f.cuda().reshape(-1)[1:1 + n_el].reshape(1, 1, n_el), hr_f.cuda().reshape(-1)[1:1 + n_el].reshape(1, 1, n_el)
    assert a1.data_ptr() % 16 == 4 and a1.is_contiguous()
    o1 = _ops.pack_frame_pair(dtype, a1, b1, db, MINV).float().cpu().reshape(-1, 8)
    assert torch.equal(o1, out.reshape(-1, 8)[1:1 + n_el])
    # odd size: the tail of the last quad
    a = lr_f.reshape(-1)[:1027].reshape(1, 1, 1027).contiguous().cuda()
    o2 = _ops.pack_frame_pair(dtype, a, a, db, MINV).float().cpu()
    assert torch.equal(o2[0, 0, :, 0], out.reshape(-1, 8)[:1027, 0]) and (o2[..., 2:] == 0).all()


# ------------------------------------------------------------------------------------------ 3
def _frames_fn(sr, mm, window, scale=None, n_fft=64):
    from pix2pixhdaudiosr_amd import _ops
    from pix2pixhdaudiosr_amd.models.mdct import _DctTables
    return _ops.SpectroToFrames.apply(sr, mm, window, _DctTables.get(n_fft, sr.device), ALPHA, MINV,
                                      float(np.sqrt(UP - 1)) if scale is None else scale)


def test_spectro_to_frames_forward_and_adjoint(g):
    dev = "cuda"
    window = torch.from_numpy(g["window"]).to(dev)
    mm = torch.tensor([float(g["lr_min"]), float(g["lr_max"])], device=dev)
    sr = torch.from_numpy(g["sr"]).to(dev).requires_grad_(True)
    out = _frames_fn(sr, mm, window)
    assert tuple(out.shape) == g["sr_frames"].shape
    assert rel_err(out.detach().cpu().numpy(), g["sr_frames"]) < 1e-5
    # adjoint vs autograd through the restatement (float64 on the CPU)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(5))
    (gx,) = torch.autograd.grad(out, sr, cot.to(dev))
    sr64 = torch.from_numpy(g["sr"]).double().requires_grad_(True)
    ref = R.sr_frames(sr64, float(g["lr_min"]), float(g["lr_max"]), ALPHA, MINV, UP, torch.from_numpy(g["window"]).double())
    (gx_ref,) = torch.autograd.grad(ref[:, 0], sr64, cot.double())
    assert rel_err(gx.cpu().numpy(), gx_ref.numpy()) < 1e-5
    # larger transforms and frame counts that do not fill a tile: forward and adjoint against the float64 restatement (same bounds),
    # and the inner-product identity <A dx, dy> = <dx, A^T dy> of the Jacobian A at x, with A dx taken from the restatement
    from pix2pixhdaudiosr_amd.util.util import kbdwin
    for n_fft, F in ((64, 16), (512, 21), (1024, 5)):
        w = kbdwin(n_fft)
        gen = torch.Generator().manual_seed(n_fft)
        x = torch.rand(3, 2, n_fft, F, generator=gen) * 2 - 1
        dy = torch.randn(3, F, n_fft, generator=gen)
        dx = torch.randn(x.shape, generator=gen)
        xg = x.to(dev).requires_grad_(True)
        y = _frames_fn(xg, torch.tensor([-150.0, -20.0], device=dev), w.to(dev), n_fft=n_fft)
        (gx,) = torch.autograd.grad(y, xg, dy.to(dev))
        x64 = x.double().requires_grad_(True)
        y_ref = R.sr_frames(x64, -150.0, -20.0, ALPHA, MINV, UP, w.double())[:, 0]
        (gx_ref,) = torch.autograd.grad(y_ref, x64, dy.double(), retain_graph=True)
        assert rel_err(y.detach().cpu().numpy(), y_ref.detach().numpy()) < 1e-5, (n_fft, F)
        assert rel_err(gx.cpu().numpy(), gx_ref.numpy()) < 1e-5, (n_fft, F)
        jvp = torch.autograd.functional.jvp(lambda t: R.sr_frames(t, -150.0, -20.0, ALPHA, MINV, UP, w.double())[:, 0], x.double(), dx.double())[1]
        lhs, rhs = float((jvp * dy.double()).sum()), float((gx.cpu().double() * dx.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float(jvp.norm() * dy.double().norm()), (n_fft, F, lhs, rhs)


# ------------------------------------------------------------------------------------------ 4
def test_fp32_step_against_the_reference(g):
    m = _model(g)
    names = [str(n) for n in g["loss_names"]]
    assert m.loss_names == names
    lr, hr, noise = _inputs(g)
    _, _, ln = m.to_spectro(lr, mask=True, noise=noise)
    assert rel_err(ln["frames"].cpu().numpy(), g["lr_frames"]) < 1e-6       # norm['frames'] carries the frames
    losses, sr = m.forward(lr, None, hr, None, infer=True, noise=noise)
    got = dict(zip(m.loss_names, losses))
    _check_losses(got, dict(zip(names, g["loss_values"])), loss_bounds(g))
    assert rel_err(sr.detach().cpu().numpy(), g["sr"]) < 1e-4
    loss_D = (got["D_fake"] + got["D_real"]) * 0.5 + (got["D_fake_t"] + got["D_real_t"]) * 0.5
    loss_G = got["G_GAN"] + got["G_GAN_Feat"] + got["G_GAN_t"]
    m.optimizer_G.zero_grad(); loss_G.backward()
    nb = {tag: noise_bias_keys([k for k, _ in getattr(m, name).named_parameters()]) for name, tag in NETS}
    for k, p in m.netG.named_parameters():
        assert_grad_close("G:" + k, p.grad.cpu().numpy(), g[f"G_g_{k}"], rtol=5e-4, noise_biases=nb["G"])
    m.optimizer_G.step()
    m.optimizer_D.zero_grad(); loss_D.backward()
    for name, tag in NETS[1:]:
        for k, p in getattr(m, name).named_parameters():
            assert_grad_close(tag + ":" + k, p.grad.cpu().numpy(), g[f"{tag}_g_{k}"], rtol=5e-4, noise_biases=nb[tag])
    m.optimizer_D.step()
    for name, tag in NETS:
        for k, p in getattr(m, name).state_dict().items():
            new_ref, old = g[f"{tag}_p1_{k}"], g[f"{tag}_p_{k}"]
            d_ref, d_got = new_ref - old, p.cpu().numpy() - old
            assert np.max(np.abs(d_got)) <= 2.0001e-4 + 1e-7
            gr = g[f"{tag}_g_{k}"]
            strong = np.abs(gr) > 1e-3 * max(np.abs(gr).max(), 1e-12)
            if strong.any() and not k.endswith(".bias"):
                assert np.mean(np.sign(d_got[strong]) == np.sign(d_ref[strong])) > 0.999, (tag, k)


def test_discriminate_time_D_public(g):
    m = _model(g)
    lr_f, hr_f = (torch.from_numpy(g[k]).unsqueeze(1) for k in ("lr_frames", "hr_frames"))
    pred = m.discriminate_time_D(lr_f, hr_f)
    sd = {str(k): torch.from_numpy(g["T_p_" + str(k)]) for k in g["T_keys"]}
    ref = R.time_d_forward(sd, R.time_inputs(lr_f, hr_f, hr_f, MINV)[1])
    assert len(pred) == 2 and all(len(p) == 1 for p in pred)
    for p, r in zip(pred, ref):
        assert rel_err(p[-1].detach().float().cpu().numpy(), r.numpy()) < 1e-4


# ------------------------------------------------------------------------------------------ 5
def test_train_step_equals_forward_plus_manual_backward(g):
    a, b = _model(g), _model(g)
    lr, hr, noise = _inputs(g)
    la = a._phase_a(lr, hr, noise)                                 # the training step's schedule, gradients left in place
    a._phase_b()
    losses, _ = b.forward(lr, None, hr, None, noise=noise)         # the reference's schedule
    lb = dict(zip(b.loss_names, losses))
    bounds = loss_bounds(g)
    _check_losses(la, {k: float(v) for k, v in lb.items()}, bounds, "step vs forward ")
    _check_losses(la, dict(zip([str(n) for n in g["loss_names"]], g["loss_values"])), bounds, "step vs fixture ")
    b.optimizer_G.zero_grad(); (lb["G_GAN"] + lb["G_GAN_Feat"] + lb["G_GAN_t"]).backward()
    b.optimizer_D.zero_grad(); ((lb["D_fake"] + lb["D_real"]) * 0.5 + (lb["D_fake_t"] + lb["D_real_t"]) * 0.5).backward()
    for name, tag in NETS:
        nb = noise_bias_keys([k for k, _ in getattr(a, name).named_parameters()])
        for (k, pa), (_, pb) in zip(getattr(a, name).named_parameters(), getattr(b, name).named_parameters()):
            assert_grad_close(f"{tag}:{k}", pa.grad.cpu().numpy(), pb.grad.cpu().numpy(), rtol=5e-4, noise_biases=nb)
            assert_grad_close(f"fixture {tag}:{k}", pa.grad.cpu().numpy(), g[f"{tag}_g_{k}"], rtol=5e-4, noise_biases=nb)
    c = _model(g)
    c.train_step(lr, hr, noise=noise)
    assert c.optimizer_G.step_count == 1 and c.optimizer_D.step_count == 1
    for name, tag in NETS:                                         # train_step itself: the weights after it against the reference's
        for k, p in getattr(c, name).state_dict().items():
            assert torch.isfinite(p).all()
            old = g[f"{tag}_p_{k}"]
            d_ref, d_got = g[f"{tag}_p1_{k}"] - old, p.cpu().numpy() - old
            assert np.max(np.abs(d_got)) <= 2.0001e-4 + 1e-7
            gr = g[f"{tag}_g_{k}"]
            strong = np.abs(gr) > 1e-3 * max(np.abs(gr).max(), 1e-12)
            if strong.any() and not k.endswith(".bias"):
                assert np.mean(np.sign(d_got[strong]) == np.sign(d_ref[strong])) > 0.999, (tag, k)


def test_graphed_step_replays(g):
    m = _model(g, mask=False)
    lr, hr, _ = _inputs(g)
    n = 3 + 4                                                      # two eager steps, capture + first replay, then 4 replays
    for i in range(n):
        if i == 3:                                                 # from here on only replays change the weights
            assert m._graph_state['graphs'] is not None
            w0 = [p.detach().clone() for p in m.time_D.parameters()]
        ld = m.train_step_graphed(lr.cuda(), hr.cuda())
        assert all(np.isfinite(float(v)) for v in ld.values()), (i, ld)
    assert m._graph_state['graphs'] is not None
    assert set(ld) == set(m.loss_names)
    assert m.optimizer_G.steps_taken() == n and m.optimizer_D.steps_taken() == n
    assert all(not torch.equal(a, b.detach()) for a, b in zip(w0, m.time_D.parameters()) if a.dim() == 4)


@pytest.mark.parametrize("storage", ["bf16", "fp16"])
def test_16bit_steps_run_and_track_fp32(g, storage):
    kw = dict(fp16=True) if storage == "bf16" else dict(fp16=True, fp16_storage=True, loss_scale=1024.0)
    m = _model(g, **kw)
    lr, hr, noise = _inputs(g)
    losses, sr = m.forward(lr, None, hr, None, infer=True, noise=noise)
    ref = dict(zip([str(n) for n in g["loss_names"]], g["loss_values"]))
    for k, v in zip(m.loss_names, losses):
        print(storage, k, float(v), ref[k])
    for k, v in zip(m.loss_names, losses):
        assert abs(float(v) - ref[k]) < 0.1 * max(1.0, abs(ref[k])), (k, float(v), ref[k])     # the existing bf16 step test's bound
    assert rel_err(sr.detach().cpu().numpy(), g["sr"]) < 0.1
    m.train_step(lr, hr, noise=noise)
    for name, _ in NETS:
        assert all(torch.isfinite(p).all() for p in getattr(m, name).parameters())


# ------------------------------------------------------------------------------------------ 6
FAMILIES = ("gconv", "halo", "cls_skip", "march", "march_w", "wgrad", "splitk", "tile256", "tile128x192", "dfirst", "dlast", "c7",
            "thin_wgrad", "timed_pack", "timed_frames")

# One bf16 training step of the tiny geometry at ndf 64 with the flag OFF, recorded on the commit before this feature (same
# options, same inputs): the library's launch counters per family and the number of kernels torch operators launched themselves
# (the glue between the library calls, counted as tools/list_step_launches.py does).
PARENT_FLAG_OFF = {"gconv": 39, "halo": 0, "cls_skip": 0, "march": 0, "march_w": 0, "wgrad": 16, "splitk": 6, "tile256": 0,
                   "tile128x192": 0, "dfirst": 2, "dlast": 6, "c7": 0, "thin_wgrad": 4, "timed_pack": 0, "timed_frames": 0,
                   "aten_kernels": 28}


def _step_counts(g, **kw):
    """Launch counters and torch-operator kernel count of one bf16 training step at ndf 64 (the dedicated first-layer kernel
    serves <= 8 -> 64 channels in 16-bit storage only), random weights, the fixture's inputs."""
    from torch.profiler import ProfilerActivity, profile
    from pix2pixhdaudiosr_amd import _lib
    from pix2pixhdaudiosr_amd.models.models import create_model
    torch.manual_seed(0)
    m = create_model(make_opt(fp16=True, ndf=64, **kw))
    lr, hr, noise = _inputs(g)
    m.train_step(lr, hr, noise=noise)                              # workspaces, packed weights
    torch.cuda.synchronize()
    L = _lib.lib()
    L.p2phd_launch_count(None, 1)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        m.train_step(lr, hr, noise=noise)
        torch.cuda.synchronize()
    out = {k: int(L.p2phd_launch_count(k.encode(), 0)) for k in FAMILIES}
    # innermost aten operators that own kernels (a parent whose child owns the same kernels is skipped)
    out["aten_kernels"] = sum(len(ev.kernels) for ev in prof.events()
                              if ev.name.startswith("aten::") and ev.kernels
                              and not any(c.name.startswith("aten::") and c.kernels for c in ev.cpu_children))
    return out


def test_launch_accounting(g):
    off = _step_counts(g, use_time_D=False)
    on = _step_counts(g)
    print("off", off)
    print("on ", on)
    assert off == PARENT_FLAG_OFF                                  # flag off: the launch list of the commit before the feature
    assert on["timed_pack"] == 3                                   # dB fake, dB real, raw fake
    assert on["timed_frames"] == 2                                 # spectrogram -> frames and its adjoint, once each
    # time_D: num_D = 2 scales x 5 convs (first, three middle, last), three forward passes.  Backward: the raw pass carries the
    # generator loss down to the frames (input gradients of all 5 layers, no weight gradients); the two dB passes carry the
    # discriminator loss (weight gradients of all 5 layers, input gradients of layers 2..5: their input is data).
    scales, passes = 2, 3
    delta = {k: on[k] - off[k] for k in off if k != "aten_kernels"}
    assert delta["dfirst"] == scales * passes                      # forward of the 2 -> 64 first layers on the <= 8-channel kernel
    assert delta["dlast"] == scales * passes * 2                   # last layer: forward + input gradient, every pass
    assert delta["gconv"] == scales * (3 * passes                  # middle layers forward
                                       + 3 * passes                # input gradients of layers 2..4 (layer 5's is dlast's)
                                       + 1)                        # input gradient of layer 1: the raw pass only
    assert delta["wgrad"] == scales * 5 * 2                        # both dB passes, every layer
    assert delta["splitk"] >= 0                                    # (a tile-level choice of the launches counted above)
    for k in ("halo", "cls_skip", "march", "march_w", "tile256", "tile128x192", "c7", "thin_wgrad"):
        assert delta[k] == 0, (k, on[k], off[k])                   # planes this small take none of these routes, in either net


# ------------------------------------------------------------------------------------------ 7
def test_checkpoint_round_trip(g, tmp_path):
    m = _model(g, checkpoints_dir=str(tmp_path))
    m.save("latest")
    path = os.path.join(str(tmp_path), "time_d", "latest_net_time_D.pth")
    assert os.path.isfile(path)
    sd = torch.load(path, map_location="cpu")
    assert list(sd.keys()) == [str(k) for k in g["T_keys"]]
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), g["T_p_" + k])
    from pix2pixhdaudiosr_amd.models.models import create_model
    torch.manual_seed(99)
    m2 = create_model(make_opt(checkpoints_dir=str(tmp_path), continue_train=True))
    for k, v in m2.time_D.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), g["T_p_" + k]), k


# ------------------------------------------------------------------------------------------ 8
def test_full_size_time_losses(g):
    """The published run's geometry (n_fft 512, hop 256, win 512, segment 32512, netG local, ngf 48, num_D 2, B 4, fp32):
    sample 0's three time-domain losses against the restatement fed this model's own sr_result."""
    from pix2pixhdaudiosr_amd.models.models import create_model
    torch.manual_seed(7)
    opt = make_opt(n_fft=512, hop_length=256, win_length=512, netG="local", ngf=48, ndf=64, num_D=2, n_downsample_global=4,
                   n_blocks_global=9, n_local_enhancers=1, n_blocks_local=3)
    m = create_model(opt)
    gen = torch.Generator().manual_seed(8)
    B, T = 4, 32512
    hr = 0.1 * torch.randn(B, T, generator=gen)
    lr = 0.1 * torch.randn(B, T, generator=gen)
    losses, sr = m.forward(lr, None, hr, None, infer=True)
    # the losses are means over the batch: sample 0's own terms come from a pass of ours on sample 0 alone
    with torch.no_grad():
        _, _, _, _, _, _, hn, lnp = m.encode_input(lr, None, hr, None)
        srf = m.sr_frames(sr.detach(), lnp)
        lt = m._time_losses(sr.detach()[:1], {**lnp, 'frames': lnp['frames'][:1]}, {**hn, 'frames': hn['frames'][:1]})
    sd = {k: v.detach().cpu() for k, v in m.time_D.state_dict().items()}
    ref = R.time_losses(sd, lnp['frames'][:1].cpu().unsqueeze(1), hn['frames'][:1].cpu().unsqueeze(1),
                        R.sr_frames(sr.detach()[:1].cpu(), float(lnp['min']), float(lnp['max']), ALPHA, MINV, UP, m.window.cpu()),
                        MINV, opt.lambda_time, n_layers=3, num_D=2)
    assert rel_err(srf[:1].cpu().numpy(), R.sr_frames(sr.detach()[:1].cpu(), float(lnp['min']), float(lnp['max']), ALPHA, MINV, UP,
                                                      m.window.cpu())[:, 0].numpy()) < 1e-4
    bounds = loss_bounds(g)
    names = ("G_GAN_t", "D_real_t", "D_fake_t")
    _check_losses(dict(zip(names, lt)), dict(zip(names, (float(v) for v in ref))), bounds, "full size ")
    assert all(np.isfinite(float(v)) for v in losses)
