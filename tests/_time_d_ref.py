"""Plain torch restatement of the reference's time-domain discriminator branch (--use_time_D), usable on CPU or GPU and
at any size.  It exists because the frozen oracle has no such branch and full-size cases cannot be fixtures; the small
case is pinned against the reference itself by tests/golden/time_d_step.npz, time_d_step_grads.npz and
time_d_step_after.npz (tools/gen_golden_time_d.py; three files so that each stays below the size limit of a committed file).

Restated lines (reference checkout): models/mdct.py:377-403 (MDCT2.forward(return_ola=True)), dct/dct_native.py:36-68
(IDCT_2N_native), models/pix2pixHD_model.py:229-232 (denormalize), :251-258 (to_frames), :314-320
(discriminate_time_D), :375-387 (the three passes), models/networks.py:300-360 (the discriminator) and :68-110 (LSGAN).
"""
import math

import torch
import torch.nn.functional as F


def mdct2_frames(signal, hop, win, window, center=True):
    """Windowed frames [.., F, win] of mdct.py:377-396, len(signal) quirk included (the padding follows the size of dim 0)."""
    signal_len = int(len(signal))
    start_pad = hop if center else 0
    additional = signal_len % hop
    end_pad = start_pad + (hop - additional if additional else 0)
    x = F.pad(signal, (start_pad, end_pad), mode='constant')
    return x.unfold(dimension=-1, size=win, step=hop) * window


def to_db(x, min_value):
    """aF.amplitude_to_DB(torch.abs(x), 20, min_value, 1) (pix2pixHD_model.py:317-318)."""
    return 20.0 * torch.log10(torch.clamp(torch.abs(x), min=min_value)) - 20.0


def idct_2n(X):
    """IDCT_2N_native over the last dimension by its definition: y[i] = X[0] + 2 sum_{k>=1} X[k] cos(pi (2i+1) k / 2N)."""
    N = X.shape[-1]
    i = torch.arange(N, dtype=torch.float64, device=X.device)
    C = 2.0 * torch.cos(math.pi * (2 * i[:, None] + 1) * i[None, :] / (2 * N))     # [i, k]
    C[:, 0] = 1.0
    return X @ C.to(X.dtype).T


def sr_frames(sr, mn, mx, alpha, min_value, up_ratio, window):
    """sqrt(up_ratio - 1) * window * to_frames(sr) as [B,1,F,win] (pix2pixHD_model.py:229-232, 251-258, 376)."""
    s = torch.abs(sr) * (mx - mn) + mn
    amp = 10.0 * torch.pow(torch.pow(10.0, 0.1 * s), 0.5) - min_value                # DB_to_amplitude(s, 10, 0.5) - min_value
    spec = (amp[..., 0, :, :] - amp[..., 1, :, :]) / (2 * alpha - 1)
    return (math.sqrt(up_ratio - 1) * window * idct_2n(spec.permute(0, 2, 1).contiguous())).unsqueeze(1)


def time_inputs(lr_frames, hr_frames, srf, min_value):
    """The three inputs of time_D in call order (pix2pixHD_model.py:379-386): dB fake (detached), dB real, RAW fake."""
    return (torch.cat((to_db(lr_frames, min_value), to_db(srf.detach(), min_value)), dim=1),
            torch.cat((to_db(lr_frames, min_value), to_db(hr_frames, min_value)), dim=1),
            torch.cat((lr_frames, srf), dim=1))


def time_d_forward(sd, x, n_layers=3, num_D=2):
    """MultiscaleDiscriminator(getIntermFeat=False).forward from its state dict `sd` (keys layer{i}.{j}.weight|bias,
    networks.py:300-360): per scale conv4x4 s2 + LeakyReLU, (n_layers - 1) x [conv s2, InstanceNorm, LeakyReLU], conv s1 +
    InstanceNorm + LeakyReLU, conv s1 -> 1 channel; scale num_D-1 first, the input average-pooled between scales."""
    res = []
    for i in range(num_D):
        keys = sorted({int(k.split('.')[1]) for k in sd if k.startswith('layer%d.' % (num_D - 1 - i))})
        h = x
        for n, j in enumerate(keys):
            w, b = sd['layer%d.%d.weight' % (num_D - 1 - i, j)], sd['layer%d.%d.bias' % (num_D - 1 - i, j)]
            stride = 2 if n < n_layers else 1
            h = F.conv2d(h, w, b, stride=stride, padding=2)
            if 0 < n < len(keys) - 1:
                h = F.instance_norm(h, eps=1e-5)
            if n < len(keys) - 1:
                h = F.leaky_relu(h, 0.2)
        res.append(h)
        if i != num_D - 1:
            x = F.avg_pool2d(x, 3, stride=2, padding=[1, 1], count_include_pad=False)
    return res


def gan_loss(preds, target_is_real):
    """GANLoss(use_lsgan=True) on a list of per-scale outputs (networks.py:100-110)."""
    return sum(F.mse_loss(p, torch.full_like(p, 1.0 if target_is_real else 0.0)) for p in preds)


def time_losses(sd, lr_frames, hr_frames, srf, min_value, lambda_time, n_layers=3, num_D=2):
    """(G_GAN_t, D_real_t, D_fake_t) of pix2pixHD_model.py:375-387."""
    x_fake, x_real, x_g = time_inputs(lr_frames, hr_frames, srf, min_value)
    d_fake = gan_loss(time_d_forward(sd, x_fake, n_layers, num_D), False) * lambda_time
    d_real = gan_loss(time_d_forward(sd, x_real, n_layers, num_D), True) * lambda_time
    g_gan = gan_loss(time_d_forward(sd, x_g, n_layers, num_D), True) * lambda_time
    return g_gan, d_real, d_fake
