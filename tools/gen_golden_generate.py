#!/usr/bin/env python3
"""Generate tests/golden/generate.npz: the REFERENCE's whole-file generation chain (generate_audio.py:27-47) on the CPU.

A tiny explicit-encoding, mode2-mask LocalEnhancer in the spirit of gen_golden.gen_model (the reference's own MDCT2,
n_fft 64, hop 32, ngf 8), segment_length 31 * 32, batchSize 2.  The input is the feeder fixture's excerpt of the
reference's test clip, cut to five segments and a remainder and band-limited to the low rate's 4 kHz by this tool (the
reference's torchaudio resampler is not what is under test), so AudioTestDataset.seg_pad_audio makes 6 segments, the last
one zero padded, and the loop runs three groups of two.  IMDCT2(idct_op=IDCT_2N_native()) stands in for the compiled
IDCT, as gen_golden.gen_mdct2 does.  Recorded: the generator's state dict, the low-rate audio, the torch.randn draw of
every to_spectro call, and the final audio.

Needs the reference checkout (gen_golden.REF); third-party imports are stubbed as in gen_golden.py.

Usage:  python tools/gen_golden_generate.py [--out tests/golden]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402
from gen_golden import _np, _stub_modules  # noqa: E402
from gen_golden_time_d import _build, _opt  # noqa: E402

SEG = 31 * 32
BATCH = 2


def gen_generate(out):
    from data.audio_dataset import AudioTestDataset
    from dct.dct_native import IDCT_2N_native
    from models.mdct import IMDCT2
    from util.util import imdct, kbdwin
    d = {}
    opt = _opt()
    opt.use_time_D = False
    opt.netG = "local"
    opt.segment_length, opt.batchSize = SEG, BATCH
    torch.manual_seed(4242)
    model = _build(opt)
    model.eval()
    for k, v in model.netG.state_dict().items():
        d[f"G_p_{k}"] = _np(v)

    F = np.load(os.path.join(out, "feeder.npz"))
    L = 5 * SEG + 500
    pcm = F["test_wav_excerpt_i16"][:L].astype(np.float64) / 32768.0
    spec = np.fft.rfft(pcm)
    spec[np.fft.rfftfreq(L, 1.0 / opt.hr_sampling_rate) > opt.lr_sampling_rate / 2] = 0.0     # the low rate's band
    lr = torch.from_numpy(np.fft.irfft(spec, L).astype(np.float32))[None]
    d["lr_audio"] = _np(lr)

    class Bare:
        segment_length = SEG
    seg = AudioTestDataset.seg_pad_audio(Bare(), lr)
    assert tuple(seg.shape) == (6, SEG)

    draws = []
    _randn = torch.randn

    def recording_randn(*a, **k):
        t = _randn(*a, **k)
        draws.append(_np(t))
        return t
    _imdct = IMDCT2(window=kbdwin, win_length=opt.win_length, hop_length=opt.hop_length, n_fft=opt.n_fft, center=opt.center,
                    out_length=opt.segment_length, device="cpu", idct_op=IDCT_2N_native())
    mag, pha, norms = [], [], []
    torch.manual_seed(99)
    torch.randn = recording_randn
    try:
        with torch.no_grad():
            for s0 in range(0, seg.shape[0], BATCH):                       # the DataLoader's batches (serial, batchSize 2)
                sr_spectro, lr_pha, norm_param, _ = model.inference(seg[s0:s0 + BATCH], None)
                mag.append(sr_spectro.abs().squeeze(1)); pha.append(lr_pha.squeeze(1)); norms.append(norm_param)
    finally:
        torch.randn = _randn
    assert len(draws) == 3
    up_ratio = opt.hr_sampling_rate / opt.lr_sampling_rate
    audio = [imdct(spectro=m, pha=p, norm_param=n, _imdct=_imdct, up_ratio=up_ratio, explicit_encoding=opt.explicit_encoding)
             for m, p, n in zip(mag, pha, norms)]
    audio = np.sqrt(up_ratio - 1) * torch.cat(audio, dim=0).view(1, -1)
    d["noise"] = np.concatenate(draws, axis=0)                             # [6, 2, mask_rows, frames]
    d["audio"] = _np(audio.float())
    d["norm_min"] = np.array([float(n["min"]) for n in norms]); d["norm_max"] = np.array([float(n["max"]) for n in norms])
    d["meta"] = np.array([opt.n_fft, opt.hop_length, SEG, BATCH, opt.hr_sampling_rate, opt.lr_sampling_rate])
    d["torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(out, "generate.npz"), **d)
    print("generate.npz", len(d), "arrays; audio", d["audio"].shape, "peak", float(np.abs(d["audio"]).max()), "dtype", audio.dtype,
          "noise", d["noise"].shape, os.path.getsize(os.path.join(out, "generate.npz")), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    a = ap.parse_args()
    _stub_modules()
    sys.path.insert(0, gg.REF)
    torch.set_num_threads(4)
    gen_generate(a.out)


if __name__ == "__main__":
    main()
