"""CPU checks of the time-domain discriminator feature (--use_time_D): tests/_time_d_ref.py reproduces the reference's
arrays and losses recorded in tests/golden/time_d_step.npz, the fixture regenerates bit-identically from its generator
where the reference checkout is present, and Pix2PixHDModel._check_supported accepts the flag exactly where the
reference's own code path works."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _time_d_ref as R
from conftest import GOLDEN, ROOT, rel_err

FILES = ("time_d_step.npz", "time_d_step_grads.npz", "time_d_step_after.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "time_d_step.npz"))


def _t(g, k):
    return torch.from_numpy(g[k])


def test_ref_reproduces_fixture_arrays_and_losses(g):
    """Same torch, same CPU, fp32: only the summation order differs from the reference -> 1e-6 relative."""
    window = _t(g, "window")
    for clip in ("lr", "hr"):
        fr = R.mdct2_frames(_t(g, clip), 32, 64, window)
        assert rel_err(fr.numpy(), g[clip + "_frames"]) < 1e-6
    srf = R.sr_frames(_t(g, "sr"), _t(g, "lr_min"), _t(g, "lr_max"), 0.6, 1e-7, 6.0, window)
    assert rel_err(srf[:, 0].numpy(), g["sr_frames"]) < 1e-6
    lr_f, hr_f = _t(g, "lr_frames").unsqueeze(1), _t(g, "hr_frames").unsqueeze(1)
    xs = R.time_inputs(lr_f, hr_f, _t(g, "sr_frames").unsqueeze(1), 1e-7)
    for x, k in zip(xs, ("time_in_fake_db", "time_in_real_db", "time_in_g_raw")):
        assert torch.isfinite(x).all()
        assert rel_err(x.numpy(), g[k]) < 1e-6, k
    # exact zeros (centre padding, silent stretches) land on 20 log10(min_value) - 20, not on -inf
    assert (g["lr_frames"] == 0).any() and float(xs[1].min()) == pytest.approx(20 * np.log10(1e-7) - 20, abs=1e-4)
    sd = {str(k): _t(g, "T_p_" + str(k)) for k in g["T_keys"]}
    got = R.time_losses(sd, lr_f, hr_f, _t(g, "sr_frames").unsqueeze(1), 1e-7, float(g["lambda_time"]))
    ref = dict(zip([str(n) for n in g["loss_names"]], g["loss_values"]))
    for k, v in zip(("G_GAN_t", "D_real_t", "D_fake_t"), got):
        assert abs(float(v) - ref[k]) <= 1e-6 * max(1.0, abs(ref[k])), (k, float(v), ref[k])


def test_loss_names_order(g):
    assert [str(n) for n in g["loss_names"]] == ['G_GAN', 'G_GAN_Feat', 'G_GAN_t', 'D_real_t', 'D_fake_t', 'D_real', 'D_fake']


def test_fixture_regenerates_bit_identically(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_golden
    finally:
        sys.path.pop(0)
    if not os.path.isdir(gen_golden.REF):
        pytest.skip("the reference checkout is not on this machine")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_golden_time_d.py"), "--out", str(tmp_path)],
                          stdout=subprocess.DEVNULL)                # stderr passes: a failing generator shows its traceback
    for f in FILES:
        a, b = np.load(os.path.join(GOLDEN, f)), np.load(os.path.join(str(tmp_path), f))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (f, k)


def _opt(**kw):
    o = dict(explicit_encoding=True, mdct_type="mdct2", n_fft=64, win_length=64, hop_length=32, use_time_D=True,
             use_hifigan_D=False, mask_mode="mode2", phase_encoding_mode=None, no_vgg_loss=True, no_instance=True,
             no_lsgan=False, label_nc=0, pool_size=0, use_match_loss=False, instance_feat=False, label_feat=False)
    o.update(kw)
    return SimpleNamespace(**o)


def test_check_supported_accepts_time_D_where_the_reference_path_works():
    from pix2pixhdaudiosr_amd.models.pix2pixHD_model import Pix2PixHDModel
    m = Pix2PixHDModel()
    m._check_supported(_opt())                                      # accepted: explicit encoding, MDCT2, n_fft == win_length
    for kw, word in ((dict(explicit_encoding=False), "explicit_encoding"), (dict(mdct_type="mdct4"), "mdct2"),
                     (dict(n_fft=128), "win_length"), (dict(use_hifigan_D=True), "use_hifigan_D")):
        with pytest.raises(NotImplementedError) as e:
            m._check_supported(_opt(**kw))
        assert word in str(e.value), (kw, str(e.value))
    m._check_supported(_opt(use_time_D=False, mdct_type="mdct4"))   # flag off: nothing new is demanded
