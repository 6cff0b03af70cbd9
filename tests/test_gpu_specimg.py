"""csrc/specimg.hip on the GPU: the renderer bit for bit against its numpy restatement (tests/_specimg_ref.py) between canaries,
the STFT against float64 torch.stft within a derived bound, and what the composed picture means (a tone sits in its row, silence
is the palette's first colour, two launches per picture)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import _specimg_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0xA5


def _lib():
    from pix2pixhdaudiosr_amd import _lib as L
    return L


def _count(reset=False):
    return _lib().lib().p2phd_launch_count(b"specimg", 1 if reset else 0)


def _lut():
    from pix2pixhdaudiosr_amd.generate import spectrogram_lut
    return spectrogram_lut()


_LUT_DEV = {}


def _lut_dev():
    if "lut" not in _LUT_DEV:
        _LUT_DEV["lut"] = torch.from_numpy(_lut()).to(DEV)
    return _LUT_DEV["lut"]


# ------------------------------------------------------------------------------------------
# render
# ------------------------------------------------------------------------------------------
def _render_raw(db, top_dev, range_db, W, H, gap):
    """p2phd_specimg_render into the middle of a buffer of canary bytes -> the picture as numpy; the canaries are checked."""
    L = _lib()
    R_, F, K = db.shape
    rows = R_ * H + (R_ - 1) * gap
    n, pad = rows * W * 3, 4096
    buf = torch.full((n + 2 * pad,), CANARY, dtype=torch.uint8, device=DEV)
    img = buf[pad:pad + n]
    rc = L.lib().p2phd_specimg_render(L.ptr(db), R_, F, K, L.ptr(top_dev), float(range_db), L.ptr(_lut_dev()), W, H, gap, L.ptr(img),
                                      L.stream_ptr())
    L.check(rc, "specimg_render")
    host = buf.cpu().numpy()
    assert (host[:pad] == CANARY).all() and (host[pad + n:] == CANARY).all(), "the renderer wrote outside its picture"
    return host[pad:pad + n].reshape(rows, W, 3)


def _plane(kind, R_, F, K, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ints":                                             # with range 85 the scale is 3 exactly: every index is an integer product
        return torch.randint(-100, 21, (R_, F, K), generator=g).float()
    x = torch.randn((R_, F, K), generator=g) * 30.0 - 40.0
    if kind == "special":                                          # NaN, +-inf, far above the top and far below the bottom
        m = torch.randint(0, 12, (R_, F, K), generator=g)
        for code, v in ((0, float('nan')), (1, float('inf')), (2, float('-inf')), (3, 1e30), (4, -1e30), (5, 400.0), (6, -400.0)):
            x[m == code] = v
    return x


# (R, F, K, W, H, gap) over R {1, 3}, F {1, 7, 300}, K {33, 129}, W {1, 5, 64, 640}, H {1, 16, 129, 200}, gap {0, 2}: W < F, = F (F = 1),
# > F; H < K, = K, > K; F = 1; one pixel; one tile of units and several.  Then three more: W = F beyond one frame, and a panel so
# tall that a workgroup takes fewer units (more than 768 rows), with a last tile that is not full.
SHAPES = [(1, 1, 33, 1, 1, 0), (1, 1, 33, 5, 16, 0), (3, 1, 129, 64, 200, 2), (1, 7, 33, 5, 16, 2), (1, 7, 33, 1, 129, 0),
          (1, 7, 129, 64, 129, 0), (3, 7, 33, 640, 200, 0), (1, 300, 33, 5, 1, 0), (3, 300, 129, 64, 16, 2), (3, 300, 33, 640, 200, 2),
          (1, 300, 129, 64, 200, 0), (3, 300, 129, 1, 129, 2),
          (3, 7, 33, 7, 33, 2), (1, 300, 129, 300, 129, 2), (1, 300, 33, 64, 1000, 0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%d_F%d_K%d_W%d_H%d_g%d" % s)
def test_render_is_the_restatement_bit_for_bit(shape):
    R_, F, K, W, H, gap = shape
    lut = _lut()
    for kind, range_db, fixed in (("ints", 85.0, 0.0), ("floats", 90.0, -3.25), ("special", 90.0, 7.5)):
        db = _plane(kind, R_, F, K, 11 + R_ + F + K).to(DEV)
        host = db.cpu().numpy()
        for top in (torch.full((1,), fixed, device=DEV), db.amax().reshape(1)):      # a fixed value; the plane's own maximum
            got = _render_raw(db, top, range_db, W, H, gap)
            want = R.render_ref(host, top.cpu().numpy()[0], range_db, W, H, gap, lut)
            assert got.shape == want.shape
            bad = np.argwhere((got != want).any(axis=-1))
            assert bad.size == 0, (kind, float(top), len(bad), bad[:5].tolist())
            assert (_render_raw(db, top, range_db, W, H, gap) == got).all()           # a second run: the same bytes
    if gap and R_ > 1:
        assert (got[H:H + gap] == 64).all()


def test_render_through_the_tensor_function_and_its_refusals():
    from pix2pixhdaudiosr_amd.generate import spectrogram_rgb
    L = _lib()
    db = _plane("floats", 2, 40, 65, 3).to(DEV)
    want = R.render_ref(db.cpu().numpy(), np.float32(-10.0), 60.0, 33, 70, 3, _lut())
    for top in (-10.0, torch.full((1,), -10.0, device=DEV)):
        img = spectrogram_rgb(db, top, 60.0, 33, 70, 3)
        assert img.dtype == torch.uint8 and tuple(img.shape) == (2 * 70 + 3, 33, 3) and img.is_cuda
        assert (img.cpu().numpy() == want).all()
    with pytest.raises(L.P2PHDError, match="width"):
        spectrogram_rgb(db, 0.0, 60.0, 0, 70, 3)
    with pytest.raises(L.P2PHDError, match="range"):
        spectrogram_rgb(db, 0.0, 0.0, 33, 70, 3)
    with pytest.raises(ValueError, match=r"\[R, F, K\]"):
        spectrogram_rgb(db[0], 0.0, 60.0, 33, 70, 3)
    with pytest.raises(ValueError, match="one value"):
        spectrogram_rgb(db, torch.zeros(2, device=DEV), 60.0, 33, 70, 3)


# ------------------------------------------------------------------------------------------
# STFT
# ------------------------------------------------------------------------------------------
# The bound, in amplitude a = 10^(db / 20) = |X| 4 / n_fft.  A radix-2/4 FFT of n points in fp32 (u = 2^-24) with twiddles rounded
# once returns X with |X_gpu - X| <= eta log2(n) sqrt(n) ||z||_2 up to O(u^2), eta = u + gamma_4 (sqrt 2 + u) ~ 6.7 u (Higham,
# Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 24.2: ||error||_2 <= log2(n) eta / (1 - log2(n) eta) ||X||_2, and
# ||X||_2 = sqrt(n) ||z||_2; a single bin's error is at most the whole vector's).  The input z = w x carries one more rounding per
# sample (the window product, and the table's own rounding), and two frames share one complex transform: z = w x_a + i w x_b, so
# an error of the transform is relative to the LARGER frame and lands on both when they are separated.  Doubling eta to 16 u
# covers both, with the norm taken as the maximum over the row's frames.  The scaling by (4 / n)^2 is exact.  The second term is
# what log10f and the final product may add: 3 ulp of an fp32 value of magnitude up to 200 (ulp 2^-16) are 3 * 2^-16 dB, a
# relative amplitude error of 3 * 2^-16 ln(10) / 20.
U = 2.0 ** -24
REL = 3.0 * 2.0 ** -16 * math.log(10.0) / 20.0
GEOMETRIES = [(64, 16), (256, 64), (1024, 256), (2048, 2048)]


def _tolerance(rows64, n_fft, hop, a_ref):
    norms = R.frame_norms_ref(rows64, n_fft, hop).max(axis=1)                          # [R]: max_g || w x_g ||_2
    return 16.0 * U * math.log2(n_fft) * (4.0 / n_fft) * math.sqrt(n_fft) * norms[:, None, None] + REL * a_ref


def _excerpt(n, start=0):
    F = np.load(os.path.join(GOLDEN, "feeder.npz"))
    x = F["test_wav_excerpt_i16"]
    assert start + n <= len(x)
    return torch.from_numpy(x[start:start + n].astype(np.float32) / 32768.0)


def _offset_rows(x, ld):
    """x [R, L] -> the same values as rows of pitch ld > L that start one float off a 16-byte boundary, NaN between the rows."""
    R_, L = x.shape
    buf = torch.full((R_ * ld + 5,), float('nan'), dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    rows = buf[1:1 + R_ * ld].view(R_, ld)[:, :L]
    rows.copy_(x)
    assert rows.data_ptr() % 16 == 4
    return rows


def _check_stft(rows_dev, rows_host, n_fft, hop):
    from pix2pixhdaudiosr_amd.generate import stft_db
    got = stft_db(rows_dev, n_fft, hop)
    R_, L = rows_host.shape
    assert tuple(got.shape) == (R_, 1 + L // hop, n_fft // 2 + 1) and got.dtype == torch.float32
    again = stft_db(rows_dev, n_fft, hop)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))                # the same bits on every run
    g = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all() and g.min() >= -200.0
    ref = R.stft_db_ref(rows_host, n_fft, hop)
    a_gpu, a_ref = 10.0 ** (g / 20.0), 10.0 ** (ref / 20.0)
    tol = _tolerance(rows_host.double().numpy(), n_fft, hop, a_ref)
    err = np.abs(a_gpu - a_ref)
    worst = float((err / tol).max())
    print(f"stft_db n_fft {n_fft} hop {hop} R {R_} L {L}: max |a_gpu - a_ref| / bound = {worst:.4f}")
    assert worst <= 1.0, (n_fft, hop, R_, L, worst, np.unravel_index((err / tol).argmax(), err.shape))
    return got, a_ref, tol


@pytest.mark.parametrize("n_fft,hop", GEOMETRIES)
def test_stft_is_within_the_bound_of_float64(n_fft, hop):
    for L in (1, n_fft // 2 - 1, n_fft, 5 * hop + 3, 4097):
        for R_ in (1, 3):
            x = torch.stack([(0.9, -0.6, 0.3)[r] * _excerpt(L, 700 * r) for r in range(R_)])
            rows = _offset_rows(x, L + 3 + 2 * R_)
            _check_stft(rows, x, n_fft, hop)
            if L == 4097 and R_ == 3:                              # a row of a call is the call on that row
                from pix2pixhdaudiosr_amd.generate import stft_db
                assert torch.equal(stft_db(rows, n_fft, hop)[1], stft_db(x[1:2].to(DEV), n_fft, hop)[0])


def test_stft_two_tones_sixty_db_apart():
    """The weaker tone's peak bin meets the bound, and the bound there is a small fraction of the tone: it is not vacuous."""
    n_fft, hop, L = 1024, 256, 4097
    t = torch.arange(L, dtype=torch.float64)
    k1, k2 = 100, 300
    x = (0.5 * torch.sin(2 * torch.pi * k1 * t / n_fft) + 0.5e-3 * torch.sin(2 * torch.pi * k2 * t / n_fft + 0.4)).float()[None]
    got, a_ref, tol = _check_stft(_offset_rows(x, L + 7), x, n_fft, hop)
    interior = slice(2, 1 + L // hop - 3)                          # frames that lie inside the clip
    assert np.allclose(a_ref[0, interior, k1], 0.5, rtol=1e-3) and np.allclose(a_ref[0, interior, k2], 0.5e-3, rtol=1e-2)
    assert (a_ref[0, interior].argmax(axis=1) == k1).all()
    assert (tol[0, interior, k2] < 0.05 * a_ref[0, interior, k2]).all()
    db = got[0].cpu().numpy()
    assert np.abs(db[interior, k1] - 20 * math.log10(0.5)).max() < 0.01 and np.abs(db[interior, k2] - 20 * math.log10(0.5e-3)).max() < 0.5
    # a full-scale sine reads 0 dB
    full = torch.sin(2 * torch.pi * k1 * t / n_fft).float()[None].to(DEV)
    from pix2pixhdaudiosr_amd.generate import stft_db
    assert abs(float(stft_db(full, n_fft, hop)[0, 5, k1])) < 1e-3


def test_stft_silence_is_one_bit_pattern():
    from pix2pixhdaudiosr_amd.generate import stft_db
    x = torch.stack([0.5 * _excerpt(1500), torch.zeros(1500), -0.5 * _excerpt(1500, 300)])
    for n_fft, hop in GEOMETRIES:
        db = stft_db(_offset_rows(x, 1503), n_fft, hop)
        floor = np.array([-200.0], dtype=np.float32).view(np.int32)[0]
        assert (db[1].cpu().numpy().view(np.int32) == floor).all()
        assert float(db[0].max()) > -100.0 and float(db[2].max()) > -100.0


def test_stft_refusals_and_the_empty_clip():
    from pix2pixhdaudiosr_amd.generate import stft_db
    L = _lib()
    x = torch.zeros((2, 256), device=DEV)
    out = torch.zeros((2, 64, 2049), device=DEV)
    tables = torch.zeros((3 * 2048,), device=DEV)
    _count(reset=True)
    for n_fft, hop, word in ((1000, 16, b"n_fft"), (32, 16, b"n_fft"), (4096, 16, b"n_fft"), (0, 16, b"n_fft"), (64, 0, b"hop"), (64, 65, b"hop"),
                             (64, -1, b"hop")):
        rc = L.lib().p2phd_stft_db(L.ptr(x), 256, 2, 256, n_fft, hop, L.ptr(tables), L.ptr(out), L.stream_ptr())
        assert rc == -1 and word in L.lib().p2phd_last_error(), (n_fft, hop)
    with pytest.raises(L.P2PHDError, match="n_fft"):
        stft_db(x, 1000, 16)
    with pytest.raises(L.P2PHDError, match="hop"):
        stft_db(x, 64, 65)
    empty = stft_db(torch.zeros((2, 0), device=DEV), 64, 16)                          # L = 0: nothing launched
    assert tuple(empty.shape) == (2, 0, 33)
    assert L.lib().p2phd_stft_db(L.ptr(x), 256, 0, 256, 64, 16, L.ptr(tables), L.ptr(out), L.stream_ptr()) == 0      # R = 0 neither
    torch.cuda.synchronize()
    assert _count() == 0 and float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------
# composition and meaning
# ------------------------------------------------------------------------------------------
def _tones(n_fft, L, bins):
    t = torch.arange(L, dtype=torch.float64)
    return torch.stack([torch.zeros(L, dtype=torch.float64) if k is None else 0.25 * torch.sin(2 * torch.pi * k * t / n_fft) for k in bins]).float()


def test_image_is_the_renderer_on_the_planes_at_their_maximum():
    from pix2pixhdaudiosr_amd.generate import spectrogram_image, stft_db
    x = torch.stack([0.9 * _excerpt(5000), 0.05 * _excerpt(5000, 1000)]).to(DEV)
    for plan in (dict(n_fft=256, hop=64, width=50, height=40, range_db=70.0, gap=1), dict(n_fft=1024, hop=256, width=64, height=600, gap=0)):
        _count(reset=True)
        img = spectrogram_image(x, **plan)
        assert _count() == 2                                       # the STFT and the renderer
        db = stft_db(x, plan['n_fft'], plan['hop']).cpu().numpy()
        want = R.render_ref(db, db.max(), plan.get('range_db', 90.0), plan['width'], plan['height'], plan['gap'], _lut())
        assert img.dtype == torch.uint8 and (img.cpu().numpy() == want).all()
        fixed = spectrogram_image(x, top_db=-6.0, **plan)
        assert (fixed.cpu().numpy() == R.render_ref(db, np.float32(-6.0), plan.get('range_db', 90.0), plan['width'], plan['height'],
                                                    plan['gap'], _lut())).all()
    with pytest.raises(ValueError, match="spectrogram width"):
        spectrogram_image(x, width=0)
    with pytest.raises(ValueError, match="at least one sample"):
        spectrogram_image(x[:, :0])


def test_a_tone_sits_in_its_row_and_silence_is_the_first_colour():
    from pix2pixhdaudiosr_amd.generate import spectrogram_image
    n_fft, hop, L, W, H, gap = 256, 64, 64 * 40, 20, 50, 2
    K = n_fft // 2 + 1
    bins = (100, None, 37)
    _count(reset=True)
    img = spectrogram_image(_tones(n_fft, L, bins).to(DEV), n_fft=n_fft, hop=hop, width=W, height=H, gap=gap).cpu().numpy()
    assert _count() == 2 and img.shape == (3 * H + 2 * gap, W, 3)
    lut = _lut()
    index = {tuple(int(c) for c in lut[i]): i for i in range(256)}
    assert len(index) == 256
    for r, k in enumerate(bins):
        panel = img[r * (H + gap):r * (H + gap) + H]
        if k is None:
            assert (panel == lut[0]).all()                         # silence: -200 dB, under any range
            continue
        idx = np.array([[index[tuple(int(c) for c in px)] for px in row] for row in panel])
        rows_with_k = [y for y in range(H) if (H - 1 - y) * K // H <= k < max((H - 1 - y) * K // H + 1, (H - y) * K // H)]
        assert len(rows_with_k) == 1
        interior = idx[:, 2:W - 2]                                 # columns whose frames lie inside the clip
        assert (interior.argmax(axis=0) == rows_with_k[0]).all()
        assert (interior.max(axis=0) == 255).all()                 # the loudest thing in the picture is the top of the scale
        assert ((interior == interior.max(axis=0)).sum(axis=0) == 1).all()
    assert (img[H:H + gap] == 64).all() and (img[2 * H + gap:2 * H + 2 * gap] == 64).all()
