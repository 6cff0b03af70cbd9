"""Host side of the spectrogram picture (no GPU): the validation of its options, the command line's refusals before any model
is loaded, the palette, the numpy restatement of the renderer (tests/_specimg_ref.py) on hand-made planes, and the host-only
C entries of csrc/specimg.hip."""
import ctypes

import numpy as np
import pytest

import _specimg_ref as R


# ------------------------------------------------------------------------------------------
# check_spectrogram
# ------------------------------------------------------------------------------------------
def test_check_accepts_the_defaults_and_fills_them_in():
    from pix2pixhdaudiosr_amd.generate import SPECTROGRAM_DEFAULTS, check_spectrogram
    assert SPECTROGRAM_DEFAULTS == {'n_fft': 1024, 'hop': 256, 'width': 1600, 'height': 512, 'range_db': 90.0, 'gap': 2}
    assert check_spectrogram() == SPECTROGRAM_DEFAULTS
    assert check_spectrogram(**SPECTROGRAM_DEFAULTS) == SPECTROGRAM_DEFAULTS
    plan = check_spectrogram(n_fft=64, hop=64, width=1, height=16384, range_db=1, gap=0, top_db=-3.5, channel=7)
    assert plan == {'n_fft': 64, 'hop': 64, 'width': 1, 'height': 16384, 'range_db': 1.0, 'gap': 0}
    assert check_spectrogram(n_fft=2048, hop=1, gap=64)['n_fft'] == 2048


@pytest.mark.parametrize("name,values", [
    ("n_fft", (0, 32, 63, 1000, 4096, 1024.0, True, "1024")),
    ("hop", (0, -1, 1025, 256.0, True)),
    ("width", (0, -5, 16385, 1600.0, True)),
    ("height", (0, 16385, 5.5, False)),
    ("range_db", (0, 0.0, -90.0, float('inf'), float('nan'), "90", True)),
    ("gap", (-1, 65, 2.0, True)),
    ("top_db", (float('inf'), float('-inf'), float('nan'), "0", True)),
    ("channel", (-1, 1.0, True, "0")),
])
def test_check_rejects_each_bad_argument_by_name(name, values):
    from pix2pixhdaudiosr_amd.generate import check_spectrogram
    for v in values:
        with pytest.raises(ValueError, match=r"who: spectrogram %s must .*got " % name):
            check_spectrogram(who="who", **{name: v})


def test_hop_is_held_to_the_n_fft_in_use():
    from pix2pixhdaudiosr_amd.generate import check_spectrogram
    assert check_spectrogram(n_fft=64, hop=64)['hop'] == 64
    with pytest.raises(ValueError, match=r"hop must be an int in \[1, n_fft = 64\], got 65"):
        check_spectrogram(n_fft=64, hop=65)
    with pytest.raises(ValueError, match=r"hop must be an int in \[1, n_fft = 128\], got 256"):
        check_spectrogram(n_fft=128)                               # the default hop does not fit a short transform


# ------------------------------------------------------------------------------------------
# the command line: refused before any model is loaded
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,message", [
    (["--spectrogram_size", "0x10"], "spectrogram width must be an int in [1, 16384], got 0"),
    (["--spectrogram_n_fft", "1000"], "spectrogram n_fft must be a power of two in [64, 2048], got 1000"),
    (["--spectrogram_range_db", "0"], "spectrogram range_db must be finite and > 0, got 0.0"),
])
def test_cli_rejects_bad_options_before_anything_is_loaded(tmp_path, capsys, extra, message):
    from pix2pixhdaudiosr_amd import generate as G
    # --load_pretrain names a folder that does not exist: reading its opt.txt would raise FileNotFoundError, not SystemExit
    base = ["--input", str(tmp_path / "in.wav"), "--output", str(tmp_path / "out.wav"), "--load_pretrain", str(tmp_path / "none"),
            "--spectrogram", str(tmp_path / "p.png")]
    with pytest.raises(SystemExit) as e:
        G.main(base + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
    assert not (tmp_path / "p.png").exists()


def test_cli_rejects_suboptions_without_the_option_and_bad_sizes(tmp_path, capsys):
    from pix2pixhdaudiosr_amd import generate as G
    base = ["--input", str(tmp_path / "in.wav"), "--output", str(tmp_path / "out.wav"), "--load_pretrain", str(tmp_path / "none")]
    with pytest.raises(SystemExit) as e:
        G.main(base + ["--spectrogram_hop", "128"])
    assert e.value.code == 2 and "--spectrogram_hop is an option of --spectrogram PATH" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        G.main(base + ["--spectrogram", str(tmp_path / "p.png"), "--spectrogram_size", "1600"])
    assert e.value.code == 2 and "expected WIDTHxHEIGHT" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                           # a file's picture is a file
        G.main(base + ["--spectrogram", str(tmp_path)])
    assert e.value.code == 2 and "--spectrogram must be a file too" in capsys.readouterr().err


def test_api_refuses_suboptions_without_a_path_and_unknown_ones():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    spec = SuperResolver._spectrogram_spec
    assert spec(None, 0, None, "enhance_file") is None
    with pytest.raises(ValueError, match=r"options of spectrogram=PATH"):
        spec(None, 1, None, "enhance_file")
    with pytest.raises(ValueError, match=r"options of spectrogram=PATH"):
        spec(None, 0, {'hop': 64}, "enhance_file")
    with pytest.raises(ValueError, match=r"unknown spectrogram_opts \['colour'\]"):
        spec("p.png", 0, {'colour': 1}, "enhance_file")
    got = spec("p.png", 1, {'hop': 64, 'top_db': -6.0}, "enhance_file")
    assert got['path'] == "p.png" and got['channel'] == 1 and got['top_db'] == -6.0 and got['plan']['hop'] == 64


# ------------------------------------------------------------------------------------------
# the palette
# ------------------------------------------------------------------------------------------
def test_lut_shape_anchors_and_monotone_luminance():
    from pix2pixhdaudiosr_amd.generate import SPECTROGRAM_LUT_ANCHORS, spectrogram_lut
    lut = spectrogram_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    for i, rgb in SPECTROGRAM_LUT_ANCHORS:
        assert tuple(int(c) for c in lut[i]) == rgb
    assert SPECTROGRAM_LUT_ANCHORS[0][0] == 0 and SPECTROGRAM_LUT_ANCHORS[-1][0] == 255
    luma = lut.astype(np.int64) @ np.array([299, 587, 114])        # Rec.601, integers
    assert (np.diff(luma) >= 0).all()
    assert luma[0] < 8 * 1000 and luma[255] > 230 * 1000            # near-black to pale
    assert tuple(lut[0]) != tuple(lut[255])
    assert len({tuple(c) for c in lut}) == 256                     # every level has a colour of its own
    # between two anchors: integer linear interpolation
    assert tuple(int(c) for c in lut[32]) == (15, 10, 72) and tuple(int(c) for c in lut[160]) == (215, 90, 90)
    assert (spectrogram_lut() == lut).all()


# ------------------------------------------------------------------------------------------
# render_ref on hand-made planes
# ------------------------------------------------------------------------------------------
def _grey_lut():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def test_ref_same_size_is_the_plane_flipped():
    F, K = 5, 4
    db = (np.arange(F * K, dtype=np.float32).reshape(1, F, K) * 3.0) - 85.0      # -85 .. -28 in steps of 3; range 85: scale 3
    img = R.render_ref(db, 0.0, 85.0, F, K, 0, _grey_lut())
    assert img.shape == (K, F, 3) and img.dtype == np.uint8
    want = (np.arange(F * K).reshape(F, K) * 9).T[::-1]            # idx = (v + 85) * 3; row y shows bin K - 1 - y
    assert (img[..., 0] == want).all() and (img[..., 1] == want).all() and (img[..., 2] == want).all()


def test_ref_pooling_is_the_maximum_and_upsampling_repeats():
    db = np.array([[[-80, -70, -60, -50], [-40, -75, -65, -10], [-85, -85, -85, -85], [-30, -85, -20, -84]]], dtype=np.float32)
    img = R.render_ref(db, 0.0, 85.0, 2, 2, 0, _grey_lut())[..., 0]               # 2:1 both ways
    # column 0: frames 0-1, column 1: frames 2-3; row 0: bins 2-3, row 1: bins 0-1
    want_db = np.array([[-10, -20], [-40, -30]], dtype=np.float32)
    assert (img == ((want_db + 85) * 3).astype(np.uint8)).all()
    wide = R.render_ref(db, 0.0, 85.0, 8, 4, 0, _grey_lut())[..., 0]              # W = 2 F repeats columns
    same = R.render_ref(db, 0.0, 85.0, 4, 4, 0, _grey_lut())[..., 0]
    assert (wide[:, 0::2] == same).all() and (wide[:, 1::2] == same).all()
    tall = R.render_ref(db, 0.0, 85.0, 4, 8, 0, _grey_lut())[..., 0]              # H = 2 K repeats rows
    assert (tall[0::2] == same).all() and (tall[1::2] == same).all()
    # uneven: F = 4 frames onto 3 columns -- [0, 1), [1, 2), [2, 4)
    odd = R.render_ref(db, 0.0, 85.0, 3, 4, 0, _grey_lut())[..., 0]
    assert (odd[:, 0] == same[:, 0]).all() and (odd[:, 1] == same[:, 1]).all() and (odd[:, 2] == np.maximum(same[:, 2], same[:, 3])).all()


def test_ref_gap_rows_are_grey_and_panels_keep_their_place():
    db = np.stack([np.full((3, 2), -85.0, np.float32), np.full((3, 2), 0.0, np.float32), np.full((3, 2), -42.5, np.float32)])
    img = R.render_ref(db, 0.0, 85.0, 3, 2, 2, _grey_lut())
    assert img.shape == (3 * 2 + 2 * 2, 3, 3)
    assert (img[0:2] == 0).all() and (img[4:6] == 255).all() and (img[8:10] == 128).all()      # 127.5 rounds to even
    assert (img[2:4] == 64).all() and (img[6:8] == 64).all()
    assert R.render_ref(db, 0.0, 85.0, 3, 2, 0, _grey_lut()).shape == (6, 3, 3)


def test_ref_nan_and_infinities():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    db = np.array([[[nan, -85.0 + 10, inf, -inf, nan, 1e30, -1e30]]], dtype=np.float32)      # F = 1, K = 7
    img = R.render_ref(db, 0.0, 85.0, 1, 7, 0, _grey_lut())[::-1, 0, 0]            # bottom row first: bin order
    assert img.tolist() == [0, 30, 255, 0, 0, 255, 0]
    # a NaN beside a number does not win; +inf beside anything does
    assert R.render_ref(db[:, :, 0:2], 0.0, 85.0, 1, 1, 0, _grey_lut())[0, 0, 0] == 30
    assert R.render_ref(db[:, :, 0:3], 0.0, 85.0, 1, 1, 0, _grey_lut())[0, 0, 0] == 255
    assert R.render_ref(db[:, :, 3:5], 0.0, 85.0, 1, 1, 0, _grey_lut())[0, 0, 0] == 0
    # a NaN top: every finite value maps to 0, +inf still to 255
    assert R.render_ref(db, nan, 85.0, 1, 7, 0, _grey_lut())[::-1, 0, 0].tolist() == [0, 0, 255, 0, 0, 0, 0]


def test_ref_rounds_half_to_even_in_float32():
    db = np.array([[[-85.0 + 0.5 / 3, -85.0 + 1.5 / 3, -85.0 + 2.5 / 3]]], dtype=np.float32)
    got = R.render_ref(db, 0.0, 85.0, 1, 3, 0, _grey_lut())[::-1, 0, 0].tolist()
    lo, scale = np.float32(0.0) - np.float32(85.0), np.float32(255.0) / np.float32(85.0)
    assert scale == np.float32(3.0)
    assert got == [int(np.rint((v - lo) * scale)) for v in db[0, 0]]


# ------------------------------------------------------------------------------------------
# the host-only C entries
# ------------------------------------------------------------------------------------------
def test_host_entries_report_sizes_and_refuse_bad_arguments():
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    assert L.p2phd_specimg_image_bytes(3, 1600, 512, 2) == (3 * 512 + 2 * 2) * 1600 * 3
    assert L.p2phd_specimg_image_bytes(1, 1, 1, 64) == 3
    assert L.p2phd_specimg_image_bytes(2, 16384, 16384, 0) == 2 * 16384 * 16384 * 3
    for bad, word in (((0, 10, 10, 0), b"panel"), ((1, 0, 10, 0), b"width"), ((1, 10, 16385, 0), b"height"), ((1, 10, 10, 65), b"gap"),
                      ((1, 10, 10, -1), b"gap"), ((65536, 10, 10, 0), b"panels")):
        assert L.p2phd_specimg_image_bytes(*bad) == 0
        assert word in L.p2phd_last_error(), (bad, L.p2phd_last_error())
    assert L.p2phd_stft_db_frames(1, 64, 16) == 1 and L.p2phd_stft_db_frames(4097, 1024, 256) == 17
    assert L.p2phd_stft_db_frames(2048, 2048, 2048) == 2 and L.p2phd_stft_db_frames(15, 64, 16) == 1
    for bad, word in (((100, 1000, 16), b"n_fft"), ((100, 32, 16), b"n_fft"), ((100, 4096, 16), b"n_fft"), ((100, 64, 0), b"hop"),
                      ((100, 64, 65), b"hop"), ((0, 64, 16), b"L"), ((-1, 64, 16), b"L")):
        assert L.p2phd_stft_db_frames(*bad) == 0
        assert word in L.p2phd_last_error(), (bad, L.p2phd_last_error())
    assert L.p2phd_specimg_tables_floats(1024) == 3 * 1024
    assert L.p2phd_specimg_tables_floats(100) == 0 and b"n_fft" in L.p2phd_last_error()
    # the launching entries check what needs no device first
    null = ctypes.c_void_p(0)
    assert L.p2phd_stft_db(null, 10, 1, 10, 1000, 16, null, null, null) == -1 and b"n_fft" in L.p2phd_last_error()
    assert L.p2phd_stft_db(null, 10, 1, 10, 64, 65, null, null, null) == -1 and b"hop" in L.p2phd_last_error()
    assert L.p2phd_stft_db(null, 9, 1, 10, 64, 16, null, null, null) == -1 and b"pitch" in L.p2phd_last_error()
    assert L.p2phd_stft_db(null, 0, 3, 0, 64, 16, null, null, null) == 0                  # L = 0: nothing to do
    for bad, word in (((1, 5, 33, null, 0.0, null, 8, 8, 0), b"range"), ((1, 5, 33, null, float('inf'), null, 8, 8, 0), b"range"),
                      ((1, 5, 33, null, 90.0, null, 0, 8, 0), b"width"), ((1, 5, 33, null, 90.0, null, 8, 8, 65), b"gap"),
                      ((1, 5, 0, null, 90.0, null, 8, 8, 0), b"bins"), ((1, 0, 33, null, 90.0, null, 8, 8, 0), b"frame")):
        assert L.p2phd_specimg_render(null, *bad, null, null) == -1
        assert word in L.p2phd_last_error(), (bad, L.p2phd_last_error())
    assert L.p2phd_specimg_render(null, 0, 5, 33, null, 90.0, null, 8, 8, 0, null, null) == 0     # no panel: nothing to do


def test_tables_fill_is_the_float64_formula_rounded_once():
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    for n in (64, 256, 1024, 2048):
        buf = np.full(3 * n + 1, np.float32(7.0))
        assert L.p2phd_specimg_tables_fill(n, ctypes.c_void_p(buf.ctypes.data)) == 0
        j = np.arange(n, dtype=np.float64)
        tw = np.exp(-2j * np.pi * j / n)
        assert (buf[0:2 * n:2] == tw.real.astype(np.float32)).all() and (buf[1:2 * n:2] == tw.imag.astype(np.float32)).all()
        assert (buf[2 * n:3 * n] == R.window_ref(n).astype(np.float32)).all()
        assert buf[3 * n] == np.float32(7.0)                       # nothing behind the table is touched
        assert buf[2 * n] == 0.0 and buf[2 * n + n // 2] == 1.0
    assert L.p2phd_specimg_tables_fill(100, ctypes.c_void_p(buf.ctypes.data)) == -1 and b"n_fft" in L.p2phd_last_error()
    assert L.p2phd_specimg_tables_fill(64, ctypes.c_void_p(0)) == -1 and b"null" in L.p2phd_last_error()
