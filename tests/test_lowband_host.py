"""The low-band splice of whole-file generation, host side: the row arithmetic that keeps mask noise out of the spliced
rows, the validation of the options, the command line, and the binding of p2phd_spectro_decode_spliced."""
import os
import re

import pytest

from conftest import ROOT

UP_RATIOS = (2, 3, 4, 6)
BINS = (64, 256, 512, 1024)


@pytest.mark.parametrize("up", UP_RATIOS)
@pytest.mark.parametrize("M", BINS)
def test_spliced_rows_hold_no_mask_noise(M, up):
    """to_spectro overwrites the top int(M (1 - 1 / up_ratio)) rows with noise (Pix2PixHDModel._mask_rows); util.imdct takes the
    rows below keep = int(M / up_ratio) from the input.  Every noise row is a row >= keep, for the integer up-ratios and for the
    float a SuperResolver computes (hr_sampling_rate / lr_sampling_rate)."""
    from pix2pixhdaudiosr_amd.util.util import lowband_keep_rows
    for ratio in (up, float(up), 48000 / (48000 // up)):
        keep = lowband_keep_rows(M, ratio)
        assert keep == int(M * (1 / ratio))                       # util.imdct's own expression
        mask_rows = int(M * (1 - 1 / ratio))                      # pix2pixHD_model.py:199 of the reference
        first_noise_row = M - mask_rows
        assert 0 < keep <= first_noise_row <= M, (M, ratio, keep, first_noise_row)
    assert lowband_keep_rows(M, 1) == M and lowband_keep_rows(M, 1.0) == M


def test_check_lowband_fade():
    from pix2pixhdaudiosr_amd.util.util import check_lowband_fade
    assert check_lowband_fade(0, 21) == 0 and check_lowband_fade(21, 21) == 21 and check_lowband_fade(0, 0) == 0
    for bad in (-1, 22, 2.0, "3", None, True):
        with pytest.raises(ValueError, match=r"imdct: lowband_fade"):
            check_lowband_fade(bad, 21)


def test_check_lowband():
    """What SuperResolver.__init__ runs on its two options (constructing one needs a device)."""
    from pix2pixhdaudiosr_amd.generate import LOWBANDS, check_lowband
    assert LOWBANDS == ('model', 'input')
    assert check_lowband('model', 0, 64, 6.0) == ('model', 0, 10)
    assert check_lowband('input', 10, 64, 6.0) == ('input', 10, 10)
    assert check_lowband('input', 4, 512, 2.0) == ('input', 4, 256)
    assert check_lowband('input', 64, 64, 1.0) == ('input', 64, 64)           # up_ratio 1: every row is the input's
    for bad in ('lr', 'Input', None, 0, ''):
        with pytest.raises(ValueError, match=r"lowband must be 'model' or 'input'"):
            check_lowband(bad, 0, 64, 6.0)
    for bad in (-1, 11, 1.5):
        with pytest.raises(ValueError, match=r"SuperResolver: lowband_fade"):
            check_lowband('input', bad, 64, 6.0)
    with pytest.raises(ValueError, match=r"lowband_fade"):
        check_lowband('model', 11, 64, 6.0)                       # validated whichever band is chosen


def test_signatures_carry_the_options():
    """The new parameters sit behind the existing ones with today's behaviour as the default."""
    import inspect
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    from pix2pixhdaudiosr_amd.util import util as U
    p = inspect.signature(U.imdct).parameters
    assert list(p)[:7] == ["spectro", "pha", "norm_param", "_imdct", "min_value", "up_ratio", "explicit_encoding"]
    assert list(p)[7:] == ["lr_spectro", "lowband_fade"] and p["lr_spectro"].default is None and p["lowband_fade"].default == 0
    q = inspect.signature(SuperResolver.__init__).parameters
    assert list(q)[1:7] == ["model", "opt", "overlap", "batch", "graph", "reference_amplitude"]
    assert q["lowband"].default == 'model' and q["lowband_fade"].default == 0


def test_cli_flags():
    from pix2pixhdaudiosr_amd.generate import _parser
    base = ["--input", "a.wav", "--output", "b.wav", "--load_pretrain", "ck"]
    a = _parser().parse_args(base)
    assert a.lowband == "model" and a.lowband_fade == 0
    b = _parser().parse_args(base + ["--lowband", "input", "--lowband_fade", "4", "--channels", "all", "--metrics_ext"])
    assert b.lowband == "input" and b.lowband_fade == 4 and b.channels == "all" and b.metrics_ext is True
    for bad in (["--lowband", "lr"], ["--lowband_fade", "1.5"], ["--lowband"]):
        with pytest.raises(SystemExit):
            _parser().parse_args(base + bad)
    assert "--lowband" in _parser().format_help() and "--lowband_fade" in _parser().format_help()


def test_binding_matches_the_header():
    """_lib lists p2phd_spectro_decode_spliced with one ctypes argument per parameter of the header's declaration: 14 (four
    tensors and the min/max pair, B, F, M, channels, keep_rows, fade_rows, min_value, scale, spec, stream)."""
    import ctypes as C
    from pix2pixhdaudiosr_amd import _lib
    with open(os.path.join(ROOT, "include", "p2phd.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bint\s+p2phd_spectro_decode_spliced\s*\(([^)]*)\)\s*;", src)
    assert m, "p2phd_spectro_decode_spliced is not declared in include/p2phd.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [p.rsplit(" ", 1)[1] for p in params] == ["sr_log_spectro", "lr_log_spectro", "pha", "norm_min_max", "B", "F", "M",
                                                    "channels", "keep_rows", "fade_rows", "min_value", "scale", "spec", "stream"]
    res, args = _lib.SIGNATURES["p2phd_spectro_decode_spliced"]
    assert res is C.c_int and len(args) == len(params) == 14
    want = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}
    assert args == [want[p.rsplit(" ", 1)[0]] for p in params]
    # its neighbour, for comparison: the same list without lr_log_spectro and fade_rows
    assert len(_lib.SIGNATURES["p2phd_spectro_decode_signed"][1]) == 12
