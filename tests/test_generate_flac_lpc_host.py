"""The host side of the FLAC writer's LPC option in whole-file generation: the option's checks (plans.check_container's flac_lpc,
flacio.check_lpc), the command line's flag and the per-file line -- everything that is refused before a file is opened."""
import pytest

from pix2pixhdaudiosr_amd.generate import plans


def test_check_container_flac_lpc():
    # off: what the call returned before the option existed, with and without the keyword
    assert plans.check_container('wav', None, False, 'float32', 48000, "t", flac_lpc=None) is None
    assert plans.check_container('flac', None, False, 'pcm16', 48000, "t") == {'block': 4096, 'md5': False}
    assert plans.check_container('flac', None, False, 'pcm16', 48000, "t", flac_lpc=None) == {'block': 4096, 'md5': False}
    assert plans.check_container('flac', 65535, True, 'pcm24', 48000, "t", flac_lpc=0) == {'block': 65535, 'md5': True}
    assert plans.check_container('flac', None, False, 'pcm16', 48000, "t", flac_lpc=12) == {'block': 4096, 'md5': False, 'lpc': 12}
    assert plans.check_container('flac', 16384, True, 'pcm24', 44100, "t", flac_lpc=1) == {'block': 16384, 'md5': True, 'lpc': 1}
    assert plans.check_container('flac', 16, False, 'pcm16', 1, "t", flac_lpc=8) == {'block': 16, 'md5': False, 'lpc': 8}
    for args, lpc, text in ((('wav', None, False, 'pcm16', 48000), 4, "option of container='flac'"), (('wav', None, False, 'pcm16', 48000), 0, "option of container='flac'"),
                            (('flac', None, False, 'pcm16', 48000), 13, "flac_lpc must be"), (('flac', None, False, 'pcm16', 48000), -1, "flac_lpc must be"),
                            (('flac', None, False, 'pcm16', 48000), True, "flac_lpc must be"), (('flac', None, False, 'pcm16', 48000), 4.0, "flac_lpc must be"),
                            (('flac', None, False, 'pcm16', 48000), "4", "flac_lpc must be"), (('flac', 16385, False, 'pcm16', 48000), 1, "at most 16384"),
                            (('flac', 65535, False, 'pcm24', 48000), 12, "at most 16384"), (('flac', None, False, 'float32', 48000), 4, "integer samples"),
                            (('flac', 15, False, 'pcm16', 48000), 4, "flac_block"), (('ogg', None, False, 'pcm16', 48000), 4, "container must be")):
        with pytest.raises(ValueError, match=text):
            plans.check_container(*args, "t", flac_lpc=lpc)


def test_flacio_check_lpc():
    from pix2pixhdaudiosr_amd.data import flacio
    assert (flacio.MAX_LPC_ORDER, flacio.MAX_LPC_BLOCK) == (plans.FLAC_LPC_MAX, plans.FLAC_LPC_BLOCK) == (12, 16384)
    for M, block in ((0, 65535), (1, 16384), (12, 16)):
        flacio.check_lpc(M, block)
    for M, block, text in ((13, 4096, "LPC order"), (-1, 4096, "LPC order"), (None, 4096, "LPC order"), (True, 4096, "LPC order"), (1, 16385, "at most 16384")):
        with pytest.raises(ValueError, match=text):
            flacio.check_lpc(M, block)


def test_command_line_flag(capsys):
    from pix2pixhdaudiosr_amd.generate import cli
    ap = cli._parser()
    a = ap.parse_args(["--input", "x.wav", "--output", "y.wav", "--load_pretrain", "ckpt"])
    assert a.flac_lpc is None
    a = ap.parse_args(["--input", "x.wav", "--output", "y.flac", "--container", "flac", "--flac_lpc", "12", "--load_pretrain", "ckpt"])
    assert (a.container, a.flac_lpc) == ("flac", 12)
    with pytest.raises(SystemExit):
        ap.parse_args(["--input", "x.wav", "--output", "y.flac", "--container", "flac", "--flac_lpc", "twelve", "--load_pretrain", "ckpt"])
    assert "--flac_lpc" in ap.format_help() and "never longer" in " ".join(ap.format_help().split())
    capsys.readouterr()
    # refused by main before anything is loaded: the flag without the container, outside the range, with too large a block
    for extra, word in ((["--flac_lpc", "4"], "container"), (["--container", "flac", "--flac_lpc", "13"], "flac_lpc"),
                        (["--container", "flac", "--flac_lpc", "-1"], "flac_lpc"), (["--container", "flac", "--flac_lpc", "1", "--flac_block", "16385"], "16384")):
        with pytest.raises(SystemExit):
            cli.main(["--input", "x.wav", "--output", "y.flac", "--load_pretrain", "/nonexistent/ckpt"] + extra)
        assert word in capsys.readouterr().err


def test_per_file_line(capsys):
    from pix2pixhdaudiosr_amd.generate import cli
    f = {'block': 4096, 'frames': 3, 'bytes': 500, 'pcm_bytes': 1000, 'md5': None}
    cli._print_flac("a.flac", f, 'pcm16')
    off = capsys.readouterr().out
    assert off == "a.flac: FLAC 16 bit, 3 frames of 4096, 500 bytes (50.0 % of the PCM)\n"      # the line of before the option
    cli._print_flac("a.flac", dict(f, lpc=12, md5="00ff"), 'pcm24')
    assert capsys.readouterr().out == "a.flac: FLAC 24 bit, 3 frames of 4096, 500 bytes (50.0 % of the PCM), MD5 00ff, LPC up to order 12\n"
