"""The host side of FLAC output in whole-file generation: the container option's checks (plans.check_container), the output names
of a folder (plans.plan_folder's `ext`) and the command line's flags -- everything that is refused before a file is opened."""
import os

import pytest

from pix2pixhdaudiosr_amd.generate import plans


def test_check_container():
    assert plans.check_container('wav', None, False, 'float32', 48000, "t") is None
    assert plans.check_container('flac', None, False, 'pcm16', 48000, "t") == {'block': 4096, 'md5': False}
    assert plans.check_container('flac', 16, True, 'pcm24', 1048575, "t") == {'block': 16, 'md5': True}
    assert plans.check_container('flac', 65535, False, 'pcm16', 1, "t") == {'block': 65535, 'md5': False}
    for args, text in ((('ogg', None, False, 'pcm16', 48000), "container must be"), (('wav', 4096, False, 'pcm16', 48000), "options of container='flac'"),
                       (('wav', None, True, 'pcm16', 48000), "options of container='flac'"), (('flac', None, False, 'float32', 48000), "integer samples"),
                       (('flac', 15, False, 'pcm16', 48000), "flac_block"), (('flac', 65536, False, 'pcm16', 48000), "flac_block"),
                       (('flac', True, False, 'pcm16', 48000), "flac_block"), (('flac', 4096.0, False, 'pcm16', 48000), "flac_block"),
                       (('flac', None, False, 'pcm16', 1048576), "1048575")):
        with pytest.raises(ValueError, match=text):
            plans.check_container(*args, "t")


def test_plan_folder_names_the_outputs(tmp_path):
    d = tmp_path / "in"
    (d / "sub").mkdir(parents=True)
    for name in ("a.wav", "b.flac", "sub/c.WAV", "notes.txt"):
        (d / name).write_bytes(b"")
    out = str(tmp_path / "out")
    assert [os.path.relpath(p[2], out) for p in plans.plan_folder(str(d), out)] == ["a.wav", "sub/c.WAV"]             # as before
    assert [os.path.relpath(p[2], out) for p in plans.plan_folder(str(d), out, ext='.flac')] == ["a.flac", "sub/c.flac"]
    assert [os.path.relpath(p[2], out) for p in plans.plan_folder(str(d), out, ('wav', 'flac'), ext='.flac')] == ["a.flac", "b.flac", "sub/c.flac"]
    (d / "b.wav").write_bytes(b"")
    with pytest.raises(ValueError, match="both be written"):
        plans.plan_folder(str(d), out, ('wav', 'flac'), ext='.flac')
    with pytest.raises(ValueError, match="both be written"):
        plans.plan_folder(str(d), out, ('wav', 'flac'))
    assert len(plans.plan_folder(str(d), out, ext='.flac')) == 3                                                      # b.flac is not listed: no collision
    with pytest.raises(ValueError, match="ext"):
        plans.plan_folder(str(d), out, ext='.ogg')
    assert not os.path.exists(out)


def test_command_line_flags():
    from pix2pixhdaudiosr_amd.generate import cli
    ap = cli._parser()
    a = ap.parse_args(["--input", "x.wav", "--output", "y.wav", "--load_pretrain", "ckpt"])
    assert (a.container, a.flac_block, a.flac_md5) == ("wav", None, False)
    a = ap.parse_args(["--input", "x.wav", "--output", "y.flac", "--container", "flac", "--flac_block", "1152", "--flac_md5", "--load_pretrain", "ckpt"])
    assert (a.container, a.flac_block, a.flac_md5) == ("flac", 1152, True)
    with pytest.raises(SystemExit):
        ap.parse_args(["--input", "x.wav", "--output", "y.ogg", "--container", "ogg", "--load_pretrain", "ckpt"])
    help_text = ap.format_help()
    assert "second copy of the payload's size" in " ".join(help_text.split())
