"""Zero-edit drop-in (round-4 review, missing 6): the reference's `train.py` / `generate_audio.py` import the hot path as
`models.mdct`, `models.models`, `util.util`, `dct.dct`, `data.data_loader` (train.py:12-17,56-58; generate_audio.py:6-8,21-23).
`python -m pix2pixhdaudiosr_amd.dropin <script>` serves exactly those names from this package through one meta-path finder
and leaves the out-of-scope modules (`options.*`, `util.visualizer`, ...) to the reference's own files.  CPU: names resolve
to the SAME objects, a script written against the reference's names runs under the launcher unedited, and every hot-path
import statement of its two scripts resolves (tests/golden/script_imports.json: those statements, read from the reference by
tools/gen_golden.py)."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = textwrap.dedent('''
    # a stand-in for the reference's script: the same module names, written for this test
    import inspect, sys
    from data.data_loader import CreateDataLoader
    from models.mdct import IMDCT2, MDCT2, MDCT4, IMDCT4
    from models.models import create_model
    from options.train_options import TrainOptions          # the reference's own (here: the stub beside this script)
    from util.visualizer import Visualizer                   # likewise
    from util.util import compute_matrics, kbdwin, imdct, mkdirs
    from dct.dct import IDCT, DCT
    import models.networks as networks
    import pix2pixhdaudiosr_amd.models.mdct as ours
    assert IMDCT2 is ours.IMDCT2 and TrainOptions().parse() == "stub options" and Visualizer.__module__ == "util.visualizer"
    assert networks.define_G.__module__.startswith("pix2pixhdaudiosr_amd.")
    idct = IDCT()
    assert idct.algorithm == "N" and "idct_op" in inspect.signature(IMDCT2.__init__).parameters
    ours._check_dct_op(idct, "idct"); ours._check_dct_op(DCT(algorithm="2N"), "dct")     # what IMDCT2(..., idct_op=IDCT()) checks
    import os
    assert os.environ["P2PHD_MDCT_TYPE"] == "mdct2"           # the launcher's default: the transform the eval code inverts
    print("DROPIN_OK", sys.argv[1:])
''')


def _fake_checkout(tmp_path):
    """The parts of a reference checkout that stay the reference's own: options/ and util/{__init__,visualizer}.py."""
    (tmp_path / "options").mkdir()
    (tmp_path / "options" / "__init__.py").write_text("")
    (tmp_path / "options" / "train_options.py").write_text(
        "from util import util\nclass TrainOptions:\n    def parse(self):\n        util.mkdirs([]); return 'stub options'\n")
    (tmp_path / "util").mkdir()
    (tmp_path / "util" / "__init__.py").write_text("")
    (tmp_path / "util" / "visualizer.py").write_text("from . import util\nclass Visualizer:\n    pass\n")
    (tmp_path / "train_like.py").write_text(SCRIPT)
    return tmp_path / "train_like.py"


def test_a_script_written_against_the_reference_names_runs_unedited(tmp_path):
    script = _fake_checkout(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("P2PHD_MDCT_TYPE", None)
    r = subprocess.run([sys.executable, "-m", "pix2pixhdaudiosr_amd.dropin", str(script), "--name", "x"], cwd=str(tmp_path),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "DROPIN_OK ['--name', 'x']" in r.stdout


def test_without_the_launcher_the_names_do_not_resolve(tmp_path):
    """Sensitivity: the same script run plainly fails on its first hot-path import (there is no `data` / `models` beside it)."""
    script = _fake_checkout(tmp_path)
    r = subprocess.run([sys.executable, str(script)], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "ModuleNotFoundError" in r.stderr


OUT_OF_SCOPE = ("options", "util.visualizer", "util.spectro_img", "util.html", "torchaudio", "debugpy")


@pytest.mark.parametrize("script", ["train.py", "generate_audio.py"])
def test_every_hot_path_import_of_the_reference_scripts_resolves(script):
    """Takes the reference script's import statements (tests/golden/script_imports.json) and resolves each one that is not
    CLI / UI / a third-party package through the alias finder, down to the imported attribute."""
    with open(os.path.join(ROOT, "tests", "golden", "script_imports.json")) as f:
        statements = json.load(f)[script]
    wanted = []
    for module, names in statements:
        top = module.split(".")[0]
        if top in ("models", "util", "dct", "data") and not module.startswith(OUT_OF_SCOPE):
            wanted += [(module, name) for name in names]
    assert len(wanted) >= 6, wanted
    code = ("import sys, importlib\nfrom pix2pixhdaudiosr_amd import dropin\ndropin.install()\n"
            "import types; sys.modules.setdefault('util', types.ModuleType('util')).__path__ = []\n"
            f"for mod, name in {wanted!r}:\n    m = importlib.import_module(mod)\n    assert hasattr(m, name), (mod, name)\n"
            "    assert m.__name__.startswith('pix2pixhdaudiosr_amd.'), (mod, m.__name__)\nprint('RESOLVED', len(%r))\n" % (wanted,))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"RESOLVED {len(wanted)}" in r.stdout
