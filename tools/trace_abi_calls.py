"""The sequence of C-ABI calls (include/p2phd.h) the host issues in one EAGER training step of the tiny golden model
(tests/test_gpu_model.py: InstanceNorm trunk with ResnetBlocks, stride-2 pairs, 2-scale discriminator with pooling), for
five variants: fp32, bf16, bf16 with P2PHD_DPAIR=0, bf16 with P2PHD_BSUM=0, bf16 with use_time_D (tests/test_gpu_time_d.py).

    python tools/trace_abi_calls.py [OUT]        (GPU; OUT defaults to stdout)

One line per call: the function, the fourteen p2phd_conv_desc fields of a descriptor argument, the value of every integer
and float argument, and `null` / `set` for every pointer (`set=argK` when it equals pointer argument K of the same
call).  No addresses, so two logs are comparable: a change of the host glue (_ops.py, networks._run, the model) that claims
to leave every launch alone shows an empty `diff` against the log of its parent commit.
The tool only observes the arguments the host passes."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pix2pixhdaudiosr_amd import _lib  # noqa: E402

DESC_FIELDS = [n for n, _ in _lib.ConvDesc._fields_]


def _address(a):
    """Address a pointer argument carries (0 = NULL), whichever way the caller spelled it."""
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if isinstance(a, (C.c_void_p, C.c_char_p)):
        return C.cast(a, C.c_void_p).value or 0
    if isinstance(a, bytes):
        return id(a)                                               # (a name: never equal to a device pointer)
    return C.addressof(getattr(a, "_obj", a))                      # byref(x) / an array / a structure


class Recorder:
    """Stands in for one loaded library: every ABI function logs its arguments, then runs."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _lib.SIGNATURES:
            return fn
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            self._log.append(self.line(name, argtypes, args))
            return fn(*args)

        setattr(self, name, call)
        return call

    @staticmethod
    def line(name, argtypes, args):
        out, seen = [], {}
        for k, (a, ty) in enumerate(zip(args, argtypes)):
            desc = getattr(a, "_obj", None)
            if isinstance(desc, _lib.ConvDesc):
                out.append("desc(" + " ".join(f"{f}={getattr(desc, f)}" for f in DESC_FIELDS) + ")")
            elif isinstance(a, bytes):
                out.append(repr(a))
            elif ty in (C.c_float, C.c_double):
                out.append(repr(float(a)))
            elif ty in (C.c_int, C.c_int64, C.c_size_t):
                out.append(str(int(a)))
            else:
                addr = _address(a)
                out.append("null" if not addr else "set" + (f"=arg{seen[addr]}" if addr in seen else ""))
                if addr:
                    seen.setdefault(addr, k)
        return f"{name}({', '.join(out)})"


def _golden(*files):
    d = {}
    for f in files:
        z = np.load(os.path.join(ROOT, "tests", "golden", f))
        d.update({k: z[k] for k in z.files})
    return d


def variants():
    import test_gpu_model as TM
    import test_gpu_time_d as TT
    gm = _golden("model_step.npz")
    gt = _golden("time_d_step.npz")
    yield "fp32", {}, lambda: TM._model(gm), gm
    yield "bf16", {}, lambda: TM._model(gm, fp16=True), gm
    yield "bf16 P2PHD_DPAIR=0", {"P2PHD_DPAIR": "0"}, lambda: TM._model(gm, fp16=True), gm
    yield "bf16 P2PHD_BSUM=0", {"P2PHD_BSUM": "0"}, lambda: TM._model(gm, fp16=True), gm
    yield "bf16 use_time_D", {}, lambda: TT._model(gt, fp16=True), gt


def main():
    torch.cuda.set_device(0)
    _lib.lib()
    log = []
    for kind, l in list(_lib._libs.items()):
        _lib._libs[kind] = Recorder(l, log)
    lines = []
    for name, env, build, g in variants():
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            model = build()
            lr, hr, noise = (torch.from_numpy(g[k]) for k in ("lr", "hr", "mask_noise"))
            del log[:]                                             # (construction and weight loading are not the step)
            model.train_step(lr, hr, noise=noise)
            torch.cuda.synchronize()
        finally:
            for k, v in saved.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        lines.append(f"# {name}: {len(log)} calls")
        lines.extend(log)
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
