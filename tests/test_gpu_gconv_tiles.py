"""The launch counters say what the host-only tile query said: for the layers tests/_exact.py reaches each special tile of the
gather-GEMM with (256 x 256, the HALO loop on 256 x 192 and 256 x 128, the tap-skipping merged launch, 128 x 192), one forward
and one input gradient run through the C ABI with the split-K tail off, and `tile256`, `tile128x192`, `halo`, `cls_skip` and the
launch count itself equal what p2phd_conv_gconv_tiles answers for the same descriptor, launch form and options.  (The outputs
are checked bit for bit on the way, as in tests/test_gpu_conv_exact.py, whose runners these are.)"""
import ctypes as C

import pytest
import torch

import _exact as X
import test_gpu_conv_exact as E
from test_gconv_tile_query import query

pytestmark = pytest.mark.gpu

FWD, DGRAD, DGRAD_EXPANDED, DGRAD_EXTRAS = 0, 1, 2, 3          # launch forms of the query
STATS, SUMS = 1, 2                                             # its flags

# (layer, call, form, flags, options): `call` runs the launch, (form, flags) is the same launch in the query's terms
CASES = [(l, "fwd_stats", FWD, STATS, {}) for l in X.HALO_FWD]
CASES += [(l, "dgrad_rx", DGRAD_EXTRAS, 0, {}) for l in X.HALO_DGRAD]
CASES += [(X.HALO_DGRAD[0], "dgrad", DGRAD_EXPANDED, 0, {})]
CASES += [(X.HALO_FWD[0], "fwd_stats", FWD, STATS, {"gconv_halo": 0})]
CASES += [(X.TILE128X192_FWD, "fwd_stats", FWD, STATS, {}), (X.TILE128X192_DGRAD, "dgrad_bsum", DGRAD, SUMS, {}),
          (X.TILE128X192_FWD, "fwd_stats", FWD, STATS, {"tile128x192": 0})]
CASES += [(X.TILE256, "fwd", FWD, 0, {"gconv_bm": 512}), (X.TILE256, "dgrad", DGRAD, 0, {"gconv_bm": 512})]
CASES += [(l, "fwd_stats", FWD, STATS, {}) for l in X.CLS_SKIP_FWD] + [(l, "dgrad", DGRAD, 0, {}) for l in X.CLS_SKIP_DGRAD]
CASES += [(X.CLS_SKIP_FWD[0], "fwd_stats", FWD, STATS, {"cls_skip": 0}), (X.at_batch(X.CLS_SKIP_DGRAD[0], 1), "dgrad", DGRAD, 0, {})]


@pytest.mark.parametrize("l,call,form,flags,opts", CASES, ids=lambda v: getattr(v, "name", None) or (v if isinstance(v, str) else None))
def test_launch_counters_say_what_the_tile_query_said(l, call, form, flags, opts):
    ops = E._ops()
    Lb = ops.lib_for(torch.bfloat16)
    with E.options(Lb, splitk_tail=0, **opts):
        spec = ops.ConvSpec(l.cin, l.cout, l.k, l.stride, l.pad, l.pad_mode, l.transposed, l.opad, False, E.NONE)
        said = query(Lb, spec.desc(*l.shape, torch.bfloat16), form, flags)
        assert not isinstance(said, int), (l.name, form, flags, said)
        if call.startswith("fwd"):
            cnt = E.run_fwd(l, "bf16", E.RELU if call == "fwd" else E.NONE, call == "fwd_stats")
        else:
            cnt = E.run_dgrad(l, "bf16", False, {"dgrad": "plain", "dgrad_rx": "rx", "dgrad_bsum": "bsum"}[call], E.RELU)
    want = {"gconv": len(said), "halo": sum(t[5] for t in said), "cls_skip": sum(t[7] for t in said),
            "tile256": sum(t[:2] == [256, 256] for t in said), "tile128x192": sum(t[:2] == [128, 192] for t in said), "splitk": 0}
    assert {k: cnt[k] for k in want} == want, (l.name, call, opts, said, cnt)
    E._dedicated_idle(cnt, l.name)


def test_the_cases_reach_every_special_tile():
    """Host part of the above: under these options the query names each special tile at least once (a case list that stopped
    reaching one would compare zeros with zeros)."""
    ops = E._ops()
    Lb = ops.lib_for(torch.bfloat16)
    seen = set()
    for l, call, form, flags, opts in CASES:
        with E.options(Lb, **opts):
            spec = ops.ConvSpec(l.cin, l.cout, l.k, l.stride, l.pad, l.pad_mode, l.transposed, l.opad, False, E.NONE)
            for t in query(Lb, spec.desc(*l.shape, torch.bfloat16), form, flags):
                seen.add(tuple(t[:2]) + (t[5], t[7]))
    assert {(256, 256, 0, 0), (256, 192, 1, 0), (256, 128, 1, 0), (256, 192, 0, 1), (128, 192, 0, 0)} <= seen, sorted(seen)
