"""The host-only conv queries (sizes, layouts, eligibility) are pinned: every conv layer of the bench workloads (cfg2, cfg3,
cfg5: generators, local enhancers, 2- and 3-scale discriminators) at N = 1, 2, 8, 32, plus each dedicated kernel's accepted
shape and one near miss per condition of its shape rule, in f32 and bf16 (w_layout 1 where it is allowed), on both libraries,
under the default options and with each routing option flipped on its own.

The fixture tests/golden/conv_queries.json holds the answers of the commit before the conv routing was gathered into one
place (convapi.hip); answers must not change with the code's structure.  It was recorded from that commit's build with

    python tests/test_conv_queries.py --record

Encoding: `base` lists the bf16 library's answers under the default options, one row per case; every other (library, option)
run is stored as {case index: row} for the rows that differ from `base`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_queries.json")

# option flips, one at a time (name, flipped value, default)
OPTIONS = [("march", 0, 1), ("dfirst", 0, 1), ("dlast", 0, 1), ("c7_generic", 1, 0), ("reflect_generic", 1, 0), ("cls_skip", 0, 1)]
LIBS = ("bf16", "f16")

# layer = (C, H, W, K, R, S, stride, pad, pad_mode, transposed, opad)


def generator_layers(ngf, n_down, n_blocks, H, W, strip_last=False):
    """GlobalGenerator (networks.py:190-208) on an H x W plane with 2 input / output channels."""
    out = [(2, H, W, ngf, 7, 7, 1, 3, 1, 0, 0)]
    for i in range(n_down):
        c = ngf * 2 ** i
        out.append((c, H >> i, W >> i, 2 * c, 3, 3, 2, 1, 0, 0, 0))
    dim, h, w = ngf * 2 ** n_down, H >> n_down, W >> n_down
    if n_blocks:
        out.append((dim, h, w, dim, 3, 3, 1, 1, 1, 0, 0))
    for i in range(n_down):
        c = ngf * 2 ** (n_down - i)
        out.append((c, H >> (n_down - i), W >> (n_down - i), c // 2, 3, 3, 2, 1, 0, 1, 1))
    if not strip_last:
        out.append((ngf, H, W, 2, 7, 7, 1, 3, 1, 0, 0))
    return out


def local_enhancer_layers(ngf, n_down, n_blocks_global, n_blocks_local, H, W):
    """LocalEnhancer with one local level (networks.py:135-163): the global generator on the half plane, the local branch."""
    out = generator_layers(2 * ngf, n_down, n_blocks_global, (H + 1) // 2, (W + 1) // 2, strip_last=True)
    out += [(2, H, W, ngf, 7, 7, 1, 3, 1, 0, 0), (ngf, H, W, 2 * ngf, 3, 3, 2, 1, 0, 0, 0)]
    if n_blocks_local:
        out.append((2 * ngf, H // 2, W // 2, 2 * ngf, 3, 3, 1, 1, 1, 0, 0))
    out += [(2 * ngf, H // 2, W // 2, ngf, 3, 3, 2, 1, 0, 1, 1), (ngf, H, W, 2, 7, 7, 1, 3, 1, 0, 0)]
    return out


def discriminator_layers(num_D, H, W, ndf=64, input_nc=4):
    """MultiscaleDiscriminator of 3-layer NLayerDiscriminators (networks.py:300-373), 3 x 3 stride-2 average pool between scales."""
    out = []
    for _ in range(num_D):
        h, w = H, W
        stages = [(input_nc, ndf, 2), (ndf, 2 * ndf, 2), (2 * ndf, 4 * ndf, 2), (4 * ndf, 8 * ndf, 1), (8 * ndf, 1, 1)]
        for cin, cout, s in stages:
            out.append((cin, h, w, cout, 4, 4, s, 2, 0, 0, 0))
            h, w = (h + 4 - 4) // s + 1, (w + 4 - 4) // s + 1
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def bench_layers():
    out = generator_layers(48, 4, 9, 512, 256) + discriminator_layers(2, 512, 256)                      # cfg2
    out += local_enhancer_layers(48, 4, 3, 2, 512, 256)                                                  # cfg3 (its D is cfg2's)
    out += local_enhancer_layers(64, 4, 0, 3, 1024, 512) + discriminator_layers(3, 1024, 512)            # cfg5
    out.append((2048, 32, 16, 2048, 3, 3, 1, 1, 1, 0, 0))                                               # cfg5's global trunk
    return list(dict.fromkeys(out))


def dedicated_layers():
    """Each dedicated kernel's accepted shape, then one near miss per condition of its shape rule."""
    def vary(base, **kw):
        names = ("C", "H", "W", "K", "R", "S", "stride", "pad", "pad_mode", "transposed", "opad")
        d = dict(zip(names, base))
        d.update(kw)
        return tuple(d[n] for n in names)
    out = []
    dlast = (512, 65, 33, 1, 4, 4, 1, 2, 0, 0, 0)
    out += [dlast, vary(dlast, C=128), vary(dlast, C=96), vary(dlast, C=640), vary(dlast, K=2), vary(dlast, R=3, S=3),
            vary(dlast, stride=2), vary(dlast, pad=1), vary(dlast, pad_mode=1), vary(dlast, H=512, W=256)]
    dfirst = (4, 512, 256, 64, 4, 4, 2, 2, 0, 0, 0)
    out += [dfirst, vary(dfirst, C=1), vary(dfirst, C=8), vary(dfirst, C=9), vary(dfirst, K=32), vary(dfirst, R=3, S=3),
            vary(dfirst, stride=1), vary(dfirst, pad=1), vary(dfirst, pad_mode=1), vary(dfirst, H=1, W=1), vary(dfirst, H=4096, W=2048)]
    c7_in = (2, 64, 256, 48, 7, 7, 1, 3, 1, 0, 0)
    out += [c7_in, vary(c7_in, C=3), vary(c7_in, K=40), vary(c7_in, K=16), vary(c7_in, K=144), vary(c7_in, K=80), vary(c7_in, K=96),
            vary(c7_in, R=5, S=5, pad=2), vary(c7_in, stride=2), vary(c7_in, pad=2), vary(c7_in, pad_mode=0), vary(c7_in, H=60),
            vary(c7_in, W=192), vary(c7_in, K=8)]
    c7_out = (48, 64, 256, 2, 7, 7, 1, 3, 1, 0, 0)
    out += [c7_out, vary(c7_out, C=40), vary(c7_out, C=144), vary(c7_out, C=80), vary(c7_out, C=16), vary(c7_out, C=128),
            vary(c7_out, K=3), vary(c7_out, R=5, S=5, pad=2), vary(c7_out, stride=2), vary(c7_out, pad=2), vary(c7_out, pad_mode=0),
            vary(c7_out, H=60), vary(c7_out, W=192), vary(c7_out, H=6), vary(c7_out, C=8), vary(c7_out, C=4)]
    m_conv = (48, 64, 256, 96, 3, 3, 2, 1, 0, 0, 0)
    out += [m_conv, vary(m_conv, C=64), vary(m_conv, K=128), vary(m_conv, R=4, S=4), vary(m_conv, stride=1), vary(m_conv, pad=2),
            vary(m_conv, pad_mode=1), vary(m_conv, H=63), vary(m_conv, W=192), vary(m_conv, H=6)]
    m_convt = (96, 32, 128, 48, 3, 3, 2, 1, 0, 1, 1)
    out += [m_convt, vary(m_convt, C=128), vary(m_convt, K=64), vary(m_convt, opad=0), vary(m_convt, pad=0), vary(m_convt, W=96),
            vary(m_convt, H=2), vary(m_convt, R=4, S=4)]
    thin = (4, 64, 64, 64, 4, 4, 2, 2, 0, 0, 0)
    out += [thin, vary(thin, K=8), vary(thin, K=4), vary(thin, K=128), vary(thin, K=256), vary(thin, C=3), vary(thin, pad=1),
            vary(thin, pad_mode=1), vary(thin, transposed=1, pad=1)]
    out += [vary(c7_in, K=4), vary(c7_in, K=256), vary(c7_out, C=256), vary(c7_in, H=30, W=30)]
    refl = (64, 16, 16, 64, 3, 3, 1, 1, 1, 0, 0)
    out += [refl, vary(refl, H=3), vary(refl, W=3), vary(refl, H=4, W=4), vary(refl, pad=2, H=8), vary(refl, R=5, S=5, pad=2),
            vary(refl, stride=2), vary(refl, K=2), vary(refl, C=2), vary(refl, C=60), vary(refl, K=4, C=8)]
    kmaj = (64, 16, 16, 64, 3, 3, 1, 1, 0, 0, 0)
    out += [kmaj, vary(kmaj, C=56), vary(kmaj, K=56), vary(kmaj, R=5, S=5, pad=2), vary(kmaj, C=72), vary(kmaj, stride=2),
            vary(kmaj, transposed=1, opad=0)]
    return list(dict.fromkeys(out))


def cases():
    """(N, layer, dtype, w_layout) in a fixed order; w_layout 1 is added where p2phd_conv_kmajor_ok allows it (decided by the
    library under test, so a library that changed its answer shows up as a missing or extra case)."""
    out = []
    for layer in bench_layers():
        for n in (1, 2, 8, 32):
            for dt in (0, 1):
                out.append((n,) + layer + (dt,))
    for layer in dedicated_layers():
        for n in (2, 32):
            for dt in (0, 1):
                out.append((n,) + layer + (dt,))
    return out


def _desc(_lib, case, w_layout):
    n, C, H, W, K, R, S, stride, pad, pad_mode, transposed, opad, dt = case
    return _lib.ConvDesc(N=n, C=C, H=H, W=W, K=K, R=R, S=S, stride=stride, pad=pad, pad_mode=pad_mode, transposed=transposed,
                         opad=opad, dtype=dt, w_layout=w_layout)


def answers(L, _lib):
    import ctypes as C
    rows = []
    for case in cases():
        kmaj = L.p2phd_conv_kmajor_ok(C.byref(_desc(_lib, case, 0)))
        for wl in ((0, 1) if kmaj else (0,)):
            d = C.byref(_desc(_lib, case, wl))
            ho, wo = C.c_int32(-1), C.c_int32(-1)
            rc = L.p2phd_conv_out_size(d, C.byref(ho), C.byref(wo))
            rows.append([wl, rc, ho.value, wo.value,
                         L.p2phd_conv_packed_bytes(d, 0), L.p2phd_conv_packed_bytes(d, 1),
                         L.p2phd_conv_pack_layout(d, 0), L.p2phd_conv_pack_layout(d, 1),
                         L.p2phd_conv_fwd_workspace_bytes(d), L.p2phd_conv_dgrad_workspace_bytes(d), L.p2phd_conv_wgrad_workspace_bytes(d),
                         L.p2phd_conv_dgrad_bsum_ok(d), L.p2phd_conv_dgrad_bsum_pays(d), L.p2phd_conv_dgrad_bsum_workspace_bytes(d),
                         L.p2phd_conv_reflect_extras_elems(d), kmaj, L.p2phd_conv_lazy_ok(d),
                         L.p2phd_conv_fp8_eligible(d), L.p2phd_conv_fp8_packed_bytes(d)])
    return rows


def collect():
    from pix2pixhdaudiosr_amd import _lib
    runs = {}
    for kind in LIBS:
        L = _lib.lib(kind)
        runs[f"{kind}:default"] = answers(L, _lib)
        for name, value, default in OPTIONS:
            assert L.p2phd_set_option(name.encode(), value) == 0, name
            try:
                runs[f"{kind}:{name}={value}"] = answers(L, _lib)
            finally:
                assert L.p2phd_set_option(name.encode(), default) == 0, name
    base = runs.pop("bf16:default")
    diffs = {}
    for key, rows in runs.items():
        assert len(rows) == len(base), key
        diffs[key] = {str(i): r for i, r in enumerate(rows) if r != base[i]}
    return {"cases": len(cases()), "base": base, "diffs": diffs}


def test_conv_queries_match_the_recorded_answers():
    want = json.load(open(FIXTURE))
    got = collect()
    assert got["cases"] == want["cases"]
    assert len(got["base"]) == len(want["base"])
    bad = [i for i, (g, w) in enumerate(zip(got["base"], want["base"])) if g != w]
    assert not bad, [(cases()[i] if i < len(cases()) else i, got["base"][i], want["base"][i]) for i in bad[:5]]
    assert sorted(got["diffs"]) == sorted(want["diffs"])
    for key in want["diffs"]:
        assert got["diffs"][key] == want["diffs"][key], key


def test_corpus_reaches_every_option():
    """The fixture is only as good as its corpus: each option that moves a query moves one here.  dfirst and dlast move none:
    their packed copies and workspaces are sized by shape alone."""
    want = json.load(open(FIXTURE))
    for name, value, _ in OPTIONS:
        for kind in LIBS:
            moved = want["diffs"][f"{kind}:{name}={value}"]
            assert (not moved) if name in ("dfirst", "dlast") else moved, (kind, name)


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with open(FIXTURE, "w") as f:
        json.dump(collect(), f, separators=(",", ":"))
    print(f"wrote {FIXTURE}: {os.path.getsize(FIXTURE)} bytes")
