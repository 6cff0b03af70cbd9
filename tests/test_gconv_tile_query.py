"""The gather-GEMM's tile choice is pinned on the host: p2phd_conv_gconv_tiles (csrc/convapi.hip) says, without a GPU, which
tile gconv_choose_tile (csrc/gconv.hip) gives every generic launch of a layer.  Corpus: that of tests/test_conv_queries.py (the
bench layers of cfg2 / cfg3 / cfg5 at N = 1, 2, 8, 32 and the dedicated-kernel shapes, f32 and the 16-bit type, w_layout 1 where
allowed) plus the layers of EXTRA, in every launch form and flag combination, on both libraries, under the default options and
with each tile option set on its own.

The fixture tests/golden/gconv_tiles.json was recorded with

    python tests/test_gconv_tile_query.py --record

from the FIRST state of the change that introduced the chooser: the old ladder of `return launch_gconv_cfg<...>` statements
with each of them replaced, one for one, by `return GconvTile{...}` and nothing else changed.  The chooser as it is written
now has to reproduce those answers exactly.

Encoding (base plus diffs, as conv_queries.json, with two look-up tables in front): `tiles` lists the distinct 9-int launch
records, `rows` the distinct per-case rows -- one answer per entry of FORMS, an answer being a negative error code or the list
of its launches' indices into `tiles` --, `base` the row index of every case for the bf16 library under the default options,
and `diffs` {run: {case index: row index}} the cases of every other (library, option) run that differ from `base`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import test_conv_queries as Q  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gconv_tiles.json")

# (form, flags): form 0 forward, 1 input gradient, 2 / 3 exact-grid reflect input gradient (expanded dy / extras), 4 fp8 forward;
# flags 1 statistics, 2 fused InstanceNorm-backward sums, 4 fused activation backward
FORMS = [(0, 0), (0, 1), (1, 0), (1, 2), (1, 4), (2, 0), (3, 0), (4, 0), (4, 1)]
OPTIONS = [("gconv_bm", v, 0) for v in (128, 192, 256, 258, 512)] + [("gconv_halo", 0, 1), ("tile128x192", 0, 1), ("cls_skip", 0, 1)]
LIBS = ("bf16", "f16")
MAX_LAUNCHES = 8

# Layers the corpus of test_conv_queries.py lacks, (N, layer): without them no case reaches the 256 x 192 HALO tile (the
# 768-channel trunk from N = 27) or the 128 x 192 tile (the two-scale generator's 1536-channel trunk at 16 x 8; its input
# gradient form with fused sums) -- the layers tests/_exact.py reaches those tiles with --, and no fp8-eligible layer is narrow
# enough for the 128 x 32 tile (the last one: 128 -> 24 channels)
EXTRA = [(27, (768, 32, 16, 768, 3, 3, 1, 1, 1, 0, 0)), (32, (192, 16, 8, 1536, 3, 3, 1, 1, 1, 0, 0)),
         (32, (1152, 16, 8, 64, 3, 3, 1, 1, 0, 0, 0)), (2, (128, 16, 16, 24, 3, 3, 1, 1, 1, 0, 0))]

# the dispatch tables of csrc/gconv.hip (kTilesF32 / kTilesFp8 / kTiles16): (bm, bn, mr, nr, nstage, halo)
EVERY_TYPE = [(128, 128, 2, 2, 2, 0), (128, 64, 2, 1, 2, 0), (128, 32, 1, 1, 2, 0),
              (256, 128, 2, 2, 3, 0), (256, 128, 2, 2, 2, 0), (256, 64, 2, 1, 3, 0), (256, 64, 2, 1, 2, 0)]
TABLE = {"f32": EVERY_TYPE,
         "fp8": EVERY_TYPE + [(256, 192, 2, 3, 2, 0)],
         "h16": EVERY_TYPE + [(256, 192, 2, 3, 2, 0), (256, 256, 4, 2, 2, 0), (256, 192, 2, 3, 2, 1), (256, 128, 2, 2, 2, 1),
                              (128, 192, 2, 3, 2, 0)]}


def cases():
    return Q.cases() + [(n,) + layer + (dt,) for n, layer in EXTRA for dt in (0, 1)]


def query(L, desc, form, flags):
    """Negative error code, or the list of 9-int launch records."""
    import ctypes as C
    buf = (C.c_int32 * (9 * MAX_LAUNCHES))()
    n = L.p2phd_conv_gconv_tiles(C.byref(desc), form, flags, buf, MAX_LAUNCHES)
    assert n <= MAX_LAUNCHES, n
    return n if n < 0 else [list(buf[9 * i:9 * i + 9]) for i in range(n)]


def answers(L, _lib):
    """[(case, w_layout, [answer per FORMS entry])]"""
    import ctypes as C
    out = []
    for case in cases():
        kmaj = L.p2phd_conv_kmajor_ok(C.byref(Q._desc(_lib, case, 0)))
        for wl in ((0, 1) if kmaj else (0,)):
            d = Q._desc(_lib, case, wl)
            out.append((case, wl, [query(L, d, form, flags) for form, flags in FORMS]))
    return out


def runs():
    """{run name: answers}, "bf16:default" first."""
    from pix2pixhdaudiosr_amd import _lib
    out = {}
    for kind in LIBS:
        L = _lib.lib(kind)
        out[f"{kind}:default"] = answers(L, _lib)
        for name, value, default in OPTIONS:
            assert L.p2phd_set_option(name.encode(), value) == 0, name
            try:
                out[f"{kind}:{name}={value}"] = answers(L, _lib)
            finally:
                assert L.p2phd_set_option(name.encode(), default) == 0, name
    return out


_RUNS = []


def all_runs():
    if not _RUNS:
        _RUNS.append(runs())
    return _RUNS[0]


def encode(all_):
    tiles, rows = [], []

    def intern(table, item):
        if item not in table:
            table.append(item)
        return table.index(item)

    def row_index(ans):
        return intern(rows, [a if isinstance(a, int) else [intern(tiles, t) for t in a] for a in ans])

    base = [row_index(ans) for _, _, ans in all_["bf16:default"]]
    diffs = {}
    for key, got in all_.items():
        if key == "bf16:default":
            continue
        assert len(got) == len(base), key
        idx = [row_index(ans) for _, _, ans in got]
        diffs[key] = {str(i): r for i, r in enumerate(idx) if r != base[i]}
    return {"cases": len(cases()), "tiles": tiles, "rows": rows, "base": base, "diffs": diffs}


def decode(fix, key):
    """The answers of one run, as query() returns them."""
    idx = list(fix["base"])
    if key != "bf16:default":
        for i, r in fix["diffs"][key].items():
            idx[int(i)] = r
    return [[a if isinstance(a, int) else [fix["tiles"][t] for t in a] for a in fix["rows"][r]] for r in idx]


def test_tile_query_matches_the_recorded_answers():
    want = json.load(open(FIXTURE))
    got = all_runs()
    assert want["cases"] == len(cases())
    assert sorted(got) == sorted(["bf16:default"] + list(want["diffs"]))
    for key, rows in got.items():
        exp = decode(want, key)
        assert len(rows) == len(exp), key
        bad = [(case, wl, FORMS[j], a, e[j]) for (case, wl, ans), e in zip(rows, exp) for j, a in enumerate(ans) if a != e[j]]
        assert not bad, (key, len(bad), bad[:5])


def _launches():
    """(run, case, w_layout, form, flags, launch record) of every launch any run reports."""
    for key, rows in all_runs().items():
        for case, wl, ans in rows:
            for (form, flags), a in zip(FORMS, ans):
                if not isinstance(a, int):
                    for t in a:
                        yield key, case, wl, form, flags, t


def _type_of(case, form):
    return "fp8" if form == 4 else ("h16" if case[-1] == 1 else "f32")


def test_every_tile_is_in_the_dispatch_table_of_its_type():
    seen = 0
    for key, case, wl, form, flags, t in _launches():
        assert tuple(t[:6]) in TABLE[_type_of(case, form)], (key, case, form, flags, t)
        assert t[6] in (0, 1) and t[7] in (0, 1), (key, case, form, flags, t)
        seen += 1
    assert seen > 10000, seen


def test_table_sizes_rely_on_these_bounds():
    """stat_table_floats sizes the statistics table for slots of >= 32 rows, bsum_table_floats the partial table of the fused
    sums for tiles of >= 128 rows (csrc/convplan.h)."""
    for key, case, wl, form, flags, t in _launches():
        assert t[8] >= 32, (key, case, form, flags, t)
        if flags & 2:
            assert t[0] >= 128 and t[8] == t[0], (key, case, form, flags, t)
        else:
            assert t[8] == 32 * t[2], (key, case, form, flags, t)


def test_corpus_reaches_every_row_of_the_dispatch_tables():
    """A corpus that misses a tile pins nothing about it (counted over all runs: the 2-slot ring of the 256-row tiles is what
    gconv_bm = 258 asks for -- the heuristic takes the 3-slot ring wherever it fits, and it fits every layer here)."""
    reached = {k: set() for k in TABLE}
    for key, case, wl, form, flags, t in _launches():
        reached[_type_of(case, form)].add(tuple(t[:6]))
    for k, table in TABLE.items():
        assert reached[k] == set(table), (k, sorted(set(table) - reached[k]))


def test_the_query_refuses_what_does_not_apply():
    import ctypes as C
    from pix2pixhdaudiosr_amd import _lib
    L = _lib.lib()
    trunk = Q._desc(_lib, (8, 768, 32, 16, 768, 3, 3, 1, 1, 1, 0, 0, 1), 0)
    plain = Q._desc(_lib, (8, 64, 32, 16, 64, 4, 4, 2, 2, 0, 0, 0, 1), 0)
    assert query(L, trunk, 2, 0) and query(L, trunk, 3, 0) and query(L, trunk, 4, 1)
    assert query(L, plain, 2, 0) < 0 and query(L, plain, 3, 0) < 0 and query(L, plain, 4, 0) < 0      # no reflect grid, stride 2
    assert query(L, trunk, 1, 2) < 0                                    # fused sums: not behind a reflection pad
    assert query(L, plain, 1, 6) < 0 and query(L, plain, 1, 1) < 0 and query(L, plain, 0, 2) < 0 and query(L, plain, 5, 0) < 0
    assert L.p2phd_conv_gconv_tiles(C.byref(plain), 0, 0, None, 0) == 1  # count only


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    with open(FIXTURE, "w") as f:
        json.dump(encode(all_runs()), f, separators=(",", ":"))
    print(f"wrote {FIXTURE}: {os.path.getsize(FIXTURE)} bytes")
