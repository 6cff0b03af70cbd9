"""The packed weight buffers themselves: p2phd_conv_pack_weights / p2phd_conv_fp8_pack_weights straight through the C ABI, into
guarded buffers of exactly the reported size, per storage type and library.

Per case (tests/_wpack.py has the helpers):
  a. the guards are intact after every pack;
  b. the same weights packed into a 0x00- and a 0xFF-prefilled buffer differ exactly in the never-written bytes U (printed; the
     launches that read the pack run on a 0xFF pack in tests/test_gpu_conv_exact.py and in test_new_layers_run_on_a_poisoned_pack);
  c. packing w1 and then w2 into one buffer leaves what packing w2 into a fresh buffer leaves, byte for byte outside U;
  d. (layers without a fragment copy) three index-coded packs decode to a map packed element -> master element or padding in
     which every master element occurs equally often (printed; the kernels' ownership rule says once), and where the header's
     plain [rows_pad][tap][Cp] layout applies (no W-fold, not merged) the map is that layout's;
  e. (the same layers) the rounding vectors land, through that map, as torch's CPU cast of them, bit for bit, padding as +0;
and the launch counters say which pack kernel ran -- every case names the one it is there for.

Which kernel a layer takes follows from the predicates of csrc/wpack.hip (launch_pack) and the planner (csrc/convapi.hip make_plans):
  dense        all taps (<= 16) of a [rows][inner][R][S] master tensor: forward of a Conv2d, input gradient of a ConvTranspose2d
  transposed   [inner][rows][R][S]: input gradient of a stride-1 Conv2d (PyTorch layout)
  walk         > 16 taps, or a W-folded index (row_mod / c_mod split): 7x7 layers, layers with <= 4 channels on one side
  kmajor / _t  w_layout = 1: forward cast / input-gradient transpose per tap
  merged       every stride-2 input gradient of a Conv2d and forward of a ConvTranspose2d (merged_plan never refuses stride 2,
               so the per-class plans with strided tap subsets, wr_step / ws_step = 2, are not reachable through the ABI)
  frag         the 16-bit layers of the dedicated kernels (march, dlast, dfirst, c7 in / out / dgrad); in f32 they have none."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import _exact as X
import _wpack as P
import test_gpu_conv_exact as E

pytestmark = pytest.mark.gpu

DT = E.DT
WPACK_FAMILIES = ("wpack_generic", "wpack_dense", "wpack_transposed", "wpack_kmajor", "wpack_kmajor_t", "wpack_merged", "wpack_fp8",
                  "wpack_frag")

# name, layer, which, w_layout, kernel = the wpack.hip kernel of the generic pack, frag = a fragment copy follows in the 16-bit
# types, skip = the cls_skip option for the pack (None: default), offset = master tensor at a 4-byte offset from 16-byte alignment
Case = collections.namedtuple("Case", "name layer which layout kernel frag skip offset")
_G = {l.name: l for l in X.GENERIC + X.WPACK + X.WGRAD_KMAJOR + X.HALO_FWD}


def _c(layer, which, kernel, layout=0, frag=False, skip=None, offset=False, tag=""):
    l = _G[layer] if isinstance(layer, str) else layer
    name = f"{l.name}:{'dgrad' if which else 'fwd'}" + (":kmajor" if layout else "") + tag
    return Case(name, l, which, layout, "wpack_" + kernel, frag, skip, offset)


CASES = [
    # dense: inner 72 (second 64-column block holds 8), rows 6; C = 2 (Cp = 8 > inner), rows 37; 16 taps; 4 taps with a K tail; 9 taps
    _c("wp_c72_k6", 0, "dense"), _c("wp_c2_k37_s2", 0, "dense"), _c("c4_s1", 0, "dense"), _c("wp_c24_k7_2x2", 0, "dense"),
    _c("wp_c24_k72", 0, "dense"), _c("tile_72to384", 0, "dense"), _c("trunk_768", 0, "dense"),
    # transposed: rows 72 / 24 (a half-filled last brick, then bricks of pure padding rows up to rows_pad = 128: run == 0),
    # inner 6 / 72 (not a multiple of 64), 9 / 16 / 4 taps
    _c("wp_c72_k6", 1, "transposed"), _c("wp_c24_k72", 1, "transposed"), _c("c4_s1", 1, "transposed"), _c("wp_c24_k7_2x2", 1, "transposed"),
    _c("c3_reflect_6x5", 1, "transposed"),
    # the tap walk: 49 taps (three full batches of 16 and one tap); the W-folded maps (row_mod / c_mod < rows / inner)
    _c("wp_c5_k6_7x7", 0, "generic"), _c("wp_c5_k6_7x7", 1, "generic"), _c("kfold_k3", 0, "generic"), _c("kfold_k3", 1, "generic"),
    _c("cfold_c3", 0, "generic"), _c("cfold_c3", 1, "generic"),                # (25 taps of an [inner][rows] tensor: too many for the transposed kernel)
    # K-major master weights: the cast; the transpose from an aligned tensor (`whole` tiles where a tile is whole) and from a
    # 4-byte-offset view (scalar path everywhere); K = 72 / rows_pad = 128 > C = 64: tiles hanging over Cp and rows_pad
    _c("wp_kmajor_c64_k72", 0, "kmajor", 1), _c("wp_kmajor_c64_k72", 1, "kmajor_t", 1), _c("wp_kmajor_c64_k72", 1, "kmajor_t", 1, offset=True, tag=":offset"),
    _c("kmajor_128to64_k4", 0, "kmajor", 1), _c("kmajor_128to64_k4", 1, "kmajor_t", 1), _c("kmajor_128to64_k4", 1, "kmajor_t", 1, offset=True, tag=":offset"),
    _c("trunk_768", 1, "kmajor_t", 1),
    # merged sub-pixel: Conv2d stride 2 input gradient (3x3, 4x4, C = 2 -> rows 4 * 8), ConvTranspose2d forward; both tap orders
    _c("c3_s2_odd", 1, "merged"), _c("c4_s2", 1, "merged"), _c("wp_c2_k37_s2", 1, "merged"), _c("ct3_s2", 0, "merged"),
    _c(X.CLS_SKIP_DGRAD[0], 1, "merged", skip=1, tag=":skip"), _c(X.CLS_SKIP_DGRAD[0], 1, "merged", skip=0, tag=":noskip"),
    _c(X.CLS_SKIP_FWD[0], 0, "merged", skip=1, tag=":skip"), _c(X.CLS_SKIP_FWD[0], 0, "merged", skip=0, tag=":noskip"),
    # the ConvTranspose2d input gradient is a direct plan on [C][K][R][S]: dense
    _c("ct3_s2", 1, "dense"),
    # fragment packs behind the generic pack (16-bit types)
    _c(X.MARCH_CONV[0], 0, "dense", frag=True), _c(X.MARCH_CONV[0], 1, "merged", frag=True),
    _c(X.MARCH_CONVT[0], 0, "merged", frag=True), _c(X.MARCH_CONVT[0], 1, "dense", frag=True),
    _c(X.DLAST[1], 0, "generic", frag=True), _c(X.DLAST[1], 1, "generic", frag=True),
    _c(X.DFIRST[3], 0, "dense", frag=True),
    _c(X.C7_IN[2], 0, "generic", frag=True), _c(X.C7_OUT[2], 0, "generic", frag=True), _c(X.C7_OUT[2], 1, "generic", frag=True),
]


def test_table_reaches_every_pack_kernel():
    """Every case asserts the counter it names; together with the e4m3 test they name every family."""
    named = {c.kernel for c in CASES} | {"wpack_frag" for c in CASES if c.frag} | {"wpack_fp8"}
    assert named == set(WPACK_FAMILIES)
    assert len({c.name for c in CASES}) == len(CASES)
    assert max(int(np.prod(X.w_shape(c.layer))) for c in CASES) == 768 * 768 * 9 <= P.MAX_ELEMS


def _counts(Lb):
    return {f: int(Lb.p2phd_launch_count(f.encode(), 0)) for f in WPACK_FAMILIES}


def _master(flat, offset):
    """Device copy of the flat float32 master tensor: 16-byte aligned, or 4 bytes behind an aligned address."""
    flat = torch.as_tensor(flat, dtype=torch.float32).reshape(-1)
    buf = torch.empty(flat.numel() + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    w = buf[1:1 + flat.numel()] if offset else buf[:flat.numel()]
    w.copy_(flat)
    assert w.data_ptr() % 16 == (4 if offset else 0)
    return w


def _host(g):
    """The payload bytes of a guarded buffer on the host."""
    return g.bytes.cpu().numpy()


def _values(g, dtype):
    """... and as float32 values of the storage type (exact: every 16-bit value is an f32 value)."""
    return g.bytes.cpu().view(dtype).float().numpy()


def _plain_src(l, which, layout):
    """Where the header's plain layout applies -- one direct or stride-1 transposed-form plan over all taps in order, no W-fold:
    rows x inner = K x C forward, C x K for an input gradient -- the master (memory) index of every element of the
    [round_up(rows, 128)][tap][cpitch(inner)] pack with its K extent padded to a multiple of 64, -1 = padding.  Else None."""
    folded = not l.transposed and l.stride == 1 and (l.cout <= 4 or (l.cin <= 4 and which == 0))
    merged = l.stride == 2 and (l.transposed == (which == 0))
    if folded or merged:
        return None
    d0, d1, R, S = X.w_shape(l)
    idx = np.arange(1, d0 * d1 * R * S + 1, dtype=np.int64)
    idx = idx.reshape(d0, R, S, d1).transpose(0, 3, 1, 2) if layout else idx.reshape(d0, d1, R, S)
    if which == 1 and not l.transposed:
        idx = idx.transpose(1, 0, 2, 3)                                     # rows = input channels
    rows, inner = idx.shape[:2]
    Cp = X.cpitch(inner)
    return P.plain_pack(np.ascontiguousarray(idx), (rows + 127) // 128 * 128, Cp, max(64, (R * S * Cp + 63) // 64 * 64)) - 1


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_pack(case, dt):
    dtype = DT[dt]
    l = case.layer
    ops, Lb, spec = E._setup(l, dtype)
    d = spec.desc(*l.shape, dtype, case.layout)
    if case.layout:
        assert Lb.p2phd_conv_kmajor_ok(C.byref(d)) == 1
    n = int(np.prod(X.w_shape(l)))
    esize = 4 if dt == "f32" else 2
    frag = case.frag and dt != "f32"
    what = f"{case.name} {dt}"
    opts = {} if case.skip is None else {"cls_skip": case.skip}
    with E.options(Lb, **opts):
        layout_id = Lb.p2phd_conv_pack_layout(C.byref(d), case.which)
        assert layout_id == (1 if case.skip == 1 and dt != "f32" else 0), (what, layout_id)   # the tap-skipping order: 16-bit types only

        def pack(flat, fill, into=None):
            w = _master(flat, case.offset)
            g = P.pack_guarded(ops, Lb, d, case.which, w, fill, into)
            X.check_guards({"packed": g}, what)                                                  # a.
            return g

        w1 = P.rounding_tensor(dtype, (n,), seed=1)
        w2 = P.rounding_tensor(dtype, (n,), seed=2)
        Lb.p2phd_launch_count(None, 1)
        g00 = pack(w2, 0x00)
        cnt = _counts(Lb)
        want_cnt = dict.fromkeys(WPACK_FAMILIES, 0)
        want_cnt[case.kernel] = 1
        want_cnt["wpack_frag"] = 1 if frag else 0
        assert cnt == want_cnt, (what, cnt)
        gff = pack(w2, 0xFF)
        b00, bff = _host(g00), _host(gff)
        U = b00 != bff                                                                           # b. never written
        assert ((b00[U] == 0x00) & (bff[U] == 0xFF)).all(), what
        nU = int(U.sum())
        g12 = pack(w1, 0xFF)
        assert not np.array_equal(_host(g12)[~U], b00[~U]), what                                 # (w1 and w2 do differ in the pack)
        pack(w2, None, into=g12)                                                                 # c.
        bad = (_host(g12) != b00) & ~U
        assert not bad.any(), f"{what}: repack differs from a fresh pack in {int(bad.sum())} bytes outside U (len(U) = {nU}), first at {np.flatnonzero(bad)[:8].tolist()}"
        if frag:
            print(f"\nWPACK {what}: kernel={case.kernel}+wpack_frag layout_id={layout_id} bytes={g00.nbytes} len(U)={nU} multiplicity=n/a (fragment copy)")
            return
        # d. the map, from three index-coded packs into poisoned buffers
        Ue = U.reshape(-1, esize).any(axis=1)
        passes = []
        for digit in P.index_digits(n):
            passes.append(np.where(Ue, 0.0, _values(pack(digit, 0xFF), dtype)))
        try:
            src = P.decode(passes, n)
            mult = P.multiplicity(src, n)
        except ValueError as e:
            raise AssertionError(f"{what}: {e} (len(U) = {nU})")
        print(f"\nWPACK {what}: kernel={case.kernel} layout_id={layout_id} bytes={g00.nbytes} len(U)={nU} multiplicity={mult}")
        assert mult == 1, f"{what}: every master element occurs {mult} times, the ownership rule says once (len(U) = {nU})"
        plain = _plain_src(l, case.which, case.layout)
        if plain is not None:
            assert plain.size == src.size and np.array_equal(src, plain.reshape(-1)), f"{what}: not the plain [rows_pad][tap][Cp] layout (len(U) = {nU})"
        # e. rounding, through the map; padding is +0
        ref = torch.cat([w2, torch.zeros(1)])[torch.from_numpy(np.where(src >= 0, src, n))].to(dtype)
        bits = {2: torch.int16, 4: torch.int32}[esize]
        got = gff.bytes.cpu().view(bits)
        diff = (got != ref.view(bits)) & torch.from_numpy(~Ue)
        if bool(diff.any()):
            at = diff.nonzero().flatten()[:8]
            s = src[at.numpy()]
            raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} packed elements differ from cast(w[src]) in their bits (len(U) = {nU}); first "
                                 f"(offset, src, w, got bits, want bits): "
                                 f"{[(int(a), int(i), float(w2[i]) if i >= 0 else 0.0, hex(int(got[a]) & 0xFFFFFFFF), hex(int(ref.view(bits)[a]) & 0xFFFFFFFF)) for a, i in zip(at, s)]}")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("l", X.WPACK, ids=lambda l: l.name)
def test_new_layers_run_on_a_poisoned_pack(l, dt):
    """The layers this module adds to the tables of tests/_exact.py: forward and input gradient on the integer operands, the pack
    made by the C entry into 0xFF memory (run_fwd / run_dgrad of the exact tests) -- no launch reads a byte of U."""
    Lb = E._ops().lib_for(DT[dt])
    kmajor = l.name.startswith("wp_kmajor")
    for layout in ((0, 1) if kmajor else (0,)):
        assert E.run_fwd(l, dt, E.NONE, False, layout=layout)["gconv"] >= 1
        assert E.run_dgrad(l, dt, False, layout=layout)["gconv"] >= 1
        if l.pad_mode:
            with E.options(Lb, reflect_generic=1):
                assert E.run_dgrad(l, dt, False, layout=layout)["gconv"] >= 1


# ----------------------------------------------------------------------------------------------------------------------
# e4m3
# ----------------------------------------------------------------------------------------------------------------------
# 1x1 with 128 channels is the smallest eligible reduction (C % 16 == 0, R S C % 128 == 0); K <= 4 is a W-fold layer and not
# eligible (fp8_eligible: fold_mode == FOLD_NONE), so the smallest K is 5; K = 130: two row blocks of 128, 126 padding rows
FP8_LAYERS = [(X.L("q_1x1_c128_k5", 128, 5, 1, 1, 0, 0, 0, 0, (1, 4, 4)), 0), (X.L("q_1x1_c128_k130", 128, 130, 1, 1, 0, 0, 0, 0, (1, 4, 4)), 0),
              (X.L("q_3x3_c128_k64", 128, 64, 3, 1, 1, 1, 0, 0, (1, 4, 4)), 0), (X.L("q_3x3_c128_k64", 128, 64, 3, 1, 1, 1, 0, 0, (1, 4, 4)), 1)]


@pytest.mark.parametrize("l,layout", FP8_LAYERS, ids=[f"{l.name}{':kmajor' if k else ''}" for l, k in FP8_LAYERS])
def test_e4m3_pack(l, layout):
    """p2phd_conv_fp8_pack_weights: tail = (amax / 448.f, 448.f / amax, amax bits) as numpy float32 arithmetic gives them, every
    byte = e4m3(float32(w * inv)) at the position of the plain [round_up(K, 128)][tap][C] layout, padding rows 0x00.  The map is
    the numpy restatement of that layout; the bf16 pack of the same plan (same rows_pad, Cp = C, KK = R S C), decoded from index
    coding, must agree with it."""
    dtype = torch.bfloat16
    ops, Lb, spec = E._setup(l, dtype)
    d = spec.desc(*l.shape, dtype, layout)
    assert Lb.p2phd_conv_fp8_eligible(C.byref(d)) == 1
    tiny = E._setup(l._replace(cout=1), dtype)[2].desc(*l.shape, dtype)
    assert Lb.p2phd_conv_fp8_eligible(C.byref(tiny)) == 0 and Lb.p2phd_conv_fp8_packed_bytes(C.byref(tiny)) == 0
    K, Cc, R, S = X.w_shape(l)
    n = K * Cc * R * S
    rows_pad = (K + 127) // 128 * 128
    nw = rows_pad * R * S * Cc
    assert Lb.p2phd_conv_fp8_packed_bytes(C.byref(d)) == nw + 256
    src = _plain_src(l, 0, layout).reshape(-1)
    passes = [_values(P.pack_guarded(ops, Lb, d, 0, _master(dg, False)), dtype) for dg in P.index_digits(n)]
    assert passes[0].size == nw and np.array_equal(P.decode(passes, n), src), "bf16 pack of the same plan"
    gen = np.random.default_rng(K * 31 + R + layout)
    base = (0.02 * gen.standard_normal(n)).astype(np.float32)
    big = np.float32(1.37) * np.abs(base).max()
    last4 = (n // 4 - 1) * 4 + 1                                            # inside the last float4: every lane's clamped loads read it
    for pos, sign in ((0, 1), (n - 1, 1), (n // 3, -1), (last4, -1), (last4 + 1, 1)):
        w = base.copy()
        w[pos] = sign * big
        what = f"fp8 {l.name} layout={layout} amax at {pos} sign {sign}"
        Lb.p2phd_launch_count(None, 1)
        g = P.pack_guarded_fp8(ops, Lb, d, _master(w, False), 0xFF)
        cnt = _counts(Lb)
        assert cnt == dict(dict.fromkeys(WPACK_FAMILIES, 0), wpack_fp8=1), (what, cnt)
        g2 = P.pack_guarded_fp8(ops, Lb, d, _master(w, False), 0x00)
        X.check_guards({"packed8": g, "second": g2}, what)
        b, b2 = _host(g), _host(g2)
        U = b != b2
        assert not U[:nw].any() and not U[nw:nw + 8].any() and not U[nw + 16:nw + 20].any(), (what, "two packs differ", int(U.sum()))
        amax = np.float32(big)
        tail = b[nw:nw + 20]
        assert tail[16:20].view(np.uint32)[0] == amax.view(np.uint32), (what, "amax bits")
        scale, inv = np.float32(amax) / np.float32(448.0), np.float32(448.0) / np.float32(amax)
        assert tail[0:8].view(np.uint32).tolist() == [scale.view(np.uint32), inv.view(np.uint32)], (what, tail[0:8].view(np.float32), scale, inv)
        q = np.concatenate([(w * inv).astype(np.float32), np.zeros(1, np.float32)])
        want = P.e4m3_encode(q[np.where(src >= 0, src, n)])
        bad = b[:nw] != want
        assert not bad.any(), (what, int(bad.sum()), [(int(i), int(src[i]), float(q[src[i]]), hex(b[i]), hex(want[i])) for i in np.flatnonzero(bad)[:8]])
        assert (b[:nw][src < 0] == 0).all()
    print(f"\nWPACK fp8 {l.name} layout={layout}: kernel=wpack_fp8 bytes={g.nbytes} len(U)={int(U.sum())} (tail bytes 8..16 and 20..256)")
    # all-zero weights: all-zero bytes, scale = 1e-30f / 448.f; into a buffer that held another pack
    gz = P.pack_guarded_fp8(ops, Lb, d, _master(np.zeros(n, np.float32), False), None, into=g)
    X.check_guards({"packed8": gz}, "fp8 zeros")
    bz = _host(gz)
    assert not bz[:nw].any() and bz[nw + 16:nw + 20].view(np.uint32)[0] == 0
    s0, i0 = np.float32(1e-30) / np.float32(448.0), np.float32(448.0) / np.float32(1e-30)
    assert bz[nw:nw + 8].view(np.uint32).tolist() == [s0.view(np.uint32), i0.view(np.uint32)]
