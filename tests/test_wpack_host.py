"""CPU checks of tests/_wpack.py: the index coding finds every element of a plain pack and rejects broken ones, the rounding
vectors hold every class they promise (judged by torch's CPU cast), the e4m3 encoder is torch.float8_e4m3fn's."""
import numpy as np
import pytest
import torch

import _wpack as P

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


def _packs(rows, inner, R, S, rows_pad, Cp, KK, dtype):
    n = rows * inner * R * S
    return n, [torch.from_numpy(P.plain_pack(d.reshape(rows, inner, R, S), rows_pad, Cp, KK)).to(dtype) for d in P.index_digits(n)]


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("geom", [(5, 3, 3, 3, 128, 8, 128), (130, 72, 1, 1, 256, 72, 128), (70, 16, 4, 4, 128, 16, 256),
                                  (300, 250, 1, 1, 384, 256, 256)], ids=lambda g: "x".join(map(str, g)))
def test_decode_finds_every_element_of_a_plain_pack(geom, dt):
    rows, inner, R, S, rows_pad, Cp, KK = geom
    n, packs = _packs(*geom, DT[dt])
    src = P.decode([p.float().numpy() for p in packs], n)
    assert src.shape == (rows_pad, KK)
    assert P.multiplicity(src, n) == 1
    # and where: element (row, c, r, s) at [row][(r S + s) Cp + c]
    want = np.full((rows_pad, KK), -1, dtype=np.int64)
    idx = np.arange(n).reshape(rows, inner, R * S)
    for t in range(R * S):
        want[:rows, t * Cp:t * Cp + inner] = idx[:, :, t]
    assert np.array_equal(src, want)
    assert int((src < 0).sum()) == rows_pad * KK - n


def test_index_digits_reach_past_two_bytes():
    n = 70000
    d = P.index_digits(n)
    assert all(a.dtype == np.float32 and a.min() >= 0 and a.max() <= 255 for a in d) and d[2].max() == 1
    assert np.array_equal(P.decode(d, n), np.arange(n))
    with pytest.raises(AssertionError):
        P.index_digits(2 ** 24)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("kind", ["duplicated", "dropped", "sum", "blend", "stale_nan", "foreign_index"])
def test_broken_packs_are_rejected(kind, dt):
    n, packs = _packs(5, 3, 3, 3, 128, 8, 128, DT[dt])
    a = [p.float().numpy().copy() for p in packs]
    row, k1, k2 = 2, 1 * 8 + 1, 4 * 8 + 2                                  # two valid elements of one row; [2][3] is a pad channel
    if kind == "duplicated":                                               # one element twice (the second copy in a pad channel)
        for p in a: p[row, 3] = p[row, k1]
    elif kind == "dropped":
        for p in a: p[row, k1] = 0
    elif kind == "sum":                                                    # two elements added: a digit beyond 255, or a wrong element twice
        for p in a: p[row, k1] = p[row, k1] + p[row, k2]
    elif kind == "blend":
        for p in a: p[row, k1] = 0.5 * (p[row, k1] + p[row, k2]) + 0.25
    elif kind == "stale_nan":                                              # an unwritten 0xFF pattern
        a[1][100, 5] = np.nan
    else:
        a[2][row, k1] = 200.0                                              # decodes far beyond n
    with pytest.raises(ValueError):
        P.multiplicity(P.decode(a, n), n)


# ----------------------------------------------------------------------------------------------------------------------
# rounding vectors
# ----------------------------------------------------------------------------------------------------------------------
def _cast(v, dtype):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dtype)


def _representable(v64, dtype):
    t = torch.from_numpy(np.ascontiguousarray(v64))
    return torch.equal(t.to(dtype).double(), t)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_class_of_the_rounding_vectors_is_present(dt):
    dtype = DT[dt]
    V = P.rounding_vectors(dtype)
    assert set(V) == set(P.CLASSES)
    fi = torch.finfo(dtype)
    for k, v in V.items():
        assert v.dtype == np.float32 and v.size > 0 and np.isfinite(v).all(), k
        if k != "ordinary":
            assert (v > 0).any() and (v < 0).any() or k == "zero", k
    bits = lambda c: c.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    for k, up in (("tie_even_below", False), ("tie_even_above", True)):
        x = V[k].astype(np.float64)
        c = _cast(V[k], dtype)
        c64 = c.double().numpy()
        assert np.isfinite(c64).all() and (np.abs(c64) >= fi.smallest_normal).all(), k
        other = 2 * x - c64                                                 # a tie: the other neighbour is as far away
        assert (other != c64).all() and _representable(other, dtype), k
        assert ((np.abs(c64) > np.abs(x)) == up).all(), k                   # where the even neighbour lies
        assert (bits(c) & 1 == 0).all(), k                                  # ... and that it is the even one
        # nothing representable lies between the two: they are adjacent codes
        assert (np.abs(bits(c) - bits(_cast(other.astype(np.float32), dtype))) == 1).all(), k
    ties = np.concatenate([V["tie_even_below"], V["tie_even_above"]])
    tb = ties.view(np.uint32)
    for k, step in (("tie_minus_ulp", -1), ("tie_plus_ulp", 1)):
        assert np.array_equal(np.sort(V[k].view(np.uint32)), np.sort((tb.astype(np.int64) + step).astype(np.uint32))), k
        # one f32 ulp off the tie decides the direction: towards zero below it, away from zero above it
        c = np.abs(_cast(V[k], dtype).double().numpy())
        assert ((c > np.abs(V[k].astype(np.float64))) == (step > 0)).all(), k
    assert (np.abs(_cast(V["max_finite"], dtype).double().numpy()) == fi.max).all() and float(np.abs(V["max_finite"]).min()) == fi.max
    assert torch.isinf(_cast(V["first_to_inf"], dtype)).all()
    lim = np.nextafter(np.abs(V["first_to_inf"]).min(), np.float32(0))     # the f32 just below the first that overflows ...
    assert lim in np.abs(V["max_finite"])                                   # ... is the largest that does not
    s = np.abs(_cast(V["subnormal"], dtype).double().numpy())
    assert (np.abs(V["subnormal"].astype(np.float64)) < fi.smallest_normal).all()      # inputs below the normal range ...
    assert (s <= fi.smallest_normal).all() and (s == fi.smallest_normal).any()          # ... the largest ones round up into it
    assert (s == 0).any() and ((s > 0) & (s < fi.smallest_normal)).any() and (s == fi.smallest_normal * fi.eps).any()   # (eps: one unit of the last place)
    sx = np.abs(V["subnormal"].astype(np.float64))
    assert ((s != sx).sum() > 10) and (s > sx).any() and (s < sx).any()     # results rounded both ways
    z = V["zero"].view(np.uint32)
    assert sorted(z.tolist()) == [0, 0x80000000]
    o = V["ordinary"]
    assert 0.01 < float(o.std()) < 0.04 and float(np.abs(o).max()) < 0.2


@pytest.mark.parametrize("dt", list(DT))
def test_rounding_tensor_holds_every_vector(dt):
    dtype = DT[dt]
    shape = (6, 5, 7, 7) if dt != "f32" else (13, 5, 3, 3)
    t = P.rounding_tensor(dtype, shape, seed=3)
    assert t.dtype == torch.float32 and tuple(t.shape) == shape and bool(torch.isfinite(t).all())
    have = set(t.reshape(-1).numpy().view(np.uint32).tolist())
    for kind in ([torch.bfloat16, torch.float16] if dt == "f32" else [dtype]):
        for k, v in P.rounding_vectors(kind).items():
            if k != "ordinary":
                assert set(v.view(np.uint32).tolist()) <= have, (kind, k)
    assert torch.equal(t, P.rounding_tensor(dtype, shape, seed=3))
    with pytest.raises(AssertionError):
        P.rounding_tensor(dtype, (4, 4, 3, 3))


# ----------------------------------------------------------------------------------------------------------------------
# e4m3
# ----------------------------------------------------------------------------------------------------------------------
def test_e4m3_encoder_equals_torch_on_codes_midpoints_and_their_neighbours():
    codes = np.arange(256, dtype=np.uint8)
    vals = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    fin = np.isfinite(vals)
    assert fin.sum() == 254 and float(np.abs(vals[fin]).max()) == 448.0
    assert np.array_equal(P.e4m3_encode(vals[fin]), codes[fin])             # every code is its own encoding (+-0 included)
    assert np.array_equal(P.e4m3_decode(codes)[fin].view(np.uint32), vals[fin].view(np.uint32))
    pos = np.sort(vals[fin & (codes < 0x80)])                               # 0 .. 448 ascending
    mid = ((pos[:-1].astype(np.float64) + pos[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1].astype(np.float64) + pos[1:]) / 2)
    mb = mid.view(np.uint32)
    x = np.concatenate([mid, (mb - 1).view(np.float32), (mb + 1).view(np.float32), np.nextafter(pos[1:], np.float32(0)),
                        np.nextafter(pos, np.float32(np.inf))[:-1]])
    x = np.concatenate([x, -x])
    assert float(np.abs(x).max()) <= 448.0
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = P.e4m3_encode(x)
    assert np.array_equal(got, want), [(float(a), int(b), int(c)) for a, b, c in zip(x[got != want][:8], got[got != want], want[got != want])]
    # ties go to the even code, both ways
    tie = P.e4m3_encode(mid)
    assert (tie & 1 == 0).all() and (P.e4m3_decode(tie) > mid).any() and (P.e4m3_decode(tie) < mid).any()


def test_e4m3_encoder_saturates():
    x = np.array([448.0, 449.0, 463.9, 464.0, 480.0, 1e6, 3e38, -464.0, -1e9], dtype=np.float32)
    assert P.e4m3_encode(x).tolist() == [0x7E] * 7 + [0xFE] * 2
    r = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 100
    got = P.e4m3_encode(r)
    want = torch.from_numpy(np.clip(r, -448, 448)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(got, want)
