"""CPU: the discrete-log reference of tests/distinct_cases.py (what the at-size GPU tests on all-distinct bases are checked against):
its dot product is exact, it notices a scalar that meets the base one tile further on -- which the fold-by-tile reference of
skew_cases.py cannot -- and it equals the CPU oracle's own MSM over bases the oracle made."""
import numpy as np
import pytest

import distinct_cases as dc
import pymodel as pm
import skew_cases as sk


def _python_sum(h, s):
    return sum(dc.row_int(a) * dc.row_int(b) for a, b in zip(h, s))


def test_weighted_sum256_is_exact():
    rng = np.random.default_rng(1)
    h = rng.integers(0, 1 << 64, size=(3000, 4), dtype=np.uint64)
    s = rng.integers(0, 1 << 64, size=(3000, 4), dtype=np.uint64)
    assert dc.weighted_sum256(h, s) == _python_sum(h, s)
    assert dc.weighted_sum256(h[:0], s[:0]) == 0
    # the exactness bound: a full block of all-ones words, every 16 x 16 entry at its maximum 2^20 (2^16 - 1)^2
    ones = np.full((dc.BLOCK, 4), np.uint64((1 << 64) - 1))
    assert dc.weighted_sum256(ones, ones) == dc.BLOCK * ((1 << 256) - 1) ** 2
    # a length that straddles a block boundary: the second block is short, and its rows differ from the first block's
    n = dc.BLOCK + 12345
    h = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    s = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    want = dc.weighted_sum256(h[:dc.BLOCK], s[:dc.BLOCK]) + _python_sum(h[dc.BLOCK:], s[dc.BLOCK:])
    assert dc.weighted_sum256(h, s) == want
    lo = dc.BLOCK - 2000
    assert dc.weighted_sum256(h[lo:], s[lo:]) == _python_sum(h[lo:], s[lo:])      # (from row 0 of a block: no block structure in the data)


def test_generators_are_seeded_and_shaped():
    for cid in range(4):
        r = dc.r_of(cid)
        n = (1 << 16) + 3
        h, planted = dc.make_logs(cid, n, 5)
        h2, _ = dc.make_logs(cid, n, 5)
        assert np.array_equal(h, h2) and h.shape == (n, 4) and h.dtype == np.uint64
        vals = [dc.row_int(row) for row in h[:2000]]
        assert all(v < r for v in vals) and len(set(vals)) == 2000
        assert dc.row_int(h[planted["zero"]]) == 0 and dc.row_int(h[planted["r"]]) == r and dc.row_int(h[planted["one"]]) == 1
        assert dc.planted_infinities(planted) == 2
        for label, d in (("2^12", 1 << 12), ("2^15", 1 << 15), ("half", n // 2)):
            i, j = planted["equal " + label]
            assert j - i == d and dc.row_int(h[i]) == dc.row_int(h[j])
            i, j = planted["opposite " + label]
            assert j - i == d and dc.row_int(h[i]) + dc.row_int(h[j]) == r
        assert sorted(dc.planted_rows(512)) == ["equal half", "one", "opposite half", "r", "zero"]
        u = dc.make_scalars(cid, 4096, 3, "uniform")
        assert np.array_equal(u, dc.make_scalars(cid, 4096, 3, "uniform")) and not np.array_equal(u, dc.make_scalars(cid, 4096, 4, "uniform"))
        assert all(dc.row_int(row) < r for row in u)
        a = dc.make_scalars(cid, 4096, 3, "any256")
        assert 0.4 < (a[:, 3] >> np.uint64(63)).mean() < 0.6                      # the top bit is in use
        hot = dc.make_scalars(cid, 4096, 3, "hot")
        values, counts = np.unique(dc.as_bytes(hot), axis=0, return_counts=True)
        assert 0.45 * 4096 < counts.max() < 0.55 * 4096 and len(values) > 0.4 * 4096
        assert all(dc.row_int(row) < r for row in hot)


@pytest.mark.parametrize("cid", [0, 1])
def test_a_base_one_tile_further_on_moves_this_reference_and_not_the_folded_one(cid):
    """An engine that gives entry i the base i + D and entry i + D the base i computes sum_k s_k h_pi(k), pi the exchange.  With distinct
    logs that differs from the expected sum.  With the bases every other at-size test uses -- a tile of D logs repeated -- it IS the
    expected sum, and the fold-by-tile reference (skew_cases.fold_scalars, then the sum over the tile) equals it: the blind spot."""
    r, D, n = dc.r_of(cid), 1 << 12, 1 << 14
    s = dc.make_scalars(cid, n, 9, "uniform")
    i = 777
    assert dc.row_int(s[i]) != dc.row_int(s[i + D])
    pi = np.arange(n)
    pi[i], pi[i + D] = i + D, i

    distinct, _ = dc.make_logs(cid, n, 2)
    want = dc.weighted_sum256(distinct, s) % r
    wrong = dc.weighted_sum256(distinct[pi], s) % r
    assert wrong != want
    assert (wrong - want) % r == (dc.row_int(s[i]) - dc.row_int(s[i + D])) * (dc.row_int(distinct[i + D]) - dc.row_int(distinct[i])) % r

    tile = distinct[:D]
    tiled = np.tile(tile, (n // D, 1))
    folded = sk.fold_scalars(cid, dc.as_bytes(s), D).view(np.uint64).reshape(D, 4)
    fold_reference = dc.weighted_sum256(tile, folded) % r
    assert dc.weighted_sum256(tiled, s) % r == fold_reference
    assert dc.weighted_sum256(tiled[pi], s) % r == fold_reference                  # the misdirected run passes the folded check


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_the_identity_holds_on_the_oracle(oracle, cid):
    """n = 512, bases h_i * G from the oracle's own one-pair multiplications (planted rows included): the oracle's MSM over them equals
    ((sum s_i h_i) mod r) * G.  "uniform" through the oracle's Pippenger; "any256" through its double-and-add MSM, which reads all 256
    bits of a scalar (the Pippenger reads the 253 / 255 bits of a canonical one, like the arkworks function it follows)."""
    curve = pm.CURVES[dc.NAMES[cid]]
    n = 512
    h, planted = dc.make_logs(cid, n, 40 + cid)
    assert set(planted) == {"zero", "r", "one", "equal half", "opposite half"}
    g = dc.generator_image(curve)
    images = dc.oracle_mul(oracle, curve, g, [dc.row_int(row) for row in h])
    bases = np.frombuffer(b"".join(dc.affine_of_projective(curve, p) for p in images), dtype=np.uint8).reshape(n, curve.affine_stride).copy()
    flag = 2 * curve.coord_bytes
    assert sorted(np.flatnonzero(bases[:, flag])) == sorted((planted["zero"], planted["r"]))
    assert bases[planted["one"]].tobytes() == g
    i, j = planted["equal half"]
    assert bases[i].tobytes() == bases[j].tobytes()
    i, j = planted["opposite half"]
    assert bases[j].tobytes() == sk.negate(cid, bases[i:i + 1])[0].tobytes()

    s = dc.make_scalars(cid, n, 50 + cid, "uniform")
    want = dc.expected(oracle, curve, h, s)
    assert sk.oracle_msm(oracle, cid, bases, dc.as_bytes(s)) == want
    assert want[2 * curve.coord_bytes:] != bytes(curve.coord_bytes)              # (not the point at infinity)

    s = dc.make_scalars(cid, n, 60 + cid, "any256")
    assert int((s[:, 3] >> np.uint64(63)).sum()) > 100
    want = dc.expected(oracle, curve, h, s)
    out = np.zeros(curve.projective_bytes, dtype=np.uint8)
    sb = np.ascontiguousarray(dc.as_bytes(s))
    assert oracle.oracle_msm_naive(cid, bases.ctypes.data, curve.affine_stride, sb.ctypes.data, n, out.ctypes.data) == 0
    assert out.tobytes() == want
