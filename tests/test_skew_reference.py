"""CPU: the fold-by-tile reference of tests/skew_cases.py (what the skewed-input GPU tests are checked against at 2^20..2^26 pairs)
equals the oracle run directly on the expanded arrays, for every scalar generator, on all four curves -- and it notices a single bit."""
import numpy as np
import pytest

import skew_cases as sk


def _cases(ea, cid, n):
    """(name, tile, scalars) for every generator on a random tile, and the degenerate tiles"""
    D = 64
    c = ea.plan(n, sk.NAMES[cid])["window_bits"]
    tile = sk.random_tile(ea, cid, D, seed=20 + cid)
    out = [(name, tile, sk.make_scalars(name, cid, n, seed=30 + i)) for i, name in enumerate(sk.GENERATORS)]
    out.append(("window_periodic", tile, sk.make_scalars("window_periodic", cid, n, 5, c=c)))
    out.append(("window_periodic_c23", tile, sk.make_scalars("window_periodic", cid, n, 6, c=23)))
    out.append(("infinity_in_tile", sk.random_tile(ea, cid, D, seed=40 + cid, infinity_at=7), sk.make_scalars("witness", cid, n, 7)))
    out.append(("same_base", sk.same_base_tile(ea, cid, seed=50 + cid), sk.make_scalars("all_equal", cid, n, 8)))
    out.append(("cancel", sk.cancel_tile(ea, cid, seed=60 + cid), sk.make_scalars("all_equal", cid, n, 9)))
    out.append(("cancel_pairs", sk.cancel_tile(ea, cid, seed=70 + cid, pairs=16), sk.cancel_scalars(sk.make_scalars("zeros_90", cid, n, 10))))
    return out


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_fold_reference_equals_the_direct_oracle(ea, oracle, cid):
    n = 1 << 14 if cid < 2 else 1 << 12
    infinity = None
    for name, tile, sc in _cases(ea, cid, n):
        got = sk.fold_reference(oracle, cid, tile, sc)
        assert got == sk.oracle_msm(oracle, cid, sk.expand(tile, n), sc), (sk.NAMES[cid], name)
        if name == "all_zero":
            infinity = got
    # the degenerate cases are what they claim to be
    cases = {name: (tile, sc) for name, tile, sc in _cases(ea, cid, 256)}
    assert sk.fold_reference(oracle, cid, *cases["cancel"]) == infinity
    assert sk.fold_reference(oracle, cid, *cases["cancel_pairs"]) == infinity
    assert sk.fold_reference(oracle, cid, *cases["all_one"]) != infinity


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_fold_reference_sees_one_bit(ea, oracle, cid):
    """Flipping any single bit of a single scalar changes the reference (low, middle, top bit; the sum over T must not lose it)."""
    n = 1 << 12
    tile = sk.random_tile(ea, cid, 32, seed=80 + cid)
    sc = sk.make_scalars("witness", cid, n, 11)
    base = sk.fold_reference(oracle, cid, tile, sc)
    for row, bit in ((0, 0), (n - 1, 0), (1234, 77), (n // 2, sk.scalar_bits(cid) - 2), (777, 255)):
        flipped = sc.copy()
        flipped[row, bit // 8] ^= np.uint8(1 << (bit % 8))
        assert sk.fold_reference(oracle, cid, tile, flipped) != base, (sk.NAMES[cid], row, bit)


def test_fold_scalars_is_exact_at_the_limits():
    """The uint64 column sums are exact: T copies of 2^256 - 1 fold to T (2^256 - 1) mod r, checked with Python integers."""
    for cid in (0, 1):
        D, T = 3, 1 << 16
        sc = np.full((D * T, 32), 0xFF, dtype=np.uint8)
        sc[1::D] = sk.make_scalars("r_minus_1", cid, T, 0)
        got = [int.from_bytes(row.tobytes(), "little") for row in sk.fold_scalars(cid, sc, D)]
        r = sk.r_of(cid)
        assert got == [T * ((1 << 256) - 1) % r, T * (r - 1) % r, T * ((1 << 256) - 1) % r]


def test_generators_are_seeded_and_shaped():
    for cid in (0, 1):
        r = sk.r_of(cid)
        for name in sk.GENERATORS:
            a, b = sk.make_scalars(name, cid, 4096, 1), sk.make_scalars(name, cid, 4096, 1)
            assert np.array_equal(a, b), name
            vals = {int.from_bytes(row.tobytes(), "little") for row in a}
            assert all(v < r for v in vals), name
        w = sk.make_scalars("witness", cid, 1 << 14, 2)
        small = np.all(w[:, 1:] == 0, axis=1) & (w[:, 0] <= 1)
        assert 0.93 < small.mean() < 0.97
        assert np.all(sk.make_scalars("short64", cid, 1000, 3)[:, 8:] == 0)
        top = {int.from_bytes(row.tobytes(), "little") for row in sk.make_scalars("top_only", cid, 1000, 4)}
        sh = sk.scalar_bits(cid) - 8
        assert all(v % (1 << sh) == 0 for v in top) and len(top) > 100
        z = sk.make_scalars("zeros_90", cid, 1 << 14, 5)
        assert 0.88 < np.all(z == 0, axis=1).mean() < 0.92
        assert len({row.tobytes() for row in sk.make_scalars("two_values", cid, 1000, 6)}) == 2


def test_digit_model_sees_the_hot_buckets():
    """The coverage model (skew_cases.hot_spots): equal scalars put all n entries of a window in one bucket; window_periodic with shared
    bucket sets puts every window's entries in ONE bucket; uniform scalars spread."""
    n, c = 1 << 12, 16
    windows = (257 + c - 1) // c
    assert sk.hot_spots(sk.make_scalars("all_equal", 0, n, 1), c, windows, 10)[:2] == (n, n)
    periodic = sk.make_scalars("window_periodic", 0, n, 1, c=c)
    filled = (253 - 1) // c
    assert sk.hot_spots(periodic, c, windows, 10)[0] == n
    assert sk.hot_spots(periodic, c, 1, 10)[0] == filled * n
    # the anchored window: a zero scalar still has an entry there, at magnitude 2^(c-1)
    a = sk.anchor_window(21, 253)
    assert a == 11 and sk.anchor_window(20, 253) is None and sk.anchor_window(17, 255) == 14
    assert sk.hot_spots(sk.make_scalars("all_zero", 0, n, 1), 21, 13, 10, anchor=a) == (n, n, n)
    assert sk.hot_spots(sk.make_scalars("all_zero", 0, n, 1), 21, 13, 10) == (0, 0, 0)
    hb, seg, _ = sk.hot_spots(sk.make_scalars("zeros_90", 0, n, 1), c, windows, 10)
    assert hb < n // 20 and seg < n // 4
    # digits reassemble the scalar: sum_w (+-mag_w) 2^(c w) == k
    sc = sk.make_scalars("two_values", 1, 8, 3)
    for cc in (7, 16, 21):
        mag = sk.digits(sc, cc)
        for i in range(8):
            k = int.from_bytes(sc[i].tobytes(), "little")
            # recover the signs from the carries: a window is negative iff its raw value plus carry exceeded 2^(c-1)
            total, carry = 0, 0
            for w in range(mag.shape[0]):
                u = (k >> (cc * w)) & ((1 << cc) - 1)
                v = u + carry
                neg = v > (1 << (cc - 1))
                assert int(mag[w, i]) == ((1 << cc) - v if neg else v)
                total += (-int(mag[w, i]) if neg else int(mag[w, i])) << (cc * w)
                carry = int(neg)
            assert total == k
