"""GPU: the sorted entries as 32-bit words with run steps (csrc/msm_types.hpp Entries32, option "entries32").

The last grouping pass writes one word per entry -- base index, sign, and the key's step from the entry before -- and the key itself
only at escapes and lane starts (run_keys); the accumulation rebuilds the keys from the steps.  Every result below is the oracle's
bytes AND the bytes of the same context with the option off, and every positive case checks that the format was really in use
("entries32_active") behind at least one grouping pass.

Shapes are small (n <= 2^14, forced window size and lane length) with one exception: a segment is cut into sub-jobs -- the path on
which every run start is an escape -- only above PART_SUBJOB = 196608 entries, so the all-equal-scalars case also runs once at
2^18 + 37 pairs, the smallest power of two at which one window's entries exceed that."""
import random

import numpy as np
import pytest

import anchor_wide_cases as m

pytestmark = pytest.mark.gpu

N = 1 << 12
NAMES = {0: "bls12_377_g1", 1: "bls12_381_g1", 2: "bls12_377_g2"}
STRIDE = {0: 104, 1: 104, 2: 200}
MOD = {0: m.R377, 1: m.R381, 2: m.R377}


def _to_np(vals):
    return np.stack([np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8) for v in vals])


def _oracle(oracle, cid, bases, sc):
    out = np.zeros(288 if cid >= 2 else 144, dtype=np.uint8)
    bases, sc = np.ascontiguousarray(bases), np.ascontiguousarray(sc)
    assert oracle.oracle_msm(cid, bases.ctypes.data, STRIDE[cid], sc.ctypes.data, len(sc), out.ctypes.data, 0) == 0
    return out.tobytes()


def _both(ctx, sc, exp, what=None, active=1, npoints=None):
    """the option on (and in use), then off: the oracle's bytes both times"""
    ctx.set_option("entries32", 1)
    got = ctx.run(sc, npoints)[0]
    assert ctx.query("entries32_active") == active and ctx.query("group_passes") >= 1, what
    assert got == exp, what
    ctx.set_option("entries32", 0)
    try:
        assert ctx.run(sc, npoints)[0] == exp, what
        assert ctx.query("entries32_active") == 0, what
    finally:
        ctx.set_option("entries32", 1)


@pytest.fixture(scope="module")
def g1(ea):
    """BLS12-377 G1: bases (one of them the point at infinity) and a context, shared by the cases below"""
    bases = ea.generate_points(N, distinct=257, seed=3201, curve=NAMES[0])
    bases[77, -8] = 1
    ctx = ea.multi_scalar_mult_init(bases, NAMES[0])
    assert ctx.query("entries32") in (0, 1)
    yield bases, ctx
    ctx.close()


def _reset(ctx, c=12, K=0):
    for k, v in (("window_bits", c), ("lane_entries", K), ("max_chunk", 0), ("anchor", 1), ("anchor_wide", 1), ("carry", 1)):
        ctx.set_option(k, v)


def test_crafted_gaps(g1, oracle):
    """Scalars bucket << (c w): the used buckets of window 1 lie 29, 30, 31 and 32 apart (steps 29 and 30, then two escapes); buckets of
    windows 0 and 1 that are neighbours in key space (the last of one, the first of the next: another segment, an escape) and 32 apart
    across the boundary; window 2 holds one lone bucket."""
    bases, ctx = g1
    c, half = 12, 1 << 11
    crafted = []
    b = 100
    for gap in (0, 29, 30, 31, 32):
        b += gap
        crafted += [b << c] * 3
    crafted += [half, half - 7, 1 << c, 25 << c, 1500 << (2 * c)]          # digit 2^(c-1) is the last bucket of its window
    crafted += [(half << 0) | (1 << c), (half - 7) | (25 << c)]            # ... and both digits in one scalar
    vals = [crafted[i % len(crafted)] for i in range(N)]
    vals[5] = 0
    sc = _to_np(vals)
    exp = _oracle(oracle, 0, bases, sc)
    for K in (0, 8):
        _reset(ctx, c, K)
        _both(ctx, sc, exp, ("gaps", K))
    assert ctx.last_timings()["window_bits"] == c


def test_all_scalars_equal(g1, oracle):
    bases, ctx = g1
    rng = random.Random(11)
    sc = _to_np([rng.randrange(m.R377)] * N)
    exp = _oracle(oracle, 0, bases, sc)
    for K in (0, 24):
        _reset(ctx, 12, K)
        _both(ctx, sc, exp, ("equal", K))


def test_all_scalars_equal_in_sub_jobs(ea, oracle):
    """One window's entries in ONE segment of more than PART_SUBJOB entries: the segment is cut into sub-jobs (k_pass_hist, k_pass_scan,
    the first blocks of k_pass_scatter), whose run starts are all escapes; the sub-job that starts a run is the one whose row of positions
    still equals the bin's start."""
    n = (1 << 18) + 37
    bases = ea.generate_points(n, distinct=257, seed=3218, curve=NAMES[0])
    rng = random.Random(12)
    # two values, in two blocks: a bin whose run starts in a later sub-job than the segment's first
    a, b = rng.randrange(m.R377), rng.randrange(m.R377)
    sc = _to_np([a] * (n - 5000) + [b] * 5000)
    exp = _oracle(oracle, 0, bases, sc)
    ctx = ea.multi_scalar_mult_init(bases, NAMES[0])
    try:
        ctx.set_option("window_bits", 12)
        _both(ctx, sc, exp, "sub-jobs")
    finally:
        ctx.close()


@pytest.mark.parametrize("K", [8, 24])
def test_lane_lengths(g1, oracle, K):
    """Short lanes: runs straddle lane boundaries (every bucket of c = 7 holds ~64 entries), the entry total is no multiple of K and
    the last lane is short."""
    bases, ctx = g1
    rng = random.Random(K)
    n = N - 3
    vals = [rng.randrange(m.R377) for _ in range(n)]
    for c in (7, 12):
        _reset(ctx, c, K)
        # the entry total is what the digits make it: where it happens to be a multiple of K, a scalar with a single digit moves it
        for fix in range(4):
            sc = _to_np(vals)
            ctx.set_option("entries32", 0)
            ctx.run(sc, n)
            if ctx.query("sorted_entries") % K != 0:
                break
            vals[10 + fix] = 1
        assert ctx.query("sorted_entries") % K != 0
        exp = _oracle(oracle, 0, bases[:n], sc)
        _both(ctx, sc, exp, ("lanes", K, c), npoints=n)
        assert ctx.last_timings()["lane_entries"] == K and ctx.query("sorted_entries") % K != 0


def test_inputs_without_entries(g1, ea, oracle):
    bases, ctx = g1
    _reset(ctx, 12, 8)
    zeros = np.zeros((N, 32), dtype=np.uint8)
    _both(ctx, zeros, _oracle(oracle, 0, bases, zeros), "zero scalars")
    assert ctx.query("sorted_entries") == 0
    # every base at infinity
    rng = random.Random(5)
    sc = _to_np([rng.randrange(m.R377) for _ in range(256)])
    inf = ea.generate_points(256, distinct=16, seed=9, curve=NAMES[0])
    inf[:, -8] = 1
    c2 = ea.multi_scalar_mult_init(inf, NAMES[0])
    try:
        c2.set_option("window_bits", 9)
        _both(c2, sc, _oracle(oracle, 0, inf, sc), "bases at infinity")
        assert c2.query("sorted_entries") == 0
    finally:
        c2.close()


def test_carried_batch_in_two_chunks(g1, oracle):
    """Edwards law: the second chunk accumulates onto the first chunk's buckets; a lane's first run starts from the stored bucket unless
    its first step says that it continues the lane before."""
    bases, ctx = g1
    rng = random.Random(21)
    vals = [rng.randrange(m.R377) for _ in range(N)]
    for i in range(0, N, 3):
        vals[i] = vals[0]          # a third of the entries of every window in one bucket: long runs, in both chunks
    sc = _to_np(vals)
    exp = _oracle(oracle, 0, bases, sc)
    for K in (8, 0):
        _reset(ctx, 9, K)
        ctx.set_option("max_chunk", N // 2 + 1)
        try:
            _both(ctx, sc, exp, ("carried", K))
            t = ctx.last_timings()
            assert t["launches"] == 2 and t["twisted_edwards"]
        finally:
            ctx.set_option("max_chunk", 0)


@pytest.mark.parametrize("law", ["377_sw", "381_g1", "377_g2_paired", "377_g2"])
def test_every_law(ea, oracle, law):
    cid = {"377_sw": 0, "381_g1": 1, "377_g2_paired": 2, "377_g2": 2}[law]
    n = N if cid < 2 else 1 << 10
    bases = ea.generate_points(n, distinct=131, seed=40 + cid, curve=NAMES[cid])
    bases[3, -8] = 1
    rng = random.Random(cid)
    vals = [rng.randrange(MOD[cid]) for _ in range(n)]
    vals[1] = vals[2] = vals[9]
    sc = _to_np(vals)
    exp = _oracle(oracle, cid, bases, sc)
    ctx = ea.MultiScalarMultContext(NAMES[cid])
    try:
        if law == "377_sw":
            ctx.set_option("twisted_edwards", 0)        # (before the bases: no Edwards image is kept)
        ctx.set_bases(bases)
        if cid == 2:
            ctx.set_option("g2_paired", 31 if law == "377_g2_paired" else 0)
        for c, K in ((11, 0), (8, 8)):
            ctx.set_option("window_bits", c)
            ctx.set_option("lane_entries", K)
            _both(ctx, sc, exp, (law, c, K))
            assert not ctx.last_timings()["twisted_edwards"]
    finally:
        ctx.close()


@pytest.mark.parametrize("wide", [1, 0])
def test_anchored_windows(g1, oracle, wide):
    """c = 12 on BLS12-377: the anchored window, plain and wide (253 = 21 x 12 + 1), forced at this size by "anchor" = 2."""
    bases, ctx = g1
    rng = random.Random(30 + wide)
    vals = [rng.randrange(m.R377) for _ in range(N)]
    for i, v in enumerate(m.edge_scalars(12)):
        if 3 + 5 * i < N:
            vals[3 + 5 * i] = v
    sc = _to_np(vals)
    exp = _oracle(oracle, 0, bases, sc)
    _reset(ctx, 12, 8)
    ctx.set_option("anchor", 2)
    ctx.set_option("anchor_wide", wide)
    try:
        _both(ctx, sc, exp, ("anchored", wide))
        assert ctx.query("anchored_window") == 21 and ctx.query("anchor_wide_active") == wide
    finally:
        ctx.set_option("anchor", 1)
        ctx.set_option("anchor_wide", 1)


def test_precomputed_tables_keep_the_64_bit_format(ea, oracle):
    n = 3000
    bases = ea.generate_points(n, distinct=100, seed=77, curve=NAMES[0])
    rng = random.Random(77)
    sc = _to_np([rng.randrange(m.R377) for _ in range(n)])
    exp = _oracle(oracle, 0, bases, sc)
    ctx = ea.MultiScalarMultContext(NAMES[0])
    try:
        ctx.set_option("precompute", 1)
        ctx.set_bases(bases)
        _both(ctx, sc, exp, "tables", active=0)
        assert ctx.last_timings()["tables"]
    finally:
        ctx.close()
