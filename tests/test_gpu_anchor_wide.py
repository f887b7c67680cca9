"""GPU: the wide anchored window (csrc/partition_plan.hpp part_plan, option "anchor_wide").

Where exactly one bit of r lies above the anchored window -- BLS12-377's Fr at c = 12, 14, 18, 21 -- that bit rides in the anchored window
and the magnitudes above 2^(c-1) use the bucket set that belonged to the one-bit window; the host adds 2^(c-1) times that set's plain sum
and 2^(c a + c) times the sum of the bases.  Every result below is the oracle's bytes, with the option on and off; the number of entries
the device grouped is the number of non-zero digits of the host model (tests/anchor_wide_cases.py).  A scalar with bits above bits(r)
makes the engine repeat the batch without the option (counter "anchor_wide_fallbacks"); two such batches in a row switch it off.

The device's entry count is query("sorted_entries") (read back from the device); last_timings()["entries"] is the CAPACITY windows x n."""
import numpy as np
import pytest

import anchor_wide_cases as m

pytestmark = pytest.mark.gpu

N = 1 << 12
NAMES = {0: "bls12_377_g1", 1: "bls12_381_g1", 2: "bls12_377_g2"}
STRIDE = {0: 104, 1: 104, 2: 200}
INF_AT = 77        # this base is the point at infinity: no entry, and not in the sum of the bases


def _bytes(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def _to_np(vals):
    return np.stack([_bytes(v) for v in vals])


def _oracle(oracle, cid, bases, sc):
    out = np.zeros(288 if cid >= 2 else 144, dtype=np.uint8)
    bases, sc = np.ascontiguousarray(bases), np.ascontiguousarray(sc)
    assert oracle.oracle_msm(cid, bases.ctypes.data, STRIDE[cid], sc.ctypes.data, len(sc), out.ctypes.data, 0) == 0
    return out.tobytes()


def _scalar_sets(seed):
    """name -> list of N integers.  One list serves both window sizes (the edge values of c = 12 and of c = 14 are all in it)."""
    import random

    rng = random.Random(seed)
    uniform = [rng.randrange(m.R377) for _ in range(N)]
    edges = list(uniform)
    planted = m.edge_scalars(12) + m.edge_scalars(14)
    assert 5 * len(planted) + 3 < N
    for i, v in enumerate(planted):
        edges[3 + 5 * i] = v
    one_bad = list(uniform)
    one_bad[1234] = (1 << 253) | rng.randrange(1 << 253)
    return {"edges": edges, "uniform": uniform, "equal": [uniform[5]] * N, "any256": [rng.randrange(1 << 256) for _ in range(N)],
            "one_bad": one_bad}


@pytest.fixture(scope="module", params=[0, 2], ids=lambda c: NAMES[c])
def case(request, ea, oracle):
    """bases, scalar sets and the oracle's bytes for them, once per curve"""
    cid = request.param
    bases = ea.generate_points(N, distinct=257, seed=310 + cid, curve=NAMES[cid])
    bases[INF_AT, -8] = 1
    sets = _scalar_sets(cid)
    exp = {}
    for name, vals in sets.items():
        # (on bases of the prime-order subgroup k P = (k mod r) P, and the oracle truncates above the last full window)
        exp[name] = _oracle(oracle, cid, bases, _to_np([v % m.R377 for v in vals]))
    ctx = ea.multi_scalar_mult_init(bases, NAMES[cid])
    ctx.set_option("anchor", 2)        # the anchored window at any size and window size
    yield cid, bases, sets, exp, ctx
    ctx.close()


def _model_entries(vals, c, wide):
    return sum(len(m.recode(v, c, 253, wide)[0]) for i, v in enumerate(vals) if i != INF_AT)


@pytest.mark.parametrize("c", [12, 14])
@pytest.mark.parametrize("wide", [1, 0])
def test_canonical_scalars_give_the_oracles_bytes_and_the_models_entry_count(case, c, wide):
    cid, bases, sets, exp, ctx = case
    ctx.set_option("window_bits", c)
    ctx.set_option("anchor_wide", wide)
    ctx.set_option("max_chunk", 0)
    before = ctx.query("anchor_wide_fallbacks")
    for name in ("edges", "uniform", "equal"):
        assert ctx.run(_to_np(sets[name]))[0] == exp[name], (name, c, wide)
        assert ctx.query("anchored_window") == 253 // c and ctx.query("anchor_wide_active") == wide
        t = ctx.last_timings()
        assert t["window_bits"] == c and t["windows"] == m.windows_of(c)        # the bucket sets and the key space stay
        assert ctx.query("sorted_entries") == _model_entries(sets[name], c, bool(wide)), (name, c, wide)
    assert ctx.query("anchor_wide_fallbacks") == before
    # ... and the option saves what it says: no entry for the top bit (14.3 % of uniform scalars have it; carries are gone either way)
    if wide:
        assert _model_entries(sets["uniform"], c, True) < _model_entries(sets["uniform"], c, False) - N // 10


@pytest.mark.parametrize("c", [12, 14])
def test_carried_batch_of_host_scalars(case, c):
    cid, bases, sets, exp, ctx = case
    ctx.set_option("window_bits", c)
    ctx.set_option("max_chunk", 1025)
    try:
        for wide in (1, 0):
            ctx.set_option("anchor_wide", wide)
            assert ctx.run(_to_np(sets["edges"]))[0] == exp["edges"], (c, wide)
            assert ctx.query("anchor_wide_active") == wide and ctx.last_timings()["launches"] >= -(-N // 1025)
    finally:
        ctx.set_option("max_chunk", 0)


@pytest.mark.parametrize("c", [12, 14])
def test_scalars_above_the_modulus_bits_fall_back_and_twice_in_a_row_switch_it_off(case, c):
    cid, bases, sets, exp, ctx = case
    ctx.set_option("window_bits", c)
    ctx.set_option("max_chunk", 0)
    ctx.set_option("anchor_wide", 1)        # (re-arms a context an earlier case has switched off)
    f0, d0 = ctx.query("anchor_wide_fallbacks"), ctx.query("anchor_wide_demotions")
    # one scalar with bit 253 set among canonical ones: the batch runs again without the option, the same bytes
    assert ctx.run(_to_np(sets["one_bad"]))[0] == exp["one_bad"]
    assert ctx.query("anchor_wide_fallbacks") == f0 + 1 and ctx.query("anchor_wide_active") == 0
    assert ctx.query("anchor_wide") == 1 and ctx.query("anchor_wide_demotions") == d0
    # a clean batch in between: the option is in use again, and the streak starts over
    assert ctx.run(_to_np(sets["uniform"]))[0] == exp["uniform"] and ctx.query("anchor_wide_active") == 1
    assert ctx.run(_to_np(sets["any256"]))[0] == exp["any256"]
    assert ctx.query("anchor_wide_fallbacks") == f0 + 2 and ctx.query("anchor_wide") == 1
    # the second such batch in a row (a carried one: the whole batch is repeated): the context stops using the option
    ctx.set_option("max_chunk", 1500)
    try:
        assert ctx.run(_to_np(sets["one_bad"]))[0] == exp["one_bad"]
    finally:
        ctx.set_option("max_chunk", 0)
    assert ctx.query("anchor_wide_fallbacks") == f0 + 3
    assert ctx.query("anchor_wide") == 0 and ctx.query("anchor_wide_demotions") == d0 + 1
    assert ctx.run(_to_np(sets["any256"]))[0] == exp["any256"]
    assert ctx.query("anchor_wide_fallbacks") == f0 + 3 and ctx.query("anchor_wide_active") == 0
    assert ctx.run(_to_np(sets["edges"]))[0] == exp["edges"] and ctx.query("anchor_wide_active") == 0
    ctx.set_option("anchor_wide", 1)
    assert ctx.query("anchor_wide") == 1


def test_bls12_381_has_no_wide_window(ea, oracle):
    """255 = 15 x 17: the anchored window at c = 17 has no bit above it; the option changes nothing."""
    import random

    rng = random.Random(381)
    vals = [rng.randrange(m.R381) for _ in range(N)]
    for i, v in enumerate([0, 1, m.R381 - 1, (1 << 255) - 1, 1 << 254]):
        vals[7 * i] = v
    sc = _to_np(vals)
    bases = ea.generate_points(N, distinct=257, seed=381, curve=NAMES[1])
    exp = _oracle(oracle, 1, bases, _to_np([v % m.R381 for v in vals]))
    ctx = ea.multi_scalar_mult_init(bases, NAMES[1])
    ctx.set_option("anchor", 2)
    ctx.set_option("window_bits", 17)
    assert ctx.query("anchor_wide") == 1
    assert ctx.run(sc)[0] == exp
    assert ctx.query("anchored_window") == 15 and ctx.query("anchor_wide_active") == 0 and ctx.query("anchor_wide_fallbacks") == 0
    assert ctx.query("sorted_entries") == sum(len(m.recode(v, 17, 255, False)[0]) for v in vals)
    ctx.close()
