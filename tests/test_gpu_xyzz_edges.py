"""GPU: the 14 x 28 XYZZ laws of csrc/curve.hpp (xyzz_madd / xyzz_madd_common / xyzz_add / xyzz_add_quad / xyzz_dbl and the
two-lane forms of csrc/fp2pair.hpp) at the corners of their own contract, three ways: device limbs == checker-armed host limbs ==
a big-integer formula model (tests/xyzz_edge_cases.py).

What tests/test_gpu_devtest.py::test_xyzz_additions_match_the_affine_model leaves open: it feeds a few hundred real curve points
whose stored X / Y are normalized and never near the 16p cap, with the five special cases in the first five lanes.  Here

  * every stored coordinate class of the invariant (limbs at 2^28 + 15, the top limb at the 16p cap, single cold / hot limbs, what
    fe_carry leaves, canonical + k p) meets every class-M class (limbs at 2^28 - 1 under the top limb of 1.5p, 1, p - 1, p + 1,
    3p/2 - 1, cold limbs) -- 2^13 records per op and curve;
  * the same-x branches (doubling, cancellation, "same x, other y", and near misses) are DERIVED from accumulators of those classes,
    and they, the infinity records and acc_inf are dealt among the general records so that every wave -- 64, 32 or 16 records of
    it -- holds several kinds: the four-lane and two-lane forms decide these cases per quad / pair by DPP;
  * every output must be a stored point again (the closure the lazy schedule relies on), and 32-round trajectories that feed output
    limbs back in start from the all-maximal accumulator.

No record is left out of the value check: the model follows every branch of the code.
Reference counterpart of the laws: SPK ec/xyzz_t.hpp:97-249 (EFD madd-2008-s, add-2008-s, dbl-2008-s-1, mdbl-2008-s-1)."""
import numpy as np
import pytest

import test_gpu_devtest as g
import xyzz_edge_cases as x
from test_gpu_devtest import arr, run_both

pytestmark = pytest.mark.gpu
libs = g.libs   # the module-scoped fixture of test_gpu_devtest (device + host library)

N_RECORDS = 1 << 13       # per op and curve
N_TRAJECTORIES, N_ROUNDS = 256, 32


def check_values(f, tag, recs, out, expected):
    """invariant on every record, value against the model on every record"""
    vals = x.raw_values(f, out)
    x.assert_stored_point_invariant(f, out, vals, tag)
    for i, exp in enumerate(expected):
        assert x.same_result(f, x.residues(f, vals[i]), exp), f"{tag}: record {i} differs from the formula model: in={recs[i].tolist()} out={out[i].tolist()}"


def check_madd(libs, cid, n):
    """MADD and MADD_COMMON (and their paired forms on G2) on n mixed records"""
    gen = x.Gen(cid, 0xED6E + cid)
    f = gen.f
    general, n_struct = x.madd_general(gen, x.n_general(n))
    rl, kinds, src = x.mixed(gen, n, general, x.MADD_SPECIAL, x.madd_special)
    x.assert_waves_are_mixed(kinds)
    assert sum(1 for s in src if 0 <= s < n_struct) == n_struct          # every structured record is in
    recs = arr(rl)
    expected, same_x = [], []
    for r in rl:
        exp, sx = x.model_madd(f, f.point(r), f.point(r[4 * f.ew:], 2), r[-1] & 1, r[-1] & 2)
        expected.append(exp)
        same_x.append(sx)
    # the constructions do what they say: the model takes the same-x branch on every record derived for it and on no other special
    # one (a general record may: an all-zero X against a base with x = 0 or p)
    for i, k in enumerate(kinds):
        assert k == "general" or same_x[i] == (k in ("double", "cancel", "same_x_inf")), (i, k)
    assert sum(1 for e, s in zip(expected, same_x) if s and e is not None) >= n // 32      # doublings that really double
    out, _ = run_both(libs, cid, "MADD", recs)
    assert (out[:, 4 * f.ew] == 0).all()
    check_values(f, f"MADD curve {cid}", recs, out, expected)
    com, _ = run_both(libs, cid, "MADD_COMMON", recs)
    sx = np.array(same_x)
    bad = np.nonzero((com[:, 4 * f.ew] != 0) != sx)[0]
    assert bad.size == 0, f"MADD_COMMON curve {cid}: 'same x' flag wrong on {bad.size} records, first {bad[0]} ({kinds[bad[0]]}): in={recs[bad[0]].tolist()}"
    assert (com[:, 4 * f.ew] <= 1).all()
    assert (com[sx, :4 * f.ew] == recs[sx, :4 * f.ew]).all()             # untouched: the caller re-reads the base and finishes
    check_values(f, f"MADD_COMMON curve {cid}", recs, com, [f.point(r) if s else e for r, e, s in zip(rl, expected, same_x)])


def check_add(libs, cid, n):
    """ADD (and its paired form on G2) and ADD_QUAD on n mixed records"""
    gen = x.Gen(cid, 0xADD0 + cid)
    f = gen.f
    general, n_struct = x.add_general(gen, x.n_general(n))
    rl, kinds, src = x.mixed(gen, n, general, x.ADD_SPECIAL, x.add_special)
    x.assert_waves_are_mixed(kinds)
    assert sum(1 for s in src if 0 <= s < n_struct) == n_struct
    recs = arr(rl)
    expected = [x.model_add(f, f.point(r), f.point(r[4 * f.ew:])) for r in rl]
    # doublings double, cancellations and "same x, other y" end at infinity, near misses do not
    for i, k in enumerate(kinds):
        if k in ("cancel", "same_x_inf") and not f.is_zero(f.val(rl[i][f.ew:2 * f.ew])):
            assert expected[i] is None, (i, k)
        if k in ("double", "near_miss"):
            assert expected[i] is not None, (i, k)
    out, _ = run_both(libs, cid, "ADD", recs)
    check_values(f, f"ADD curve {cid}", recs, out, expected)
    quad, _ = run_both(libs, cid, "ADD_QUAD", recs, host_too=False)       # (may differ limb-wise from the one-lane form)
    if quad is not None:
        check_values(f, f"ADD_QUAD curve {cid}", recs, quad, expected)


def check_dbl(libs, cid, n):
    gen = x.Gen(cid, 0xDB10 + cid)
    f = gen.f
    rl, _ = x.dbl_general(gen, n)
    gen.rng.shuffle(rl)
    recs = arr(rl)
    out, _ = run_both(libs, cid, "DBL", recs)
    check_values(f, f"DBL curve {cid}", recs, out, [x.model_dbl(f, f.point(r)) for r in rl])


def check_trajectories(libs, cid, n_acc, rounds):
    """rounds x (MADD with a fresh extreme base | ADD against a second running point | DBL), output limbs fed back as the next input,
    from the all-maximal accumulator and n_acc - 1 random extreme ones: device == host limbs, the invariant and the model step after
    every round."""
    gen = x.Gen(cid, 0x7EA9 + cid)
    f, rng = gen.f, gen.rng
    ew4 = 4 * f.ew
    start = arr([gen.max_acc()] + [gen.extreme_acc() for _ in range(n_acc - 1)])
    mp = x.M_EXTREME
    # mixed additions
    cur = start
    for rd in range(rounds):
        tail = arr([gen.cm(pool=mp) + gen.cm(pool=mp) + [rng.randrange(2)] for _ in range(n_acc)])
        if rd == 0:
            tail[0] = arr([gen.cm("max") + gen.cm("max") + [0]])[0]
        recs = np.ascontiguousarray(np.concatenate([cur, tail], axis=1))
        rl = recs.tolist()
        out, _ = run_both(libs, cid, "MADD", recs)
        check_values(f, f"MADD trajectory curve {cid} round {rd}", recs, out,
                     [x.model_madd(f, f.point(r), f.point(r[ew4:], 2), r[-1] & 1, 0)[0] for r in rl])
        cur = out[:, :ew4]
    # full additions: A += B on even rounds, B += A on odd ones.  B starts as A in half of the lanes (the all-maximal one among them),
    # so that round 0 doubles those
    a = start
    b = arr([start[i].tolist() if i % 2 == 0 else gen.extreme_acc() for i in range(n_acc)])
    for rd in range(rounds):
        acc, oth = (a, b) if rd % 2 == 0 else (b, a)
        recs = np.ascontiguousarray(np.concatenate([acc, oth], axis=1))
        rl = recs.tolist()
        expected = [x.model_add(f, f.point(r), f.point(r[ew4:])) for r in rl]
        out, _ = run_both(libs, cid, "ADD", recs)
        check_values(f, f"ADD trajectory curve {cid} round {rd}", recs, out, expected)
        quad, _ = run_both(libs, cid, "ADD_QUAD", recs, host_too=False)
        if quad is not None:
            check_values(f, f"ADD_QUAD trajectory curve {cid} round {rd}", recs, quad, expected)
        if rd % 2 == 0:
            a = out
        else:
            b = out
    # doublings
    cur = start
    for rd in range(rounds):
        out, _ = run_both(libs, cid, "DBL", cur)
        check_values(f, f"DBL trajectory curve {cid} round {rd}", cur, out, [x.model_dbl(f, f.point(r)) for r in cur.tolist()])
        cur = out


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_madd_at_the_edges_of_the_stored_point_bounds(libs, cid):
    check_madd(libs, cid, N_RECORDS)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_add_and_add_quad_at_the_edges_of_the_stored_point_bounds(libs, cid):
    check_add(libs, cid, N_RECORDS)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_dbl_at_the_edges_of_the_stored_point_bounds(libs, cid):
    check_dbl(libs, cid, N_RECORDS)


@pytest.mark.parametrize("cid", [0, 1, 2, 3])
def test_trajectories_from_the_extreme_accumulators_stay_inside_the_contract(libs, cid):
    check_trajectories(libs, cid, N_TRAJECTORIES, N_ROUNDS)
