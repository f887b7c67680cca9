"""CPU: the integer reference of tests/groth16_cases.py (what tests/test_gpu_groth16.py judges whole proofs by), judged first.  The
verifier's equation in the exponent accepts every satisfied case and rejects every unsatisfied one, a changed public input and a moved
h(tau); the CRS logs agree with the instance's own a and b at tau; the edges the generator promises are there, counted."""
import random

import pytest

import groth16_cases as gc
import ntt_cases as nc

CASES = gc.cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_exponent_identity_accepts_satisfied_and_rejects_unsatisfied(case):
    for which, inst in ((0, case.instance()), (1, case.second())):
        assert inst.is_satisfied()
        proof = case.setup().prove(inst, *case.randomizers(which))
        assert case.setup().verifies(proof), (case, which)
    bad = case.instance(False)
    assert not bad.is_satisfied() and bad.z == case.instance().z and bad.A == case.instance().A and bad.B == case.instance().B
    assert sum(x != y for x, y in zip(bad.C, case.instance().C)) == 1
    assert not case.setup(False).verifies(case.setup(False).prove(bad, *case.randomizers()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_changed_public_input_and_a_moved_h_are_rejected(case):
    st, inst = case.setup(), case.instance()
    r = nc.modulus(case.family)
    proof = st.prove(inst, *case.randomizers())
    for i in range(case.num_inputs):
        z_pub = list(inst.z[:case.num_inputs])
        z_pub[i] = (z_pub[i] + 1) % r
        assert not st.verifies(proof, z_pub), i
    assert st.verifies(proof, inst.z[:case.num_inputs])
    for shift in (1, r - 1, pow(st.tau, st.size // 2, r)):
        moved = st.prove(inst, *case.randomizers(), h_shift=shift)
        assert moved["h_tau"] == (proof["h_tau"] + shift) % r and moved["a"] == proof["a"] and moved["b"] == proof["b"]
        assert (moved["c"] - proof["c"]) % r == shift * st.t * pow(st.delta, -1, r) % r
        assert not st.verifies(moved), shift


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_queries_agree_with_the_instance_at_tau(case):
    """sum z_i u_i == sum L_j a_j over the padded a (the input rows included), sum z_i v_i == sum L_j b_j, and for a satisfied instance
    sum z_i w_i == sum L_j a_j b_j; h(tau) t is the difference, and h_query's logs are tau^j t / delta"""
    r = nc.modulus(case.family)
    for inst in (case.instance(), case.second()):
        st = case.setup()
        a, b = inst.padded(st.size)
        dot = lambda x, y: sum(p * q for p, q in zip(x, y)) % r
        assert dot(inst.z, st.u) == dot(st.lag, a)
        assert dot(inst.z, st.v) == dot(st.lag, b)
        assert dot(inst.z, st.w) == dot(st.lag, [x * y for x, y in zip(a, b)])
        assert st.h_at_tau(inst) * st.t % r == (dot(st.lag, a) * dot(st.lag, b) - dot(inst.z, st.w)) % r
    bad = case.setup(False)
    a, b = bad.inst.padded(bad.size)
    assert (dot(bad.inst.z, bad.w) - dot(bad.lag, [x * y for x, y in zip(a, b)])) % r == bad.lag[case.n // 2] * bad.inst.z[bad.inst.out(case.n // 2)] % r
    assert pow(st.tau, st.size, r) != 1 and all(2 <= x < r for x in (st.tau, st.alpha, st.beta, st.gamma, st.delta))
    assert (st.tau, st.alpha, st.beta, st.gamma, st.delta) == (bad.tau, bad.alpha, bad.beta, bad.gamma, bad.delta)
    assert len(st.h_query) == st.size - 1 and len(st.a_query) == len(st.b_query) == case.nvars
    assert len(st.l_query) == case.nvars - case.num_inputs and len(st.gamma_abc) == case.num_inputs
    for j in (0, 1, st.size - 2):
        assert st.h_query[j] * st.delta % r == pow(st.tau, j, r) * st.t % r


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_planted_edges_are_there(case):
    inst, st = case.instance(), case.setup()
    r = nc.modulus(case.family)
    ni, nvars = case.num_inputs, case.nvars
    assert (inst.n, inst.nvars, inst.num_inputs) == (case.n, nvars, ni) and case.n + ni + case.slack == st.size
    priv = inst.z[ni:]
    assert inst.z[0] == 1 and len(inst.z) == nvars
    assert 0 in priv and 1 in priv and r - 1 in priv
    small = sum(1 for x in priv if x in (0, 1))
    assert 0.35 * len(priv) <= small <= 0.65 * len(priv), (small, len(priv))
    if ni > 1:
        assert inst.z[ni - 1] == 0 and gc.zero_logs(st.gamma_abc) == 0
    # the variables of no row of A: private, at least two, and exactly the infinities of a_query
    cols = lambda rows: {j for rw in rows for _, j in rw}
    not_a = set(range(nvars)) - cols(inst.A)
    assert set(inst.no_a) <= not_a and len(inst.no_a) >= 3 and min(inst.no_a) >= ni
    assert [i for i, x in enumerate(st.a_query) if x == 0] == sorted(i for i in not_a if i >= ni)
    assert gc.zero_logs(st.a_query[:ni]) == 0                                   # a public variable has its own row L_{n+i}
    # most variables are in no row of B: most of b_g1_query / b_g2_query is infinity, and not all of it
    in_b = cols(inst.B)
    assert in_b <= set(inst.in_b) and 2 * len(in_b) < nvars
    assert [i for i, x in enumerate(st.b_query) if x == 0] == sorted(set(range(nvars)) - in_b)
    assert nvars // 2 < gc.zero_logs(st.b_query) < nvars
    # one private variable in no row of A, B or C: the infinity of l_query (the other no_a variables are in B or C)
    none = set(range(nvars)) - cols(inst.A) - in_b - cols(inst.C)
    assert inst.dead in none and inst.dead >= ni
    assert [i + ni for i, x in enumerate(st.l_query) if x == 0] == sorted(i for i in none if i >= ni)
    # C: one entry a row, on the row's own output, whose value is not 0; no coefficient is 0
    assert all(len(rw) == 1 and rw[0][1] == inst.out(i) and rw[0][0] and inst.z[inst.out(i)] for i, rw in enumerate(inst.C))
    assert gc.zero_logs(st.h_query) == 0
    # the second assignment: the same lists, other values, public inputs included
    other = case.second()
    assert other.A is inst.A and other.B is inst.B and other.C is inst.C
    assert other.z[0] == 1 and other.z != inst.z and (ni == 1 or other.z[1:ni] != inst.z[1:ni]) and other.a != inst.a and other.b != inst.b


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_without_randomizers_the_proof_is_the_non_hiding_one(case):
    st, inst = case.setup(), case.instance()
    r = nc.modulus(case.family)
    ni = case.num_inputs
    dot = lambda x, y: sum(p * q for p, q in zip(x, y)) % r
    plain = st.prove(inst, 0, 0)
    assert plain["a"] == (st.alpha + dot(inst.z, st.u)) % r
    assert plain["b"] == (st.beta + dot(inst.z, st.v)) % r
    assert plain["c"] * st.delta % r == (dot(inst.z[ni:], st.lq[ni:]) + plain["h_tau"] * st.t) % r
    assert st.verifies(plain)
    # and the randomizers move every element by what the formulas say
    r_, s_ = case.randomizers()
    hid = st.prove(inst, r_, s_)
    assert (hid["a"] - plain["a"]) % r == r_ * st.delta % r and (hid["b"] - plain["b"]) % r == s_ * st.delta % r
    assert (hid["c"] - plain["c"]) % r == (s_ * hid["a"] + r_ * hid["b"] - r_ * s_ * st.delta) % r
    assert hid["x"] == plain["x"] and hid["h_tau"] == plain["h_tau"]


def test_the_case_list():
    assert [(c.family, c.k, c.slack, c.num_inputs) for c in CASES] == [(f, k, s, ni) for f in ("bls12_377", "bls12_381")
                                                                      for k, s, ni in ((4, 0, 3), (6, 9, 3), (10, 0, 3), (4, 0, 1))]
    assert all(c.n == c.size - c.num_inputs - c.slack for c in CASES)
    assert len({c.setup().tau for c in CASES}) == len(CASES)                     # seeded from the name: no two cases share the waste
    rng = random.Random(1)
    again = gc.Instance("bls12_381", 13, 24, 3, rng)
    assert again.is_satisfied() and len(again.z) == 24
