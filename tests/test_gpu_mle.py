"""GPU: dense multilinear extensions and sumcheck prover rounds over Fr (csrc/mle.hpp, csrc/msm_mle.hpp) through the Python layer, byte
for byte against Python big integers (tests/mle_cases.py) at every edge the kernels have -- tables below, at and above a tile, one, two
and three passes of fix_variables with the ping-pong, the half tables of eq, one, two and three reduction levels of a round, plain and
fused --; a whole proof accepted by a verifier written in Python integers and a tampered table rejected; the stream order of flag bit 1,
pinned with late producers as tests/test_gpu_stream_order.py pins the _device calls; and a speed guard against the forward transform."""
import os
import random
import re
import statistics
import time

import numpy as np
import pytest

import mle_cases as mc
import ntt_cases as nc
import stream_cases as st
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
# DESIGN.md 4k, by products (55 a point and 2 an element against the 16 an element of the forward NN transform of 2^20): one fused
# round of Spartan's list at nv = 22, mle_evaluate at nv = 24
MODEL_RATIO = {"round": 3.4, "evaluate": 2.0}


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def domains(ea):
    """one domain per (field, k) for the whole module"""
    made = {}

    def get(field, k, tile_log=0):
        if (field, k) not in made:
            made[(field, k)] = ea.Radix2EvaluationDomain(1 << k, CURVE_OF[field])
        d = made[(field, k)]
        d.set_option("poly_tile_log", tile_log)
        return d

    yield get
    for d in made.values():
        d.close()


def dev(torch, raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda().reshape(-1, 32)


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else (t.tobytes() if hasattr(t, "tobytes") else bytes(t))


# ---- fix_variables and evaluate ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile_log", [4, 10])
@pytest.mark.parametrize("field", FIELDS)
def test_fix_variables_against_the_model(domains, torch_, field, tile_log):
    """num_vars 0, 1, 2, one below, at and one above the tile; k = 0, 1, tile_log, tile_log + 1, 2 tile_log + 1, num_vars: one, two and
    three passes and the ping-pong; both forms; host and device pointers byte-equal"""
    r = nc.modulus(field)
    dom = domains(field, 4, tile_log)
    rng = random.Random(0xF1 + tile_log)
    passes = set()
    for nv, k in mc.fix_cases(tile_log):
        passes.add(max(1, -(-k // tile_log)))
        for montgomery in (True, False):
            table = mc.raw_bytes(mc.raw_values(field, 1 << nv, rng))
            point = [rng.randrange(r) for _ in range(k)]
            want = nc.encode(field, mc.fix_variables(r, nc.decode(field, table, not montgomery), point), not montgomery)
            host = raw_of(dom.mle_fix_variables(table, point, montgomery=montgomery))
            got = raw_of(dom.mle_fix_variables(dev(torch_, table), point, montgomery=montgomery))
            assert host == want, (nv, k, montgomery, "host")
            assert got == want, (nv, k, montgomery, "device")
            if k == nv:
                assert dom.mle_evaluate(dev(torch_, table), point, montgomery=montgomery) == mc.evaluate(r, nc.decode(field, table, not montgomery), point)
    assert passes == ({1, 2, 3} if tile_log == 4 else {1, 2})
    assert dom.query("mle_work_bytes") > 0


@pytest.mark.parametrize("field", FIELDS)
def test_equal_residues_give_equal_results(domains, torch_, field):
    """a table and a point, and the same residues written as other 256-bit patterns (v + r, v + 2r where they fit)"""
    r = nc.modulus(field)
    dom = domains(field, 4, 4)
    rng = random.Random(0xE0)
    nv, k = 6, 5
    vals = [rng.randrange(r) for _ in range(1 << nv)]
    other = [v + r * rng.randrange(1, ((1 << 256) - 1 - v) // r + 1) for v in vals]
    assert all(o < 1 << 256 and o % r == v for o, v in zip(other, vals)) and other != vals
    point = [rng.randrange(r) for _ in range(k)]
    for montgomery in (True, False):
        a = raw_of(dom.mle_fix_variables(dev(torch_, mc.raw_bytes(vals)), point, montgomery=montgomery))
        b = raw_of(dom.mle_fix_variables(dev(torch_, mc.raw_bytes(other)), point, montgomery=montgomery))
        assert a == b
        ea_, eb = dom.eq_table(point, montgomery=montgomery), dom.eq_table([p + r for p in point], montgomery=montgomery)
        assert raw_of(ea_) == raw_of(eb)


# ---- the eq table --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_eq_table_against_the_model(domains, torch_, field):
    r = nc.modulus(field)
    dom = domains(field, 4)
    rng = random.Random(0xE9)
    for k in (0, 1, 2, 3, 4, 7, 10, 12, 13):
        p = [rng.randrange(r) for _ in range(k)]
        want = mc.eq_table(r, p)
        assert sum(want) % r == 1
        for montgomery in (True, False):
            host = raw_of(dom.eq_table(p, montgomery=montgomery))
            got = dom.eq_table(p, montgomery=montgomery, device=True)
            assert host == nc.encode(field, want, not montgomery), (k, montgomery)
            assert raw_of(got) == host, (k, montgomery)
        assert sum(nc.decode(field, raw_of(got), True)) % r == 1
        if k:
            q = [rng.randrange(r) for _ in range(k)]
            assert dom.mle_evaluate(dom.eq_table(p, device=True), q) == dom.mle_evaluate(dom.eq_table(q, device=True), p)


# ---- one round -----------------------------------------------------------------------------------------------------------------------------

ROUND_NV = {"one table of degree 1": (1, 2, 3, 8, 13), "spartan": tuple(range(1, 14)), "hyperplonk": (1, 2, 6, 11, 13), "worst": (1, 2, 6, 10)}


@pytest.mark.parametrize("name", list(ROUND_NV))
@pytest.mark.parametrize("field", FIELDS)
def test_sumcheck_round_against_the_model(domains, torch_, field, name):
    """plain from nv = 1 and fused from nv = 2 to 13 with tiles of 16 pairs, so that one, two and three reduction levels are reached;
    the folded tables of the fused call are byte-equal to mle_fix_variables with one value; host and device pointers agree"""
    torch = torch_
    dom = domains(field, 4, 4)
    rng = random.Random(0x5C)
    levels = set()
    for nv in ROUND_NV[name]:
        c = mc.RoundCase(field, name, nv, rng)
        montgomery = nv % 2 == 0
        tabs = [dev(torch, mc.raw_bytes(t)) for t in c.tables]
        want, _ = c.expected(not montgomery, False)
        got = dom.sumcheck_round(tabs, c.terms(), montgomery=montgomery)
        levels.add(dom.query("sumcheck_levels"))
        assert got == want, (nv, "plain")
        if nv <= 6:
            assert dom.sumcheck_round([mc.raw_bytes(t) for t in c.tables], c.terms(), montgomery=montgomery) == want, (nv, "plain, host")
        if nv < 2:
            continue
        rp = nc.decode(field, mc.raw_bytes([c.r_prev]), not montgomery)[0]
        want, wfold = c.expected(not montgomery, True)
        got, folded = dom.sumcheck_round(tabs, c.terms(), r_prev=rp, montgomery=montgomery)
        levels.add(dom.query("sumcheck_levels"))
        assert got == want, (nv, "fused")
        for i in range(c.m):
            assert raw_of(folded[i]) == wfold[i], (nv, i)
            assert raw_of(folded[i]) == raw_of(dom.mle_fix_variables(tabs[i], [rp], montgomery=montgomery)), (nv, i)
        if nv <= 6:
            got, folded = dom.sumcheck_round([mc.raw_bytes(t) for t in c.tables], c.terms(), r_prev=rp, montgomery=montgomery)
            assert got == want and [raw_of(f) for f in folded] == wfold, (nv, "fused, host")
    assert levels == {1, 2, 3}, levels


def test_the_results_do_not_depend_on_the_tile(domains, torch_):
    torch = torch_
    rng = random.Random(0x71)
    c = mc.RoundCase("bls12_381", "hyperplonk", 12, rng)
    tabs = [dev(torch, mc.raw_bytes(t)) for t in c.tables]
    seen = []
    for tile_log in (4, 7, 10):
        dom = domains("bls12_381", 4, tile_log)
        ev, folded = dom.sumcheck_round(tabs, c.terms(), r_prev=5)
        seen.append((ev, [raw_of(f) for f in folded], raw_of(dom.mle_fix_variables(tabs[0], [3] * 12))))
    assert seen[0] == seen[1] == seen[2]


# ---- a whole proof -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_sumcheck_prove_is_accepted_and_a_tampered_table_rejected(domains, torch_, field):
    """nv = 12, vanilla HyperPlonk's list, challenges from a seeded hash of the round evaluations: P_0(0) + P_0(1) is the model's sum
    over the cube, P_i(r_i) = P_{i+1}(0) + P_{i+1}(1) by interpolation, the last value is sum_j c_j prod_k f_k(r) -- with f_k(r) as
    returned and as mle_evaluate gives them on the untouched inputs --; a table with one element changed is rejected against the
    unchanged claim"""
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 4)
    rng = random.Random(0x9A0F)
    nv = 12
    m, terms = mc.term_lists(field, rng)["hyperplonk"]
    vals = [[rng.randrange(r) for _ in range(1 << nv)] for _ in range(m)]
    tabs = [dev(torch, nc.encode(field, t, False)) for t in vals]
    before = [raw_of(t) for t in tabs]
    claim = mc.hypercube_sum(r, vals, terms)
    challenge = mc.hash_challenge(r, 0x5EED)
    rounds, point, finals = dom.sumcheck_prove(tabs, terms, challenge)
    assert [raw_of(t) for t in tabs] == before                                  # the caller's tables are not modified
    assert len(rounds) == nv and all(len(ev) == mc.degree(terms) + 1 for ev in rounds)
    assert point == [challenge(i, ev) for i, ev in enumerate(rounds)]
    assert mc.verify(r, claim, rounds, point, finals, terms) == []
    assert finals == [mc.evaluate(r, t, point) for t in vals]
    assert finals == [dom.mle_evaluate(t, point) for t in tabs]
    assert mc.verify(r, claim + 1, rounds, point, finals, terms) != []
    # host bytes give the same transcript (a smaller table: the host path stages every round)
    small = [t[:1 << 6] for t in vals]
    a = dom.sumcheck_prove([dev(torch, nc.encode(field, t, False)) for t in small], terms, challenge)
    b = dom.sumcheck_prove([nc.encode(field, t, False) for t in small], terms, challenge)
    assert a == b and mc.verify(r, mc.hypercube_sum(r, small, terms), *a, terms) == []
    # one element changed
    bad = [list(t) for t in vals]
    bad[5][1234] = (bad[5][1234] + 1) % r
    rounds, point, finals = dom.sumcheck_prove([dev(torch, nc.encode(field, t, False)) for t in bad], terms, challenge)
    assert mc.verify(r, claim, rounds, point, finals, terms) != []


# ---- the stream order of flag bit 1 ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def side(torch_):
    """(stream, calibrated delay) for the late producers of this module, once.  The stream comes from torch's high-priority pool: on
    HIP torch creates a pool stream when it is first handed out and the runtime gives it the least loaded hardware queue of its
    priority, so a stream drawn here from the pool the other modules use would move every later module's side stream to another
    queue -- and tests/test_gpu_sparse.py's late_out, which synchronises the default stream with a delay already enqueued, onto the
    default stream's own.  A producer is no less late at a higher priority."""
    stream = torch_.cuda.Stream(priority=-1)
    return stream, st.Delay(torch_, stream)


def _late_call(torch, stream, delay, raws, shapes, out_shapes, call):
    """inputs and out= tensors behind ONE late producer on a side stream, which fills the outputs with OUT_POISON before it hands over
    the inputs (a result written on any other stream is overwritten afterwards): the window is open immediately before the call and
    the producer took its time; returns what `call(inputs, outs)` returned"""
    outs = [st.poisoned(torch, s) for s in out_shapes]
    views = st.late_many(torch, raws, stream, delay, fill=outs)
    ins = []
    for v, shape in zip(views, shapes):
        t = v.reshape(shape)
        t.started, t.produced = v.started, v.produced
        ins.append(t)
    made = ins + outs
    with torch.cuda.stream(stream):
        assert all(st.window_open(t.produced) for t in made), "invalid: a producer had finished before the call was made"
        got = call(ins, outs)
    stream.synchronize()
    assert st.closed(*made), "invalid: a producer took %s ms" % [st.delay_ms(t) for t in made]
    return got


def _no_poison(raw):
    rows = [raw[i:i + 32] for i in range(0, len(raw), 32)]
    assert bytes([st.POISON]) * 32 not in rows and bytes([st.OUT_POISON]) * 32 not in rows


@pytest.mark.parametrize("field", FIELDS)
def test_fix_and_eq_after_late_producers_on_a_side_stream(domains, torch_, side, field):
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 4, 4)
    rng = random.Random(0x1A7E)
    nv, k = 9, 5
    table = mc.raw_bytes(mc.raw_values(field, 1 << nv, rng))
    point = [rng.randrange(r) for _ in range(k)]
    want = nc.encode(field, mc.fix_variables(r, nc.decode(field, table, False), point), False)
    stream, delay = side
    for with_out in (False, True):
        got = _late_call(torch, stream, delay, [table], [(1 << nv, 32)], [(1 << (nv - k), 32)] if with_out else [],
                         lambda ins, outs: dom.mle_fix_variables(ins[0], point, out=outs[0] if outs else None))
        assert raw_of(got) == want
        _no_poison(raw_of(got))
    p = [rng.randrange(r) for _ in range(7)]
    got = _late_call(torch, stream, delay, [bytes(32)], [(1, 32)], [(1 << 7, 32)], lambda ins, outs: dom.eq_table(p, out=outs[0]))
    assert raw_of(got) == nc.encode(field, mc.eq_table(r, p), False)


@pytest.mark.parametrize("field", FIELDS)
def test_sumcheck_round_after_late_producers_on_a_side_stream(domains, torch_, side, field):
    torch = torch_
    dom = domains(field, 4, 4)
    rng = random.Random(0x1A7F)
    c = mc.RoundCase(field, "spartan", 9, rng)
    raws = [mc.raw_bytes(t) for t in c.tables]
    n = 1 << c.nv
    want, _ = c.expected(False, False)
    stream, delay = side
    got = _late_call(torch, stream, delay, raws, [(n, 32)] * c.m, [], lambda ins, outs: dom.sumcheck_round(ins, c.terms()))
    assert got == want
    rp = nc.decode(field, mc.raw_bytes([c.r_prev]), False)[0]
    want, wfold = c.expected(False, True)
    got, folded = _late_call(torch, stream, delay, raws, [(n, 32)] * c.m, [(n // 2, 32)] * c.m, lambda ins, outs: dom.sumcheck_round(ins, c.terms(), r_prev=rp, out=outs))
    assert got == want
    for f, w in zip(folded, wfold):
        assert raw_of(f) == w
        _no_poison(raw_of(f))


# ---- refusals on a live handle -------------------------------------------------------------------------------------------------------------

def test_refusals_on_a_live_handle(ea, domains, torch_):
    torch = torch_
    dom = domains("bls12_381", 4)
    nv = 5
    n = 1 << nv
    big = torch.zeros((4 * n, 32), dtype=torch.uint8, device="cuda")
    tabs = [big[:n], big[n:2 * n]]
    terms = [(1, [0, 1])]
    with pytest.raises(ea.MsmError, match="folded table 1 overlaps table 1"):          # the last element of the table
        dom.sumcheck_round(tabs, terms, r_prev=3, out=[big[3 * n:3 * n + n // 2], big[2 * n - 1:2 * n - 1 + n // 2]])
    with pytest.raises(ea.MsmError, match="folded table 0 overlaps folded table 1"):
        dom.sumcheck_round(tabs, terms, r_prev=3, out=[big[2 * n:2 * n + n // 2], big[2 * n + n // 2 - 1:3 * n - 1]])
    ev, folded = dom.sumcheck_round(tabs, terms, r_prev=3, out=[big[2 * n:2 * n + n // 2], big[2 * n + n // 2:3 * n]])   # side by side is fine
    assert ev == [0, 0, 0]
    with pytest.raises(ea.MsmError, match="overlaps the input"):
        dom.mle_fix_variables(big[:n], [1, 2], out=big[n - 1:n - 1 + n // 4])
    with pytest.raises(ea.MsmError, match="term 0: factor index 2"):
        dom.sumcheck_round(tabs, [(1, [0, 2])])
    with pytest.raises(ValueError, match="at most 5 factor indices"):
        dom.sumcheck_round(tabs, [(1, [0] * 6)])
    with pytest.raises(ea.MsmError, match="one variable cannot be folded"):
        dom.sumcheck_round([big[:2], big[2:4]], terms, r_prev=3)


# ---- speed -------------------------------------------------------------------------------------------------------------------------------

def speed_bound(which, nv):
    """(bound on the call / forward transform, source): 1.5 x the ratio profiles/mle.txt recorded, or 2 x the modelled ratio"""
    path = os.path.join(ROOT, "profiles", "mle.txt")
    if os.path.exists(path):
        m = re.search(r"^bls12_381 ratio %s nv = %d / forward NN 2\^20: ([0-9.]+)" % (which, nv), open(path).read(), flags=re.M)
        if m:
            return 1.5 * float(m.group(1)), "profiles/mle.txt"
    return 2 * MODEL_RATIO[which], "the model"


def test_speed_guard_against_the_transform(domains, torch_):
    """BLS12-381, device-resident random bytes, warmed up, median of 5: one fused round of Spartan's list at nv = 22 and mle_evaluate at
    nv = 24, each against the forward NN transform of 2^20 on the same handle, which this change does not touch, run in the same test
    on the same box.  Bound: 1.5 x the ratio profiles/mle.txt recorded (tools/mle_bench.py; the margin covers box-to-box spread and
    clock differences under the power limit), or 2 x the modelled ratio above without that file."""
    torch = torch_
    r = nc.modulus("bls12_381")
    dom = domains("bls12_381", 20)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED)
    z = torch.randint(0, 256, (1 << 20, 32), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((1 << 20, 32), dtype=torch.uint8, device="cuda")

    def median5(fn):
        fn()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    t_ntt = median5(lambda: dom.fft(z, out=out))
    rng = random.Random(0xBE)
    _, terms = mc.term_lists("bls12_381", rng)["spartan"]
    tabs = [torch.randint(0, 256, (1 << 22, 32), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
    folded = [torch.empty((1 << 21, 32), dtype=torch.uint8, device="cuda") for _ in range(4)]
    rp = rng.randrange(r)
    t_round = median5(lambda: dom.sumcheck_round(tabs, terms, r_prev=rp, out=folded))
    del tabs, folded
    table = torch.randint(0, 256, (1 << 24, 32), dtype=torch.uint8, device="cuda", generator=g)
    point = [rng.randrange(r) for _ in range(24)]
    t_eval = median5(lambda: dom.mle_evaluate(table, point))
    for which, nv, t in (("round", 22, t_round), ("evaluate", 24, t_eval)):
        bound, source = speed_bound(which, nv)
        print("%s nv = %d: %.3f ms, forward NN 2^20 %.3f ms, ratio %.4f, bound %.4f from %s" % (which, nv, 1e3 * t, 1e3 * t_ntt, t / t_ntt, bound, source))
        assert t / t_ntt <= bound, which
