"""GPU: the exact work and staging bytes every family of Fr-vector calls reports after host-pointer calls, and host against device
pointers bit for bit (csrc/fr_stage.hpp and the glue of msm_poly / msm_scan / msm_quot / msm_mle / msm_sparse / msm_poseidon).

The other tests bound these queries from below or compare them with each other; here seventeen calls run once each with host pointers,
in a fixed order, on a domain of 2^10 per field, and after each the seven byte queries must EQUAL tests/golden/stage_bytes.json, which
was recorded by `measure` below at the commit before the staging helper existed (allocation sizes: no tolerance).  The same calls then
run on device pointers; the three calls whose host path runs in place inside the staging buffer (batch inversion, the element-wise
operations, the division by the vanishing polynomial) run there both with out apart and with out == in."""
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CURVES = ("bls12_377_g1", "bls12_381_g1")
DOMAIN_QUERIES = ("work_bytes", "poly_work_bytes", "scan_work_bytes", "quotient_work_bytes", "mle_work_bytes")
QUERIES = DOMAIN_QUERIES + ("sparse.work_bytes", "poseidon.work_bytes")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage_bytes.json")
N = 1000
ALIASED = ("batch_inversion", "mul_sub", "scale", "divide_by_vanishing_poly_on_coset")


class Session:
    """the handles and the inputs of one field; `calls` are the seventeen calls in the order of the recorded table"""

    def __init__(self, ea, curve):
        self.dom = dom = ea.Radix2EvaluationDomain(1 << 10, curve)
        rng = random.Random(0x57A6E)
        p = self.p = dom.modulus
        self.el = lambda: rng.randrange(1, p)
        self.vec = lambda *shape: np.frombuffer(b"".join(self.el().to_bytes(32, "little") for _ in range(int(np.prod(shape)))),
                                                dtype=np.uint8).reshape(*shape, 32).copy()
        self.a, self.b, self.c = self.vec(N), self.vec(N), self.vec(N)
        self.wires, self.sigmas, self.z = self.vec(3, dom.size), self.vec(3, dom.size), self.vec(dom.size)
        self.cols = [self.vec(N), self.vec(7), np.zeros((0, 32), dtype=np.uint8)]
        self.tables = [self.vec(256), self.vec(256)]
        self.sc = [self.el() for _ in range(16)]
        rows = [[(self.el(), c) for c in sorted(rng.sample(range(70), rng.randrange(0, 6)))] for _ in range(50)]
        self.matrix = ea.SparseMatrix.from_rows(dom, rows, 70)
        self.zvec = self.vec(70)
        par = None if curve.startswith("bls12_377") else dict(alpha=17, full_rounds=8, partial_rounds=31)
        self.hasher = ea.Poseidon(dom, 2, parameters=par, domain="AleoPoseidon2")
        self.inputs, self.leaves = self.vec(33, 3), self.vec(5, 2)

    def close(self):
        self.hasher.close()
        self.matrix.close()
        self.dom.close()

    def bytes_now(self):
        return [self.dom.query(q) for q in DOMAIN_QUERIES] + [self.matrix.query("work_bytes"), self.hasher.query("work_bytes")]

    def calls(self, put=lambda a: a, device=False, alias=False):
        """(name, thunk) per call; `put` moves an input to where the call reads it, `alias` asks the ALIASED calls for out == in"""
        d, s = self.dom, self.sc

        def out(t):
            return dict(out=t) if alias else {}

        def inv():
            v = put(self.a)
            return d.batch_inversion(v, **out(v))

        def mul_sub():
            a = put(self.a)
            return d.mul_sub(a, put(self.b), put(self.c), **out(a))

        def scale():
            a = put(self.a)
            return d.scale(a, s[0], **out(a))

        def vanishing():
            v = put(self.a)
            return d.divide_by_vanishing_poly_on_coset(v, **out(v))

        return [
            ("batch_inversion", inv),
            ("mul_sub", mul_sub),
            ("scale", scale),
            ("evaluate", lambda: d.evaluate(put(self.a), s[1])),
            ("divide_by_linear", lambda: d.divide_by_linear(put(self.a), s[2])),
            ("evaluate_all_lagrange_coefficients", lambda: d.evaluate_all_lagrange_coefficients(s[3], device=device)),
            ("divide_by_vanishing_poly_on_coset", vanishing),
            ("prefix_product", lambda: d.prefix_product(put(self.b))),
            ("permutation_product", lambda: d.permutation_product(put(self.wires), put(self.sigmas), s[4], s[5], s[6:9])),
            ("plonk_quotient", lambda: d.plonk_quotient(put(self.wires), put(self.sigmas), put(self.z), s[9], s[4], s[5], s[6:9], 1 << 8)),
            ("linear_combination", lambda: d.linear_combination([put(c) for c in self.cols], s[10:13])),
            ("mle_fix_variables", lambda: d.mle_fix_variables(put(self.tables[0]), s[13:16])),
            ("eq_table", lambda: d.eq_table(s[1:9], device=device)),
            ("sumcheck_round", lambda: d.sumcheck_round([put(t) for t in self.tables], [(s[0], [0, 1]), (s[1], [0])], r_prev=s[2])),
            ("sparse_apply", lambda: self.matrix.apply(put(self.zvec))),
            ("poseidon_sponge", lambda: self.hasher.sponge(put(self.inputs), 2)),
            ("poseidon_merkle_tree", lambda: self.hasher.merkle_tree(put(self.leaves)).nodes),
        ]


def raw(x):
    """a result -- vectors, integers, tuples and lists of them -- as bytes"""
    if isinstance(x, (tuple, list)):
        return b"".join(raw(v) for v in x)
    if isinstance(x, int):
        return x.to_bytes(32, "little")
    return x.cpu().numpy().tobytes() if hasattr(x, "cpu") else x.tobytes()


def measure(ea, torch, curve):
    """(the byte table after each host-pointer call, the results on host pointers, on device pointers, on device pointers in place)"""
    s = Session(ea, curve)
    try:
        table, host = [], {}
        for name, call in s.calls():
            host[name] = raw(call())
            table.append([name, s.bytes_now()])

        def put(a):
            return torch.from_numpy(a).cuda()

        apart = {name: raw(call()) for name, call in s.calls(put, device=True)}
        inplace = {name: raw(call()) for name, call in s.calls(put, device=True, alias=True) if name in ALIASED}
        return table, host, apart, inplace
    finally:
        s.close()


@pytest.fixture(scope="module")
def measured(ea):
    import torch

    assert torch.cuda.is_available()
    return {curve: measure(ea, torch, curve) for curve in CURVES}


@pytest.mark.parametrize("curve", CURVES)
def test_bytes_after_host_pointer_calls_equal_the_record(measured, curve):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden["queries"] == list(QUERIES)
    table = measured[curve][0]
    for row in table:
        print(curve, row)
    assert len(table) == 17
    assert table == golden[curve]


@pytest.mark.parametrize("curve", CURVES)
def test_host_pointers_equal_device_pointers(measured, curve):
    _, host, apart, inplace = measured[curve]
    assert sorted(inplace) == sorted(ALIASED) and len(host) == len(apart) == 17
    for name in host:
        assert len(host[name]) > 0
        assert host[name] == apart[name], name
    for name in inplace:
        assert host[name] == inplace[name], name + " with out == in"
