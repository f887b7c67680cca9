"""GPU: whole Groth16 proofs from the library's own calls, one call's output feeding the next across subsystems -- FixedBase makes the
CRS, SparseMatrix.apply and groth16_witness_map turn one assignment into h, six MSM contexts (five on G1, one on G2) commit to it,
fold_partials and mul_points assemble A, B and C, Pairing.check verifies them -- judged by integers (tests/groth16_cases.py, itself
judged by tests/test_groth16_reference.py): the test chooses the toxic waste, so A, B and C have known discrete logs and exact expected
bytes, one one-pair multiplication of a generator by the CPU oracle each.  The verifier on the GPU is a second judgement, and it must
agree with the verifier in the exponent on every rejected proof.

What only such a chain shows: the form in which run reads what groth16_witness_map returns (the option "scalars_montgomery", in both
forms), base sets that are mostly points at infinity (b_g1_query, b_g2_query), MSMs of 1 and 3 points (the public inputs), contexts
reused for a second assignment, and one point encoding shared by FixedBase, the MSM, fold_partials, mul_points and the pairing."""
import pytest

import distinct_cases as dc
import groth16_cases as gc
import ntt_cases as nc
import pairing_cases as pc
import pymodel as pm

pytestmark = pytest.mark.gpu

CASES = gc.cases()
IDS = [c.name for c in CASES]
EXTRA = [c for c in CASES if (c.k, c.slack) == (6, 9)]                           # one case per family for the other paths to the same bytes
G1_QUERIES = ("a_query", "b_g1_query", "l_query", "h_query", "gamma_abc")
ELEMENTS = (("A", "a", 0), ("B", "b", 1), ("B1", "b", 0), ("C", "c", 0))       # (element, its log in Setup.prove, 0 = G1 / 1 = G2)


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


def dev(torch, raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda().reshape(-1, 32)


def rows(v, lo, hi):
    """elements lo .. hi of a vector of 32-byte elements: bytes, a NumPy array or a tensor of shape (n, 32)"""
    return v[32 * lo:32 * hi] if isinstance(v, (bytes, bytearray)) else v[lo:hi]


def affine(curve, img):
    return dc.affine_of_projective(curve, img)


def projective(curve, img):
    """an Affine image as the normalised Projective image fold_partials takes: the same coordinate bytes and a one (encoding only)"""
    return curve.encode_projective_normalized(curve.decode_affine(img))


def negated(curve, img):
    return curve.encode_affine(curve.neg(curve.decode_affine(img)))


class World:
    """one family for the whole module: the window tables of the two generators, one domain per k, one Pairing"""

    def __init__(self, ea, family):
        self.ea, self.family = ea, family
        self.names = pc.CURVE_OF[family]
        self.curves = tuple(pm.CURVES[name] for name in self.names)
        self.tables = tuple(ea.FixedBase.get_window_table(dc.generator_image(c), curve=name, expected_scalars=1 << 12)
                            for c, name in zip(self.curves, self.names))
        self.pairing = ea.Pairing(self.names[0])
        self.domains = {}

    def domain(self, k):
        if k not in self.domains:
            self.domains[k] = self.ea.Radix2EvaluationDomain(1 << k, self.names[0])
        return self.domains[k]

    def close(self):
        for h in self.tables + (self.pairing,) + tuple(self.domains.values()):
            h.close()


@pytest.fixture(scope="module")
def worlds(ea):
    made = {}

    def get(family):
        if family not in made:
            made[family] = World(ea, family)
        return made[family]

    yield get
    for w in made.values():
        w.close()


class Prover:
    """one circuit's proving and verifying key on the device, made from the logs, and the calls of a prover and a verifier on them"""

    def __init__(self, torch, oracle, world, case, satisfied=True):
        self.torch, self.oracle, self.world, self.case = torch, oracle, world, case
        self.setup, self.inst = case.setup(satisfied), case.instance(satisfied)
        self.field, self.r = case.family, nc.modulus(case.family)
        self.dom = world.domain(case.k)
        ea, st = world.ea, self.setup
        g1, g2 = world.curves
        # ---- step 1: the CRS from its logs, one FixedBase call a group; a zero log comes back as the infinity image, nothing else does
        logs1 = {"a_query": st.a_query, "b_g1_query": st.b_query, "l_query": st.l_query, "h_query": st.h_query, "gamma_abc": st.gamma_abc,
                 "vk": [st.alpha, st.beta, st.delta, self.r - st.alpha]}
        logs2 = {"b_g2_query": st.b_query, "vk": [st.beta, st.gamma, st.delta]}
        self.crs, self.infinities = {}, {}
        for which, logs in ((0, logs1), (1, logs2)):
            curve = world.curves[which]
            flat = [x for part in logs.values() for x in part]
            out = world.tables[which].msm(dev(torch, nc.encode(self.field, flat, True)).reshape(-1))
            assert out.is_cuda and tuple(out.shape) == (len(flat), curve.affine_stride)
            host = out.cpu().numpy()
            infinity = curve.encode_affine(None)
            for i, x in enumerate(flat):
                assert (host[i].tobytes() == infinity) == (x == 0) and host[i, 2 * curve.coord_bytes] == (x == 0), (case, which, i)
            at = 0
            for name, part in logs.items():
                self.crs[(which, name)] = out[at:at + len(part)]
                self.infinities[(which, name)] = gc.zero_logs(part)
                at += len(part)
        vk1 = self.crs[(0, "vk")].cpu().numpy()
        vk2 = self.crs[(1, "vk")].cpu().numpy()
        self.alpha_g1, self.beta_g1, self.delta_g1, self.neg_alpha_g1 = (vk1[i].tobytes() for i in range(4))
        self.beta_g2, self.gamma_g2, self.delta_g2 = (vk2[i].tobytes() for i in range(3))
        want1 = dc.oracle_mul(oracle, g1, dc.generator_image(g1), logs1["vk"])
        want2 = dc.oracle_mul(oracle, g2, dc.generator_image(g2), logs2["vk"])
        assert [projective(g1, vk1[i].tobytes()) for i in range(4)] == want1, (case, "alpha, beta, delta, -alpha in G1")
        assert [projective(g2, vk2[i].tobytes()) for i in range(3)] == want2, (case, "beta, gamma, delta in G2")
        # ---- step 2: one context a query, set_bases once
        self.ctx, self.set_bases_calls = {}, 0
        for name in G1_QUERIES + ("b_g2_query",):
            which = 1 if name == "b_g2_query" else 0
            ctx = self.ctx[name] = ea.MultiScalarMultContext(world.names[which])
            ctx.set_bases(self.crs[(which, name)])
            self.set_bases_calls += 1
            assert ctx.npoints == len(self.crs[(which, name)])
        self.A = ea.SparseMatrix.from_rows(self.dom, self.inst.A, case.nvars)
        self.B = ea.SparseMatrix.from_rows(self.dom, self.inst.B, case.nvars)

    def close(self):
        for h in tuple(self.ctx.values()) + (self.A, self.B):
            h.close()

    def z_of(self, inst, montgomery=True):
        return dev(self.torch, nc.encode(self.field, inst.z, not montgomery))

    def mul(self, which, point, k):
        """k * (one Affine image) as a normalised Projective image, by mul_points on a context of that curve"""
        ctx = self.ctx["b_g2_query" if which else "a_query"]
        out = ctx.mul_points(point, int(k).to_bytes(32, "little"), projective=True)
        assert isinstance(out, bytes) and len(out) == self.world.curves[which].projective_bytes
        return out

    def fold(self, which, parts):
        return self.world.ea.fold_partials(parts, curve=self.world.names[which])

    def prove(self, z, r_, s_, montgomery=True, bump=None):
        """step 3.  z: the assignment in the form `montgomery` says, a GPU tensor (nvars, 32) or host bytes; nothing else is uploaded.
        bump: a coefficient of h to increment before its MSM.  Returns the images of A, B, B1, C and h."""
        case, torch = self.case, self.torch
        ni, size = case.num_inputs, case.size
        g1, g2 = self.world.curves
        for ctx in self.ctx.values():
            ctx.set_option("scalars_montgomery", 1 if montgomery else 0)
        h = self.dom.groth16_witness_map(self.A, self.B, z, ni, montgomery=montgomery)
        assert tuple(h.shape) == (size, 32) and (isinstance(z, (bytes, bytearray)) or h.is_cuda)
        assert not bytes(bytearray(h[size - 1].tolist())).strip(b"\0"), "h has degree size - 2: its last coefficient is 0"
        if bump is not None:
            e = torch.zeros_like(h)
            e[bump] = dev(torch, nc.encode(self.field, [1], not montgomery))[0]
            h = self.dom.add(h, e, montgomery=montgomery)
        run = lambda name, scalars: self.ctx[name].run(scalars)[0]
        out = {"h": h}
        out["A"] = self.fold(0, [projective(g1, self.alpha_g1), run("a_query", z), self.mul(0, self.delta_g1, r_)])
        out["B"] = self.fold(1, [projective(g2, self.beta_g2), run("b_g2_query", z), self.mul(1, self.delta_g2, s_)])
        out["B1"] = self.fold(0, [projective(g1, self.beta_g1), run("b_g1_query", z), self.mul(0, self.delta_g1, s_)])
        out["C"] = self.fold(0, [run("l_query", rows(z, ni, case.nvars)), run("h_query", rows(h, 0, size - 1)),
                                 self.mul(0, affine(g1, out["A"]), s_), self.mul(0, affine(g1, out["B1"]), r_),
                                 self.mul(0, self.delta_g1, -r_ * s_ % self.r)])
        return out

    def expected(self, logs):
        """the images of A, B, B1 and C from the logs of Setup.prove: one multiplication of a generator each, by the CPU oracle"""
        out = {}
        for which in (0, 1):
            curve = self.world.curves[which]
            names = [(el, log) for el, log, w in ELEMENTS if w == which]
            imgs = dc.oracle_mul(self.oracle, curve, dc.generator_image(curve), [logs[log] for _, log in names])
            out.update({el: img for (el, _), img in zip(names, imgs)})
        return out

    def assert_proof(self, got, logs, what):
        want = self.expected(logs)
        for el, log, _ in ELEMENTS:
            assert got[el] == want[el], "%s, %s: %s is not %s times the generator" % (self.case, what, el, log)

    def verify(self, proof, z_pub, montgomery=True):
        """step 5: (what Pairing.check says about e(A, B) e(-alpha G1, beta G2) e(-vk_x, gamma G2) e(-C, delta G2), the image of vk_x)"""
        g1, g2 = self.world.curves
        ctx = self.ctx["gamma_abc"]
        ctx.set_option("scalars_montgomery", 1 if montgomery else 0)
        vk_x = ctx.run(z_pub)[0]
        p = affine(g1, proof["A"]) + self.neg_alpha_g1 + negated(g1, affine(g1, vk_x)) + negated(g1, affine(g1, proof["C"]))
        q = affine(g2, proof["B"]) + self.beta_g2 + self.gamma_g2 + self.delta_g2
        ok = self.world.pairing.check(p, q, group=4)
        assert ok.shape == (1,) and ok.dtype == bool
        return bool(ok[0]), vk_x

    def public(self, z_pub):
        return dev(self.torch, nc.encode(self.field, z_pub, False))


@pytest.fixture(scope="module")
def prover(request, torch_, oracle, worlds):
    """the keys of one case on the device (the satisfied circuit's; .twin(): the unsatisfied one's), for all the tests of that case"""
    case = request.param
    made = {}

    def get(satisfied=True):
        if satisfied not in made:
            made[satisfied] = Prover(torch_, oracle, worlds(case.family), case, satisfied)
        return made[satisfied]

    p = get()
    p.twin = lambda: get(False)
    yield p
    for x in made.values():
        x.close()


per_case = pytest.mark.parametrize("prover", CASES, ids=IDS, indirect=True)
per_family = pytest.mark.parametrize("prover", EXTRA, ids=[c.name for c in EXTRA], indirect=True)


@per_case
def test_the_crs_has_the_infinities_the_logs_say(prover):
    """steps 1 and 2 (asserted row by row while the keys are made): every zero log is the infinity image and nothing else is.  Here: how
    many there are -- most of b_g1_query and b_g2_query, some of a_query, one or more of l_query, none of h_query and gamma_abc -- and
    that the subgroup check of the library counts the same."""
    case = prover.case
    inf = prover.infinities
    assert inf[(0, "b_g1_query")] == inf[(1, "b_g2_query")] > case.nvars // 2
    assert inf[(0, "a_query")] >= 2 and inf[(0, "l_query")] >= 1 and inf[(0, "h_query")] == inf[(0, "gamma_abc")] == 0
    for name, ctx in prover.ctx.items():
        which = 1 if name == "b_g2_query" else 0
        chk = ctx.check_bases(prover.crs[(which, name)])
        assert chk.ok and chk.counts["flagged_infinity"] == inf[(which, name)], (case, name)
    assert prover.set_bases_calls == 6


@per_case
def test_the_proof_is_the_logs_times_the_generators_and_verifies(prover):
    """steps 3 to 5 for the satisfied circuit and for the unsatisfied twin, by the same calls: A, B, B1 and C byte-equal to their logs
    times the generators, vk_x too; Pairing.check accepts the one and rejects the other, as the verifier in the exponent does."""
    case = prover.case
    for p, satisfied in ((prover, True), (prover.twin(), False)):
        logs = p.setup.prove(p.inst, *case.randomizers())
        z = p.z_of(p.inst)                                                      # the one upload: the verifier reads its first rows
        proof = p.prove(z, *case.randomizers())
        p.assert_proof(proof, logs, "satisfied" if satisfied else "unsatisfied")
        ok, vk_x = p.verify(proof, rows(z, 0, case.num_inputs))
        g1 = p.world.curves[0]
        assert vk_x == dc.oracle_mul(p.oracle, g1, dc.generator_image(g1), [logs["x"]])[0], "%s: vk_x is not x times the generator" % case
        assert p.setup.verifies(logs) == satisfied
        assert ok == satisfied, "%s: Pairing.check says %s about the %s instance" % (case, ok, "satisfied" if satisfied else "unsatisfied")


@per_case
def test_a_changed_public_input_and_a_moved_h_are_rejected(prover):
    """the same proof against public inputs of which one was changed; and a proof whose h had one coefficient incremented on the device
    before its MSM, which is still the bytes the integers give for h(tau) + tau^j.  Rejected on the GPU and in the exponent."""
    case, st, inst = prover.case, prover.setup, prover.inst
    r, ni = prover.r, case.num_inputs
    logs = st.prove(inst, *case.randomizers())
    z = prover.z_of(inst)
    proof = prover.prove(z, *case.randomizers())
    for i in sorted({0, ni - 1}):
        z_pub = list(inst.z[:ni])
        z_pub[i] = (z_pub[i] + 1) % r
        assert not st.verifies(logs, z_pub)
        assert prover.verify(proof, prover.public(z_pub))[0] is False, "%s: accepted with public input %d changed" % (case, i)
    assert prover.verify(proof, prover.public(inst.z[:ni]))[0] is True
    for j in (0, case.size // 2 + 1, case.size - 2):
        moved_logs = st.prove(inst, *case.randomizers(), h_shift=pow(st.tau, j, r))
        moved = prover.prove(z, *case.randomizers(), bump=j)
        prover.assert_proof(moved, moved_logs, "h[%d] + 1" % j)
        assert not st.verifies(moved_logs)
        assert prover.verify(moved, prover.public(inst.z[:ni]))[0] is False, "%s: accepted with h[%d] incremented" % (case, j)


@per_case
def test_a_second_assignment_on_the_same_keys_and_the_first_again(prover):
    """step 6: another assignment of the same circuit through the same contexts, matrices, domain and pairing handle -- nothing is made
    again, set_bases is not called again --, then the first assignment once more: its first bytes."""
    case, st = prover.case, prover.setup
    ni = case.num_inputs
    handles = [id(x) for x in list(prover.ctx.values()) + [prover.A, prover.B, prover.dom, prover.world.pairing]]
    first = prover.prove(prover.z_of(prover.inst), *case.randomizers())
    other = case.second()
    logs = st.prove(other, *case.randomizers(1))
    second = prover.prove(prover.z_of(other), *case.randomizers(1))
    prover.assert_proof(second, logs, "the second assignment")
    assert st.verifies(logs) and prover.verify(second, prover.public(other.z[:ni]))[0] is True
    if ni > 1:                                                                  # and not against the first assignment's public inputs
        assert prover.verify(second, prover.public(prover.inst.z[:ni]))[0] is False
    again = prover.prove(prover.z_of(prover.inst), *case.randomizers())
    for el, _, _ in ELEMENTS:
        assert again[el] == first[el], "%s: %s of the first assignment changed after the second" % (case, el)
    prover.assert_proof(again, st.prove(prover.inst, *case.randomizers()), "the first assignment again")
    assert prover.verify(again, prover.public(prover.inst.z[:ni]))[0] is True
    assert handles == [id(x) for x in list(prover.ctx.values()) + [prover.A, prover.B, prover.dom, prover.world.pairing]]
    assert prover.set_bases_calls == 6


@per_family
def test_plain_integers_and_host_bytes_give_the_same_proof(prover):
    """steps 7 and 8.  What groth16_witness_map returns is what run reads when the option "scalars_montgomery" says the same form as the
    call's montgomery=: arkworks images with the option on (the main path of this module), plain integers with it off -- the same
    proof bytes; so do host bytes for z in place of the device tensor (h then comes back in host memory and run takes that)."""
    case, inst = prover.case, prover.inst
    ni = case.num_inputs
    main = prover.prove(prover.z_of(inst), *case.randomizers())
    try:
        plain = prover.prove(prover.z_of(inst, montgomery=False), *case.randomizers(), montgomery=False)
        assert plain["h"].is_cuda
        assert nc.decode(prover.field, plain["h"].cpu().numpy().tobytes(), True) == nc.decode(prover.field, main["h"].cpu().numpy().tobytes(), False)
        for el, _, _ in ELEMENTS:
            assert plain[el] == main[el], "%s: %s from plain integers differs" % (case, el)
        ok, vk_x = prover.verify(plain, dev(prover.torch, nc.encode(prover.field, inst.z[:ni], True)), montgomery=False)
        assert ok is True and vk_x == prover.verify(main, prover.public(inst.z[:ni]))[1]
    finally:
        for ctx in prover.ctx.values():
            ctx.set_option("scalars_montgomery", 1)
    raw = nc.encode(prover.field, inst.z, False)
    host = prover.prove(raw, *case.randomizers())
    assert not hasattr(host["h"], "is_cuda") and host["h"].tobytes() == main["h"].cpu().numpy().tobytes()
    for el, _, _ in ELEMENTS:
        assert host[el] == main[el], "%s: %s from host bytes differs" % (case, el)
    assert prover.verify(host, raw[:32 * ni])[0] is True
    prover.assert_proof(main, prover.setup.prove(inst, *case.randomizers()), "the main path")


@per_family
def test_a_as_one_msm_over_the_concatenated_bases(prover):
    """A = alpha G + MSM(a_query, z) + r_ delta G as ONE MSM over [alpha G, a_query .., delta G] with the scalars [1, z .., r_]: the
    same bytes as the three parts folded"""
    case, torch = prover.case, prover.torch
    r_, s_ = case.randomizers()
    g1 = prover.world.curves[0]
    want = prover.prove(prover.z_of(prover.inst), r_, s_)["A"]
    bases = torch.cat([dev_image(torch, prover.alpha_g1), prover.crs[(0, "a_query")], dev_image(torch, prover.delta_g1)])
    scalars = torch.cat([dev(torch, nc.encode(prover.field, [1], False)), prover.z_of(prover.inst), dev(torch, nc.encode(prover.field, [r_], False))])
    ctx = prover.world.ea.MultiScalarMultContext(prover.world.names[0])
    try:
        ctx.set_option("scalars_montgomery", 1)
        ctx.set_bases(bases)
        assert ctx.npoints == case.nvars + 2
        got = ctx.run(scalars)[0]
    finally:
        ctx.close()
    assert got == want, "%s: A as one MSM differs from A as three parts" % case
    assert got == dc.oracle_mul(prover.oracle, g1, dc.generator_image(g1), [prover.setup.prove(prover.inst, r_, s_)["a"]])[0]


def dev_image(torch, img):
    return torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda().reshape(1, -1)
