"""GPU: batch pairings and pairing products (csrc/pairing.hpp, csrc/msm_pairing.hpp) through the Python layer.  The golden cases of
tools/gen_pairing_golden.py (the big-integer model never runs here) through host and device pointers, in both output forms and with
out=; batches that cross the block edge and groups that cross lanes and blocks, byte-equal to the host build of the same code on the same
inputs (one reference of 195 pairs, computed once; the product of a group is the product of its pairs' values); bilinearity without
the model; check; a KZG opening from the library's own calls; and the stream order of flag bit 1, pinned with late producers as
tests/test_gpu_poseidon.py pins it."""
import random

import numpy as np
import pytest

import pairing_cases as pc
import stream_cases as st

pytestmark = pytest.mark.gpu

FAMS = ("bls12_377", "bls12_381")
N_REF = 195


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def engines(ea):
    made = {f: ea.Pairing(pc.CURVE_OF[f][0]) for f in FAMS}
    yield made
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def reference(ea, built):
    """per family: 195 G1 images, 195 G2 images (a few flagged infinity, one with junk coordinates), the canonical Gt image of every
    pair from the HOST build of pairing.hpp, and those values as model elements"""
    out = {}
    for fam in FAMS:
        F = pc.FAMILIES[fam]
        g1 = ea.generate_points(N_REF, distinct=N_REF, seed=0x5041 + len(fam), curve=pc.CURVE_OF[fam][0]).copy()
        g2 = ea.generate_points(N_REF, distinct=N_REF, seed=0x5042 + len(fam), curve=pc.CURVE_OF[fam][1]).copy()
        for i in (0, 64, 129):
            g1[i, 96] = 1
        g2[65, 192] = 1
        g2[194, :192] = 0xC3
        g2[194, 192] = 1
        ht = pc.hosttest()
        ht.ht_reset_checks()
        ec = pc.host_pairing(F, g1.tobytes(), g2.tobytes(), canonical=True)
        em = pc.host_pairing(F, g1[:8].tobytes(), g2[:8].tobytes())
        assert ht.ht_check_failures() == 0
        imgs = [ec[576 * i:576 * i + 576] for i in range(N_REF)]
        out[fam] = (g1, g2, imgs, [pc.gt_from_image(F, e, True) for e in imgs], em)
    return out


def dev(torch, raw, shape):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda().reshape(shape)


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "is_cuda") else np.asarray(t).tobytes()


def products(F, vals, group):
    out = []
    for j in range(0, len(vals), group):
        acc = pc.f12_one()
        for v in vals[j:j + group]:
            acc = pc.f12_mul(F, acc, v)
        out.append(pc.gt_image(F, acc, True))
    return b"".join(out)


@pytest.mark.parametrize("fam", FAMS)
def test_golden_cases_host_and_device_pointers_both_forms(engines, torch_, fam):
    F = pc.FAMILIES[fam]
    h = engines[fam]
    g1, g2, em, ec = pc.load_golden(F)
    a, b, n = b"".join(g1), b"".join(g2), len(g1)
    got = h.pairing(a, b)
    assert got.shape == (n, 576) and got.dtype == np.uint8 and got.tobytes() == b"".join(em)
    assert h.pairing(np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8), canonical=True).tobytes() == b"".join(ec)
    ta, tb = dev(torch_, a, (n, 104)), dev(torch_, b, (n, 200))
    d = h.pairing(ta, tb)
    assert d.is_cuda and tuple(d.shape) == (n, 576) and raw_of(d) == b"".join(em)
    out = torch_.full((n, 576), 0x77, dtype=torch_.uint8, device="cuda")
    assert h.pairing(ta, tb, canonical=True, out=out) is out
    assert raw_of(out) == b"".join(ec)
    assert h.query("last_launches") == 2 and h.query("workspace_bytes") > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("fam", FAMS)
def test_batches_across_the_block_edge_equal_the_host_build(engines, reference, torch_, fam, n):
    g1, g2, imgs, _, em = reference[fam]
    h = engines[fam]
    got = h.pairing(dev(torch_, g1[:n].tobytes(), (n, 104)), dev(torch_, g2[:n].tobytes(), (n, 200)), canonical=True)
    assert raw_of(got) == b"".join(imgs[:n])
    if n == 65:
        assert h.pairing(g1[:8], g2[:8]).tobytes() == em                     # the Montgomery form, host pointers


@pytest.mark.parametrize("n,group", [(130, 2), (130, 65), (130, 130), (195, 3), (195, 65), (195, 195)])
@pytest.mark.parametrize("fam", FAMS)
def test_groups_across_lanes_and_blocks_equal_the_host_build(engines, reference, torch_, fam, n, group):
    F = pc.FAMILIES[fam]
    g1, g2, _, vals, _ = reference[fam]
    h = engines[fam]
    want = products(F, vals[:n], group)
    got = h.pairing(dev(torch_, g1[:n].tobytes(), (n, 104)), dev(torch_, g2[:n].tobytes(), (n, 200)), group=group, canonical=True)
    assert tuple(got.shape) == (n // group, 576) and raw_of(got) == want
    if group == n:
        assert h.product_of_pairings(g1[:n], g2[:n], canonical=True) == want
        parts = group                                                          # one item per pair, then the tree of fan-in 8
        levels = 0
        while 8 ** levels < parts:
            levels += 1
        assert h.query("last_launches") == 2 + levels


@pytest.mark.parametrize("fam", FAMS)
def test_bilinearity_without_the_model(ea, engines, fam):
    F = pc.FAMILIES[fam]
    c1, c2 = pc.CURVE_OF[fam]
    rng = random.Random("gpu bilinear " + fam)
    n = 64
    P = ea.generate_points(n, distinct=n, seed=77, curve=c1)
    Q = ea.generate_points(n, distinct=n, seed=78, curve=c2)
    a = [rng.randrange(1 << 252, F.r) for _ in range(n)]
    b = [rng.randrange(1 << 252, F.r) for _ in range(n)]
    sc = lambda v: b"".join((x % F.r).to_bytes(32, "little") for x in v)
    h = engines[fam]
    left = h.pairing(ea.mul_points(P, sc(a), curve=c1), ea.mul_points(Q, sc(b), curve=c2))
    right = h.pairing(ea.mul_points(P, sc([x * y for x, y in zip(a, b)]), curve=c1), Q)
    assert left.tobytes() == right.tobytes()
    one = pc.gt_image(F, pc.f12_one())
    assert all(left[i].tobytes() != one for i in range(n))


@pytest.mark.parametrize("fam", FAMS)
def test_check(engines, torch_, fam):
    F = pc.FAMILIES[fam]
    h = engines[fam]
    g1, g2, _, _ = pc.load_golden(F)
    # cases 1..3 and their negations 15..17: (P, Q), (-P, Q)
    a = b"".join(g1[i] + g1[14 + i] for i in (1, 2, 3))
    b = b"".join(g2[i] + g2[14 + i] for i in (1, 2, 3))
    ok = h.check(a, b, group=2)
    assert ok.dtype == bool and ok.tolist() == [True, True, True]
    assert h.check(a, b) is True
    assert h.check(a, b, group=1).tolist() == [False] * 6
    d = h.check(dev(torch_, a, (6, 104)), dev(torch_, b, (6, 200)), group=2)
    assert d.is_cuda and d.cpu().tolist() == [True, True, True]
    # one coordinate of one pair replaced by another subgroup point's
    wrong = bytearray(b)
    wrong[200 * 3:200 * 3 + 200] = g2[5]
    assert h.check(a, bytes(wrong), group=2).tolist() == [True, False, True]
    assert h.check(a, bytes(wrong)) is False
    assert h.check(dev(torch_, a, (6, 104)), dev(torch_, bytes(wrong), (6, 200))) is False


def _affine_of_projective(F, raw):
    """arkworks' Jacobian Projective<G1> image (X, Y, Z in Montgomery form) as an affine point of the model"""
    rinv = pow(pc.R384, -1, F.p)
    X, Y, Z = (int.from_bytes(raw[48 * i:48 * i + 48], "little") * rinv % F.p for i in range(3))
    if Z == 0:
        return None
    zi = pow(Z, -1, F.p)
    return (X * zi * zi % F.p, Y * zi * zi * zi % F.p)


@pytest.mark.parametrize("fam", FAMS)
def test_a_kzg_opening_from_the_library_s_own_calls(ea, engines, fam):
    F = pc.FAMILIES[fam]
    c1, c2 = pc.CURVE_OF[fam]
    rng = random.Random("kzg " + fam)
    n = 16
    tau, z = rng.randrange(2, F.r), rng.randrange(2, F.r)
    sc = lambda v: b"".join((x % F.r).to_bytes(32, "little") for x in v)
    G, H = pc.g1_image(F, F.g1), pc.g2_image(F, F.g2)
    srs = ea.mul_points(G * n, sc([pow(tau, i, F.r) for i in range(n)]), curve=c1)
    coeffs = [rng.randrange(F.r) for _ in range(n)]
    ctx = ea.MultiScalarMultContext(c1)
    dom = ea.Radix2EvaluationDomain(n, c1)
    try:
        ctx.set_bases(srs)
        C = _affine_of_projective(F, ctx.run(sc(coeffs))[0])
        q, v = dom.divide_by_linear(sc(coeffs), z, montgomery=False)
        assert v == sum(c * pow(z, i, F.r) for i, c in enumerate(coeffs)) % F.r
        W = _affine_of_projective(F, ctx.run(bytes(q) + bytes(32))[0])
    finally:
        ctx.close()
        dom.close()
    tH = ea.mul_points(H, sc([tau - z]), curve=c2)
    tH = tH if isinstance(tH, bytes) else np.asarray(tH).tobytes()
    h = engines[fam]
    for value, want in ((v, True), (v + 1, False)):
        lhs = pc.g1_add(F, C, pc.g1_neg(F, pc.g1_mul(F, F.g1, value)))        # C - v G
        a = pc.g1_image(F, lhs) + pc.g1_image(F, pc.g1_neg(F, W))
        assert h.check(a, H + tH) is want, value


@pytest.fixture(scope="module")
def side(torch_):
    """(stream, calibrated delay) for the late producers of this module, once; the stream comes from torch's high-priority pool, for the
    reason tests/test_gpu_poseidon.py gives"""
    stream = torch_.cuda.Stream(priority=-1)
    return stream, st.Delay(torch_, stream)


@pytest.mark.parametrize("fam", FAMS)
def test_pairing_after_late_producers_on_a_side_stream(engines, reference, torch_, side, fam):
    """both inputs and the out= tensor behind ONE late producer on a side stream, which fills the output with OUT_POISON before it hands
    over the inputs: a result written on any other stream is overwritten afterwards"""
    g1, g2, imgs, _, _ = reference[fam]
    h = engines[fam]
    stream, delay = side
    n = 70
    out = st.poisoned(torch_, (n, 576))
    ta, tb = st.late_many(torch_, [g1[:n].tobytes(), g2[:n].tobytes()], stream, delay, fill=[out])
    with torch_.cuda.stream(stream):
        assert st.window_open(ta.produced) and st.window_open(out.produced), "invalid: the producer had finished before the call was made"
        got = h.pairing(ta, tb, canonical=True, out=out)
    stream.synchronize()
    assert st.closed(ta, out), "invalid: the producer took %s ms" % st.delay_ms(ta)
    assert got is out and raw_of(out) == b"".join(imgs[:n])
    # and check, with its one byte per group
    ok = st.poisoned(torch_, (n,))
    ta, tb = st.late_many(torch_, [g1[:n].tobytes(), g2[:n].tobytes()], stream, delay, fill=[ok])
    with torch_.cuda.stream(stream):
        assert st.window_open(ta.produced)
        res = h.check(ta, tb, group=1, out=ok)
    stream.synchronize()
    assert st.closed(ta, ok)
    one = pc.gt_image(pc.FAMILIES[fam], pc.f12_one(), True)
    assert res.cpu().tolist() == [imgs[i] == one for i in range(n)]
