"""CPU: the big-integer pairing model of tests/pairing_cases.py against the definition.  The addition chain of bls12.rs'
final_exponentiation, evaluated in integers, is 3 (p^4 - p^2 + 1) / r modulo Phi_12(p) for both parameters x; e(G1, G2) is not one and
has order r; e(a P, b Q) = e(P, Q)^(a b) for full-width a, b; e(P, Q) e(-P, Q) = 1; the golden files of tools/gen_pairing_golden.py
regenerate byte for byte.  (The reference tree records no Gt value for either curve, so the model is pinned by these laws alone.)"""
import os
import random

import pytest

import pairing_cases as pc

FAMS = sorted(pc.FAMILIES)


@pytest.fixture(scope="module")
def e_gen():
    return {n: pc.pairing(F, F.g1, F.g2) for n, F in pc.FAMILIES.items()}


@pytest.mark.parametrize("fam", FAMS)
def test_the_chain_of_the_reference_computes_the_cube_of_the_reduced_power(fam):
    F = pc.FAMILIES[fam]
    p, r, x = F.p, F.r, F.x
    phi = p ** 4 - p ** 2 + 1
    assert phi % r == 0 and r == x ** 4 - x ** 2 + 1
    # exponents of r = f^((p^6 - 1)(p^2 + 1)) through bls12.rs final_exponentiation; conjugation is -1 there, exp_by_x is x (with its sign)
    y0 = -2
    y5 = x
    y1 = 2 * y5
    y3 = y0 + y5
    y0 = x * y3
    y2 = x * y0
    y4 = x * y2
    y4 += y1
    y1 = x * y4
    y3 = -y3
    y1 += y3
    y1 += 1
    y3 = -1
    y0 += 1
    y0 *= p ** 3
    y4 += y3
    y4 *= p
    y5 += y2
    y5 *= p ** 2
    y5 += y0 + y4 + y1
    assert (y5 - 3 * (phi // r)) % phi == 0
    assert (y5 - (phi // r)) % phi != 0
    assert F.final_power == 3 * (p ** 6 - 1) * (p ** 2 + 1) * (phi // r)


@pytest.mark.parametrize("fam", FAMS)
def test_the_generators_pair_to_an_element_of_order_r(fam, e_gen):
    F = pc.FAMILIES[fam]
    e = e_gen[fam]
    assert e != pc.f12_one()
    assert pc.f12_pow(F, e, F.r) == pc.f12_one()
    assert pc.f12_mul(F, e, pc.f12_inv(F, e)) == pc.f12_one()
    assert pc.gt_from_image(F, pc.gt_image(F, e)) == e and pc.gt_from_image(F, pc.gt_image(F, e, True), True) == e


@pytest.mark.parametrize("fam", FAMS)
def test_bilinearity_with_full_width_scalars(fam, e_gen):
    F = pc.FAMILIES[fam]
    rng = random.Random("bilinear " + fam)
    a, b = rng.randrange(1 << 252, F.r), rng.randrange(1 << 252, F.r)
    P, Q = pc.g1_mul(F, F.g1, a), pc.g2_mul(F, F.g2, b)
    e = pc.pairing(F, P, Q)
    assert e == pc.f12_pow(F, e_gen[fam], a * b % F.r)
    assert pc.f12_mul(F, e, pc.pairing(F, pc.g1_neg(F, P), Q)) == pc.f12_one()
    assert pc.pairing_product(F, [(P, Q), (pc.g1_neg(F, P), Q)]) == pc.f12_one()
    assert pc.pairing(F, None, Q) == pc.f12_one() and pc.pairing(F, P, None) == pc.f12_one()


@pytest.mark.parametrize("fam", FAMS)
def test_the_golden_file_regenerates_byte_for_byte(fam):
    F = pc.FAMILIES[fam]
    assert os.path.getsize(pc.golden_path(F)) < 64 << 10
    assert open(pc.golden_path(F), "rb").read() == pc.golden_bytes(F)
    g1, g2, em, ec = pc.load_golden(F)
    assert len(g1) == 24
    one_m, one_c = pc.gt_image(F, pc.f12_one()), pc.gt_image(F, pc.f12_one(), True)
    assert sum(e == one_m for e in em) == 6 and sum(e == one_c for e in ec) == 6     # the six pairs with an infinity
