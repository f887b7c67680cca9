"""CPU: the identities the soundness argument of csrc/check_points.hpp rests on, re-derived with Python integers for both curve
families, and the generated constants against the arkworks literals (tests/golden/subgroup_constants.json)."""
import json
import math
import os
import re
import subprocess
import sys

import pytest

import check_cases as cc  # noqa: F401  (puts tools/ and oracle/ on the path)
import pymodel as pm
import subgroup_consts as sc
from conftest import ROOT

FAMILIES = ("bls12_377", "bls12_381")


@pytest.fixture(scope="module")
def consts():
    return {f: sc.derive(f) for f in FAMILIES}


@pytest.mark.parametrize("fam", FAMILIES)
def test_orders_and_cofactors(fam, consts):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "constants.json")))
    d = consts[fam]
    u, p, r = d["u"], d["p"], d["r"]
    h1, h2 = sc.cofactors(fam)
    assert r == u ** 4 - u ** 2 + 1
    assert p - u == h1 * r                                   # #E(Fp) = p + 1 - t with t = u + 1
    assert u * u - (u + 1) * u + p == h1 * r                 # deg(psi - [u])
    assert h2 == int(golden[fam + "_g2"]["COFACTOR"])
    assert math.gcd(h1, h2) == 1 and math.gcd(h2, r) == 1
    assert (-u * u) ** 2 + (-u * u) + 1 == r                 # -u^2 is a root of X^2 + X + 1 mod r
    assert bin(abs(u)).count("1") == (7 if fam == "bls12_377" else 6) and abs(u).bit_length() == 64


@pytest.mark.parametrize("fam", FAMILIES)
def test_endomorphisms_on_the_generators(fam, consts):
    d = consts[fam]
    u, g1, g2, _ = sc.FAMILIES[fam]
    p = d["p"]
    beta = d["beta"]
    assert pow(beta, 3, p) == 1 and beta != 1
    G = g1.generator()
    assert sc.phi(g1, beta, G) == g1.neg(g1.mul(u * u, G))
    # negative control: the other cube root of unity rejects the generator
    other = d["beta_other"]
    assert pow(other, 3, p) == 1 and other not in (1, beta)
    assert not sc.g1_test(g1, u, other, G)
    px = pm.Fp2(d["psi_x"][0], d["psi_x"][1], p, g2.nonresidue % p)
    py = pm.Fp2(d["psi_y"][0], d["psi_y"][1], p, g2.nonresidue % p)
    G2 = g2.generator()
    assert sc.psi(g2, px, py, G2) == sc.mul_signed(g2, u, G2)
    assert g2.on_curve(sc.psi(g2, px, py, G2))
    # the tests reject a point off the subgroup and accept a random subgroup point
    Q1 = cc.curve_point_from_x(g1, 1000)
    assert g1.mul(g1.r, Q1) is not None and not sc.g1_test(g1, u, beta, Q1)
    Q2 = cc.curve_point_from_x(g2, 1000)
    assert g2.mul(g2.r, Q2) is not None and not sc.g2_test(g2, u, px, py, Q2)
    assert sc.g1_test(g1, u, beta, g1.mul(0xDEADBEEF12345, G)) and sc.g2_test(g2, u, px, py, g2.mul(0xDEADBEEF12345, G2))


def test_bls12_381_constants_equal_the_reference_literals(consts):
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "subgroup_constants.json")))["bls12_381"]
    d = consts["bls12_381"]
    assert d["beta"] == int(ref["BETA"])
    assert d["psi_x"] == tuple(int(v) for v in ref["PSI_X"])
    assert d["psi_y"] == tuple(int(v) for v in ref["PSI_Y"])


def test_field_consts_inc_is_what_the_generator_prints():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_field_consts.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(os.path.join(ROOT, "2022-entries_amd", "csrc", "field_consts.inc")).read()
    R = 1 << 392
    for fam, struct in (("bls12_377", "Bls12_377_Sub"), ("bls12_381", "Bls12_381_Sub")):
        d = sc.derive(fam)
        body = out[out.index("struct " + struct):]
        m = re.search(r"BETA\[14\] = \{([^}]*)\}", body)
        limbs = [int(v.strip().rstrip("u"), 16) for v in m.group(1).split(",")]
        assert sum(v << (28 * i) for i, v in enumerate(limbs)) == d["beta"] * R % d["p"]
