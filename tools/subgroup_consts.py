"""Constants of the subgroup checks (csrc/check_points.hpp), DERIVED per curve family and pinned by identities on the generators.

  u       the BLS parameter (ARKC bls12_377/src/curves/mod.rs:17-19, bls12_381/src/curves/mod.rs)
  beta    the primitive cube root of unity in Fq with  phi(G) = (beta x, y) = -[u^2] G  on the G1 generator
  psi_x, psi_y   the coefficients of  psi(x, y) = (conj(x) psi_x, conj(y) psi_y)  (untwist, Frobenius, twist) with
                 psi(G2) = [u] G2  on the G2 generator; powers of the sextic-twist non-residue xi

tools/gen_field_consts.py prints them as limb tables; tests/test_check_points_consts.py checks the identities the soundness
argument of check_points.hpp rests on and compares BLS12-381's values with the arkworks literals.
Importing this module prints nothing.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import pymodel as pm  # noqa: E402

# family: (u, G1 model, G2 model, xi = the Fq6 non-residue the twist divides / multiplies b by, as (c0, c1))
FAMILIES = {
    "bls12_377": (0x8508c00000000001, pm.BLS12_377_G1, pm.BLS12_377_G2, (0, 1)),
    "bls12_381": (-0xd201000000010000, pm.BLS12_381_G1, pm.BLS12_381_G2, (1, 1)),
}


def fp2_pow(a, e):
    r = pm.Fp2(1, 0, a.p, a.nr)
    while e:
        if e & 1:
            r = r * a
        a = a * a
        e >>= 1
    return r


def cube_roots_of_unity(p):
    """The two primitive cube roots of unity of Fp: g^((p-1)/3) for the smallest g that is not a cube, and its square."""
    assert p % 3 == 1
    g = 2
    while pow(g, (p - 1) // 3, p) == 1:
        g += 1
    c = pow(g, (p - 1) // 3, p)
    assert c != 1 and pow(c, 3, p) == 1
    return c, c * c % p


def mul_signed(curve, k, P):
    return curve.mul(k, P) if k >= 0 else curve.neg(curve.mul(-k, P))


def phi(curve, beta, P):
    return (P[0] * beta % curve.p, P[1])


def conj(v):
    return pm.Fp2(v.c0, -v.c1, v.p, v.nr)


def psi(curve, px, py, P):
    return (conj(P[0]) * px, conj(P[1]) * py)


def g1_test(curve, u, beta, P):
    """phi(P) == -[u^2] P   (P affine, not infinity)"""
    return phi(curve, beta, P) == curve.neg(curve.mul(u * u, P))


def g2_test(curve, u, px, py, P):
    """psi(P) == [u] P"""
    return psi(curve, px, py, P) == mul_signed(curve, u, P)


def derive(family):
    u, g1, g2, xi = FAMILIES[family]
    p, r = g1.p, g1.r
    roots = cube_roots_of_unity(p)
    good = [b for b in roots if g1_test(g1, u, b, g1.generator())]
    assert len(good) == 1, "exactly one cube root of unity has the eigenvalue -u^2 on G1"
    beta = good[0]
    x = pm.Fp2(xi[0], xi[1], p, g2.nonresidue % p)
    cx, cy = fp2_pow(x, (p - 1) // 3), fp2_pow(x, (p - 1) // 2)
    cands = [(cx, cy), (cx.inv(), cy.inv())]   # D-type twist: the powers themselves; M-type: their inverses
    goodp = [c for c in cands if g2_test(g2, u, c[0], c[1], g2.generator())]
    assert len(goodp) == 1, "exactly one of xi^e, xi^-e maps the G2 generator to [u] G2"
    px, py = goodp[0]
    return {"u": u, "p": p, "r": r, "beta": beta, "beta_other": [b for b in roots if b != beta][0],
            "psi_x": (px.c0, px.c1), "psi_y": (py.c0, py.c1), "b_g1": g1.b % p, "b_g2": (g2.b[0] % p, g2.b[1] % p)}


def cofactors(family):
    """(h1, h2) from the parameter alone: #E(Fp) = h1 r, #E'(Fp2) = h2 r."""
    u = FAMILIES[family][0]
    h1, rem1 = divmod((u - 1) ** 2, 3)
    h2, rem2 = divmod(u ** 8 - 4 * u ** 7 + 5 * u ** 6 - 4 * u ** 4 + 6 * u ** 3 - 4 * u ** 2 - 4 * u + 13, 9)
    assert rem1 == 0 and rem2 == 0
    return h1, h2
