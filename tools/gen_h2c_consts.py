#!/usr/bin/env python3
"""Generate 2022-entries_amd/csrc/h2c_consts.inc: every constant of hash-to-curve on BLS12-381 (csrc/h2c.hpp), DERIVED from the
suite parameters of RFC 9380 section 8.8 alone -- Z, A', B' of the isogenous curves E', the curve equations, p and the curve
parameter z -- with plain Python integers.  Nothing is copied from a table of isogeny coefficients.

  G1  E': y^2 = x^3 + A'x + B' over Fp is 11-isogenous to E: y^2 = x^3 + 4.  #E'(Fp) = #E(Fp) = h r with 11^2 | h: a random point
      times h r / 11 is a rational point T of order 11; <T> is the kernel.
  G2  E' over Fp2 is 3-isogenous to E: y^2 = x^3 + 4(1 + i).  The kernel abscissa is the one root in Fp2 of the 3-division
      polynomial psi_3 = 3x^4 + 6A'x^2 + 12B'x - A'^2 (found as gcd(x^q - x, psi_3)); of y_Q only the square g(x_Q) is needed.
  Velu, over the half kernel S (one of Q, -Q each): v_Q = 2(3 x_Q^2 + A'), u_Q = 4 y_Q^2,
      X(x) = x + sum_S v_Q/(x - x_Q) + u_Q/(x - x_Q)^2,  Y = y dX/dx,  codomain A* = A' - 5 sum v = 0, B* = B' - 7 sum(u + x_Q v).
  Then (x, y) -> (c^2 x, c^3 y) with c^6 = B/B*.  Of the six c exactly one reproduces Q0 and Q1 of all five recorded vectors
  (tests/golden/h2c/*_SSWU_RO_.json, which hold u); the generator fails if the number that fit is not one.
  With h = prod_S (x - x_Q) monic the map is  x_num/h^2,  y y_num/h^3  (the coefficients are those of RFC 9380 appendix E, there
  written as four polynomials).  The kernel keeps x = xn/xd projective and needs only x_num, h, y_num, homogenised.

sqrt_ratio constants (RFC 9380 appendix F.2.1): one exponentiation gamma = u v^(2^s-1) (u v^(2^(s+1)-1))^((q - 2^s - 1)/2^(s+1)) for
q = 2^s + 1 (mod 2^(s+1)) -- s = 1 for p = 3 (mod 4), s = 3 for p^2 = 9 (mod 16) -- leaves gamma^2 v / u a 2^(s-1)-th root of unity
when u/v is a square and a primitive 2^s-th root otherwise; ROOTS lists the correcting factors, squares first.

Field elements are radix-2^28 limb tables in Montgomery form (R = 2^392), one row per Fp component; exponents are plain words.
Run:  python tools/gen_h2c_consts.py > 2022-entries_amd/csrc/h2c_consts.inc
"""
import json
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL, LB = 14, 28
R = 1 << (NL * LB)
P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
Z_CURVE = -0xd201000000010000
R_ORDER = Z_CURVE ** 4 - Z_CURVE ** 2 + 1
H1 = (Z_CURVE - 1) ** 2 // 3


class Field:
    """Fp (m = 1) or Fp2 = Fp[i]/(i^2 + 1) (m = 2); elements are tuples of m integers."""

    def __init__(self, m):
        self.m, self.p, self.q = m, P, P ** m
        self.zero = (0,) * m
        self.one = (1,) + (0,) * (m - 1)

    def el(self, *c):
        return tuple(int(x) % P for x in c) + (0,) * (self.m - len(c))

    def add(self, a, b):
        return tuple((x + y) % P for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % P for x, y in zip(a, b))

    def neg(self, a):
        return tuple(-x % P for x in a)

    def mul(self, a, b):
        if self.m == 1:
            return (a[0] * b[0] % P,)
        return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)

    def sqr(self, a):
        return self.mul(a, a)

    def inv(self, a):
        if self.m == 1:
            return (pow(a[0], -1, P),)
        n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
        return (a[0] * n % P, -a[1] * n % P)

    def div(self, a, b):
        return self.mul(a, self.inv(b))

    def pow(self, a, e):
        out = self.one
        while e:
            if e & 1:
                out = self.mul(out, a)
            a = self.mul(a, a)
            e >>= 1
        return out

    def muli(self, a, k):
        return tuple(x * k % P for x in a)

    def is_square(self, a):
        return a == self.zero or self.pow(a, (self.q - 1) // 2) == self.one

    def sqrt(self, a):
        """A square root by Tonelli-Shanks over q - 1 = 2^s t; None when there is none."""
        if a == self.zero:
            return a
        if not self.is_square(a):
            return None
        s, t = 0, self.q - 1
        while t % 2 == 0:
            s, t = s + 1, t // 2
        rng = random.Random(1)
        while True:
            g = tuple(rng.randrange(P) for _ in range(self.m))
            if not self.is_square(g):
                break
        c, x, b = self.pow(g, t), self.pow(a, (t + 1) // 2), self.pow(a, t)
        while b != self.one:
            k, b2 = 0, b
            while b2 != self.one:
                b2, k = self.sqr(b2), k + 1
            f = c
            for _ in range(s - k - 1):
                f = self.sqr(f)
            x, c, s = self.mul(x, f), self.sqr(f), k
            b = self.mul(b, c)
        assert self.sqr(x) == a
        return x

    def cube_roots(self, a):
        """All three cube roots of a cube a != 0 (q = 1 mod 3)."""
        e, t = 0, self.q - 1
        while t % 3 == 0:
            e, t = e + 1, t // 3
        assert 1 <= e <= 8
        rng = random.Random(2)
        while True:
            g = tuple(rng.randrange(P) for _ in range(self.m))
            if self.pow(g, (self.q - 1) // 3) != self.one:
                break
        zeta = self.pow(g, t)                       # of order exactly 3^e
        x0 = self.pow(a, pow(3, -1, t))             # x0^3 = a * (an element of the 3-Sylow group)
        cand = x0
        for _ in range(3 ** e):
            if self.pow(cand, 3) == a:
                w = self.pow(zeta, 3 ** (e - 1))    # a primitive cube root of unity
                return [cand, self.mul(cand, w), self.mul(cand, self.sqr(w))]
            cand = self.mul(cand, zeta)
        raise ValueError("not a cube")

    def sgn0(self, a):
        """RFC 9380 section 4.1"""
        sign, zero = 0, 1
        for x in a:
            sign |= zero & (x & 1)
            zero &= int(x == 0)
        return sign


# ---- polynomials over a Field, coefficient lists from the constant term up ------------------------------------------------------
def p_trim(F, a):
    while a and a[-1] == F.zero:
        a = a[:-1]
    return a


def p_add(F, a, b):
    n = max(len(a), len(b))
    a, b = a + [F.zero] * (n - len(a)), b + [F.zero] * (n - len(b))
    return p_trim(F, [F.add(x, y) for x, y in zip(a, b)])


def p_scale(F, a, k):
    return p_trim(F, [F.mul(x, k) for x in a])


def p_sub(F, a, b):
    return p_add(F, a, p_scale(F, b, F.neg(F.one)))


def p_mul(F, a, b):
    if not a or not b:
        return []
    out = [F.zero] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = F.add(out[i + j], F.mul(x, y))
    return p_trim(F, out)


def p_mod(F, a, f):
    a = list(a)
    inv = F.inv(f[-1])
    while len(a) >= len(f):
        k = F.mul(a[-1], inv)
        off = len(a) - len(f)
        for i, c in enumerate(f):
            a[off + i] = F.sub(a[off + i], F.mul(k, c))
        a = p_trim(F, a[:-1])
    return p_trim(F, a)


def p_gcd(F, a, b):
    while b:
        a, b = b, p_mod(F, a, b)
    return p_scale(F, a, F.inv(a[-1]))


def p_deriv(F, a):
    return p_trim(F, [F.muli(c, i) for i, c in enumerate(a)][1:])


def p_eval(F, a, x):
    out = F.zero
    for c in reversed(a):
        out = F.add(F.mul(out, x), c)
    return out


# ---- curves y^2 = x^3 + A x + B, affine, None = infinity ---------------------------------------------------------------------------
def ec_add(F, A, P1, P2):
    if P1 is None:
        return P2
    if P2 is None:
        return P1
    (x1, y1), (x2, y2) = P1, P2
    if x1 == x2:
        if F.add(y1, y2) == F.zero:
            return None
        lam = F.div(F.add(F.muli(F.sqr(x1), 3), A), F.muli(y1, 2))
    else:
        lam = F.div(F.sub(y2, y1), F.sub(x2, x1))
    x3 = F.sub(F.sub(F.sqr(lam), x1), x2)
    return (x3, F.sub(F.mul(lam, F.sub(x1, x3)), y1))


def ec_mul(F, A, k, Pt):
    out = None
    while k:
        if k & 1:
            out = ec_add(F, A, out, Pt)
        Pt = ec_add(F, A, Pt, Pt)
        k >>= 1
    return out


def ec_neg(F, Pt):
    return None if Pt is None else (Pt[0], F.neg(Pt[1]))


class Suite:
    """The parameters of RFC 9380 section 8.8.1 / 8.8.2, as the issue of this feature states them."""

    def __init__(self, group):
        self.group = group
        if group == "g1":
            F = self.F = Field(1)
            self.Z = F.el(11)
            self.A = F.el(0x144698a3b8e9433d693a02c96d4982b0ea985383ee66a8d8e8981aefd881ac98936f8da0e0f97f5cf428082d584c1d)
            self.B = F.el(0x12e2908d11688030018b12e8753eee3b2016c1f0f24f4070a0b9c14fcef35ef55a23215a316ceaa5d1cc48e98e172be0)
            self.B_E = F.el(4)
            self.ell = 11
        else:
            F = self.F = Field(2)
            self.Z = F.el(-2, -1)
            self.A = F.el(0, 240)
            self.B = F.el(1012, 1012)
            self.B_E = F.el(4, 4)
            self.ell = 3
        self.fixture = os.path.join(ROOT, "tests", "golden", "h2c", "BLS12381%s_XMD-SHA-256_SSWU_RO_.json" % group.upper())

    def g(self, x):
        F = self.F
        return F.add(F.add(F.mul(F.sqr(x), x), F.mul(self.A, x)), self.B)


def sswu(S, u):
    """The simplified SWU map of RFC 9380 section 6.6.2, as the operations list states it (not the optimised form)."""
    F = S.F
    zu2 = F.mul(S.Z, F.sqr(u))
    tv1 = F.add(F.sqr(zu2), zu2)
    if tv1 == F.zero:
        x1 = F.div(S.B, F.mul(S.Z, S.A))
    else:
        x1 = F.mul(F.div(F.neg(S.B), S.A), F.add(F.one, F.inv(tv1)))
    gx1 = S.g(x1)
    x2 = F.mul(zu2, x1)
    gx2 = S.g(x2)
    if F.is_square(gx1):
        x, y = x1, F.sqrt(gx1)
    else:
        x, y = x2, F.sqrt(gx2)
    if F.sgn0(u) != F.sgn0(y):
        y = F.neg(y)
    return (x, y)


def kernel_half(S):
    """[(x_Q, y_Q^2)] over one of Q, -Q each of the kernel of the isogeny E' -> E."""
    F = S.F
    if S.group == "g1":
        n = H1 * R_ORDER
        assert n % 121 == 0
        rng = random.Random(11)
        while True:
            x = F.el(rng.randrange(P))
            y = F.sqrt(S.g(x))
            if y is None:
                continue
            T = ec_mul(F, S.A, n // 11, (x, y))
            if T is not None:
                break
        assert ec_mul(F, S.A, 11, T) is None
        pts, Q = [], None
        for _ in range(5):
            Q = ec_add(F, S.A, Q, T)
            pts.append((Q[0], F.sqr(Q[1])))
        return sorted(pts)      # (the order of summation does not matter; sorted so that the choice of T does not show)
    # psi_3 = 3x^4 + 6A x^2 + 12B x - A^2, and its roots in Fp2: gcd with x^q - x
    f = [F.neg(F.sqr(S.A)), F.muli(S.B, 12), F.muli(S.A, 6), F.zero, F.el(3)]
    xq, base, e = [F.one], [F.zero, F.one], F.q
    while e:
        if e & 1:
            xq = p_mod(F, p_mul(F, xq, base), f)
        base = p_mod(F, p_mul(F, base, base), f)
        e >>= 1
    lin = p_gcd(F, f, p_sub(F, xq, [F.zero, F.one]))
    assert len(lin) == 2, "psi_3 has %d roots in Fp2, not one" % (len(lin) - 1)
    xq = F.neg(lin[0])
    return [(xq, S.g(xq))]


def derive(S):
    """dict: kernel [(x_Q, v_Q, u_Q)], the three polynomials before scaling, and the scalings (s2, s3) = (c^2, c^3) that fit."""
    F = S.F
    ker = [(x, F.muli(F.add(F.muli(F.sqr(x), 3), S.A), 2), F.muli(y2, 4)) for x, y2 in kernel_half(S)]
    t = w = F.zero
    for x, v, u in ker:
        t = F.add(t, v)
        w = F.add(w, F.add(u, F.mul(x, v)))
    a_star, b_star = F.sub(S.A, F.muli(t, 5)), F.sub(S.B, F.muli(w, 7))
    assert a_star == F.zero, "the codomain is not of the form y^2 = x^3 + b"
    # X = N / h^2,  dX/dx = (N' h - 2 N h') / h^3
    h = [F.one]
    for x, _, _ in ker:
        h = p_mul(F, h, [F.neg(x), F.one])
    N = p_mul(F, [F.zero, F.one], p_mul(F, h, h))
    for x, v, u in ker:
        others = [F.one]
        for x2, _, _ in ker:
            if x2 != x:
                others = p_mul(F, others, [F.neg(x2), F.one])
        o2 = p_mul(F, others, others)
        N = p_add(F, N, p_mul(F, o2, p_add(F, p_scale(F, [F.neg(x), F.one], v), [u])))
    Yn = p_sub(F, p_mul(F, p_deriv(F, N), h), p_scale(F, p_mul(F, N, p_deriv(F, h)), F.el(2)))
    k = F.div(S.B_E, b_star)
    s3s = [F.sqrt(k)]
    assert s3s[0] is not None
    s3s.append(F.neg(s3s[0]))
    out = {"kernel": ker, "h": h, "x_num": N, "y_num": Yn, "b_star": b_star}
    vec = json.load(open(S.fixture))["vectors"]
    fits = []
    for s2 in F.cube_roots(k):
        for s3 in s3s:
            out["s2"], out["s3"] = s2, s3
            ok = True
            for v in vec:
                for j, name in enumerate(("Q0", "Q1")):
                    u = F.el(*[int(c, 16) for c in v["u"][j].split(",")])
                    want = tuple(F.el(*[int(c, 16) for c in v[name][xy].split(",")]) for xy in "xy")
                    ok = ok and isogeny(S, out, sswu(S, u)) == want
            if ok:
                fits.append((s2, s3))
    assert len(fits) == 1, "%d of the six scalings reproduce the recorded Q0, Q1; expected one" % len(fits)
    out["s2"], out["s3"] = fits[0]
    return out


def isogeny(S, iso, Pt):
    """Velu's map as its sums, then the scaling; None at a kernel point."""
    F = S.F
    x, y = Pt
    X, dX = x, F.one
    for xq, v, u in iso["kernel"]:
        d = F.sub(x, xq)
        if d == F.zero:
            return None
        di = F.inv(d)
        d2, d3 = F.sqr(di), F.mul(F.sqr(di), di)
        X = F.add(X, F.add(F.mul(v, di), F.mul(u, d2)))
        dX = F.sub(dX, F.add(F.mul(v, d2), F.mul(F.muli(u, 2), d3)))
    return (F.mul(iso["s2"], X), F.mul(iso["s3"], F.mul(y, dX)))


# ---- rendering -----------------------------------------------------------------------------------------------------------------
def limbs(x):
    x = x * R % P
    return "{%s}" % ", ".join("0x%08xu" % ((x >> (LB * i)) & ((1 << LB) - 1)) for i in range(NL))


def el_rows(F, a):
    return "{%s}" % ", ".join(limbs(c) for c in a)


def words(x, n):
    assert 0 <= x < 1 << (32 * n)
    return ", ".join("0x%08xu" % ((x >> (32 * i)) & 0xffffffff) for i in range(n))


def sqrt_ratio_roots(S):
    """The correcting factors c with c^2 = 1/w for the 2^(s-1)-th roots of unity w (u/v a square), then c^2 = Z/w' for the primitive
    2^s-th roots w' (u/v none)."""
    F = S.F
    s = 1 if F.m == 1 else 3
    assert F.q % (1 << (s + 1)) == (1 << s) + 1
    rng = random.Random(3)
    while True:
        g = tuple(rng.randrange(P) for _ in range(F.m))
        zeta = F.pow(g, (F.q - 1) >> s)
        if F.pow(zeta, 1 << (s - 1)) != F.one:
            break                                    # zeta: a primitive 2^s-th root of unity
    sq, non = [], []
    for k in range(1 << s):
        w = F.pow(zeta, k)
        if k % 2 == 0:
            sq.append(F.one if w == F.one else F.sqrt(F.inv(w)))
        else:
            non.append(F.sqrt(F.div(S.Z, w)))
    assert None not in sq and None not in non
    # (either root of a pair serves: the sign of y is fixed afterwards; sorted so that the choice of g does not show)
    sq, non = sorted(min(x, F.neg(x)) for x in sq), sorted(min(x, F.neg(x)) for x in non)
    sq = [F.one if x in (F.one, F.neg(F.one)) else x for x in sq]
    sq.sort(key=lambda x: x != F.one)                # 1 first
    assert len(sq) == len(non) == 1 << (s - 1)
    return s, sq, non


def render():
    out = ["// GENERATED by tools/gen_h2c_consts.py -- do not edit.",
           "// Hash-to-curve constants of BLS12-381 (RFC 9380 section 8.8), derived from Z, A', B' alone.  Field elements: one row of",
           "// radix-2^28 limbs * R mod p (R = 2^392) per Fp component; EXP: plain 32-bit words.",
           "struct H2c_381_Common {",
           "  static constexpr uint32_t TWO_256[%d] = %s;   // 2^256" % (NL, limbs(1 << 256)),
           "};"]
    for group in ("g1", "g2"):
        S = Suite(group)
        F = S.F
        iso = derive(S)
        s, sq, non = sqrt_ratio_roots(S)
        exp = (F.q - (1 << s) - 1) >> (s + 1)
        m, nw = F.m, 12 * F.m
        dh = len(iso["h"]) - 1
        assert len(iso["x_num"]) == 2 * dh + 2 and len(iso["y_num"]) == 3 * dh + 1
        out.append("struct H2c_381_%s {" % group.upper())
        out.append("  static constexpr int M = %d, S = %d, NROOTS = %d, EXP_WORDS = %d, EXP_BITS = %d, DEG_H = %d;" % (m, s, len(sq), nw, exp.bit_length(), dh))
        for name, v, note in (("A", S.A, "A' of E'"), ("B", S.B, "B' of E'"), ("Z", S.Z, "the non-square Z"), ("ZA", F.mul(S.Z, S.A), "Z A'")):
            out.append("  static constexpr uint32_t %s[%d][%d] = %s;   // %s" % (name, m, NL, el_rows(F, v), note))
        out.append("  static constexpr uint32_t EXP[%d] = {%s};   // (q - 2^S - 1) / 2^(S+1)" % (nw, words(exp, nw)))
        out.append("  // c with (gamma c)^2 v == u: NROOTS for u/v a square, then NROOTS with (gamma c)^2 v == Z u")
        out.append("  static constexpr uint32_t ROOTS[%d][%d][%d] = {" % (2 * len(sq), m, NL))
        for c in sq + non:
            out.append("    %s," % el_rows(F, c))
        out.append("  };")
        for name, poly, k, note in (("X_NUM", iso["x_num"], iso["s2"], "c^2 x_num, degree 2 DEG_H + 1"), ("H", iso["h"], F.one, "h = prod (x - x_Q), monic"),
                                    ("Y_NUM", iso["y_num"], iso["s3"], "c^3 y_num, degree 3 DEG_H")):
            out.append("  static constexpr uint32_t %s[%d][%d][%d] = {   // %s; from the constant term up" % (name, len(poly), m, NL, note))
            for c in poly:
                out.append("    %s," % el_rows(F, F.mul(c, k)))
            out.append("  };")
        out.append("};")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    print(render(), end="")
