"""A big-integer model of the BLS12-377 / BLS12-381 pairing, written from the definition, the case builders of the pairing tests and the
wrappers of the host build (libmsm_hosttest.so, ht_pairing_*).

The model shares nothing with csrc/pairing.hpp.  Fp12 is Fp[w] modulo the minimal polynomial of w over Fp (w^6 = xi, so w^12 = -5 for
BLS12-377 and w^12 = 2 w^6 - 2 for BLS12-381): an element is a list of 12 integers, the product is the dense 12 x 12 one, the inverse is
the extended Euclidean algorithm on polynomials.  A point of the twist is untwisted into E(Fp12), the Miller function f_{|x|,Q}(P) is
accumulated with the affine chord-and-tangent law there (vertical lines dropped) and raised to the INTEGER 3 (p^12 - 1) / r by one pow.
The value is arkworks' Bls12::pairing: eprint 2016/130 Table 1 computes the cube of the reduced Tate power (test_pairing_model.py evaluates
the chain in integers), and everything a projective line formula scales the lines by lies in a proper subfield, which the power kills.

The Gt image: twelve 48-byte little-endian Fp elements in arkworks' order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... (Fp12 = Fp6[w]/(w^2 - v),
Fp6 = Fp2[v]/(v^3 - xi)): the coefficient of v^m w^h is the Fp2 coefficient of w^(2m + h); Montgomery (R = 2^384) unless canonical.
"""
from __future__ import annotations

import ctypes
import os
import random
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "2022-entries_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pairing")


class Family:
    def __init__(self, name, p, r, x, beta, xi, g1, g2, m_twist):
        self.name, self.p, self.r, self.x, self.beta, self.xi, self.g1, self.g2, self.m_twist = name, p, r, x, beta, xi, g1, g2, m_twist
        # the minimal polynomial of w: w^12 = red6 * w^6 + red0
        if xi == (0, 1):        # w^6 = u, u^2 = beta
            self.red6, self.red0 = 0, beta % p
        else:                   # w^6 = 1 + u, u^2 = -1: (w^6 - 1)^2 = -1
            assert xi == (1, 1) and beta == -1
            self.red6, self.red0 = 2, (-2) % p
        self.final_power = 3 * (p ** 12 - 1) // r
        assert (p ** 12 - 1) % r == 0


F377 = Family(
    "bls12_377",
    0x01ae3a4617c510eac63b05c06ca1493b1a22d9f300f5138f1ef3622fba094800170b5d44300000008508c00000000001,
    8444461749428370424248824938781546531375899335154063827935233455917409239041,
    0x8508c00000000001, -5, (0, 1),
    (81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695,
     241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030),
    ((233578398248691099356572568220835526895379068987715365179118596935057653620464273615301663571204657964920925606294,
      140913150380207355837477652521042157274541796891053068589147167627541651775299824604154852141315666357241556069118),
     (63160294768292073209381361943935198908131692476676907196754037919244929611450776219210369229519898517858833747423,
      149157405641012693445398062341192467754805999074082136895788947234480009303640899064710353187729182149407503257491)),
    False)
F381 = Family(
    "bls12_381",
    0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
    52435875175126190479447740508185965837690552500527637822603658699938581184513,
    -0xd201000000010000, -1, (1, 1),
    (3685416753713387016781088315183077757961620795782546409894578378688607592378376318836054947676345821548104185464507,
     1339506544944476473020471379941921221584933875938349620426543736416511423956333506472724655353366534992391756441569),
    ((352701069587466618187139116011060144890029952792775240219908644239793785735715026873347600343865175952761926303160,
      3059144344244213709971259814753781636986470325476647558659373206291635324768958432433509563104347017837885763365758),
     (1985150602287291935568054521177171638300868978215655730859378665066344726373823718423869104263333984641494340347905,
      927553665492332455747201965776037880757740193453592970025027978793976877002675564980949289727957565575433344219582)),
    True)
FAMILIES = {"bls12_377": F377, "bls12_381": F381}
CURVE_OF = {"bls12_377": ("bls12_377_g1", "bls12_377_g2"), "bls12_381": ("bls12_381_g1", "bls12_381_g2")}


# ---- Fp2 (pairs) -----------------------------------------------------------------------------------------------------------------
def f2_mul(F, a, b):
    p = F.p
    return ((a[0] * b[0] + F.beta * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def f2_add(F, a, b):
    return ((a[0] + b[0]) % F.p, (a[1] + b[1]) % F.p)


def f2_sub(F, a, b):
    return ((a[0] - b[0]) % F.p, (a[1] - b[1]) % F.p)


def f2_inv(F, a):
    n = pow((a[0] * a[0] - F.beta * a[1] * a[1]) % F.p, -1, F.p)
    return (a[0] * n % F.p, -a[1] * n % F.p)


def f2_pow(F, a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = f2_mul(F, out, a)
        a = f2_mul(F, a, a)
        e >>= 1
    return out


# ---- the curves: affine points, None is infinity ---------------------------------------------------------------------------------
def _ec_add(add, sub, mul, inv, P, Q, three_x2_over_2y):
    if P is None:
        return Q
    if Q is None:
        return P
    if P[0] == Q[0]:
        if P[1] != Q[1] or P[1] == sub(P[1], P[1]):
            return None
        lam = three_x2_over_2y(P)
    else:
        lam = mul(sub(Q[1], P[1]), inv(sub(Q[0], P[0])))
    x3 = sub(sub(mul(lam, lam), P[0]), Q[0])
    return (x3, sub(mul(lam, sub(P[0], x3)), P[1]))


def g1_add(F, P, Q):
    p = F.p
    return _ec_add(lambda a, b: (a + b) % p, lambda a, b: (a - b) % p, lambda a, b: a * b % p, lambda a: pow(a, -1, p), P, Q,
                   lambda T: 3 * T[0] * T[0] * pow(2 * T[1], -1, p) % p)


def g2_add(F, P, Q):
    return _ec_add(lambda a, b: f2_add(F, a, b), lambda a, b: f2_sub(F, a, b), lambda a, b: f2_mul(F, a, b), lambda a: f2_inv(F, a), P, Q,
                   lambda T: f2_mul(F, f2_mul(F, (3, 0), f2_mul(F, T[0], T[0])), f2_inv(F, f2_add(F, T[1], T[1]))))


def _ec_mul(add, P, k):
    out = None
    while k:
        if k & 1:
            out = add(out, P)
        P = add(P, P)
        k >>= 1
    return out


def g1_mul(F, P, k):
    return _ec_mul(lambda a, b: g1_add(F, a, b), P, k % F.r)


def g2_mul(F, P, k):
    return _ec_mul(lambda a, b: g2_add(F, a, b), P, k % F.r)


def g1_neg(F, P):
    return None if P is None else (P[0], -P[1] % F.p)


# ---- Fp12 = Fp[w] / (w^12 - red6 w^6 - red0) ---------------------------------------------------------------------------------------
def f12_one():
    return [1] + [0] * 11


def f12_mul(F, a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for d in range(22, 11, -1):
        c = t[d]
        if F.red6:
            t[d - 6] += F.red6 * c
        t[d - 12] += F.red0 * c
    return [v % F.p for v in t[:12]]


def f12_pow(F, a, e):
    out = f12_one()
    for bit in bin(e)[2:]:
        out = f12_mul(F, out, out)
        if bit == "1":
            out = f12_mul(F, out, a)
    return out


def _poly_trim(a):
    while a and a[-1] == 0:
        a.pop()
    return a


def _poly_divmod(F, a, b):
    p = F.p
    a = a[:]
    q = [0] * max(1, len(a) - len(b) + 1)
    inv = pow(b[-1], -1, p)
    while len(a) >= len(b) and a:
        c = a[-1] * inv % p
        s = len(a) - len(b)
        q[s] = c
        for i, y in enumerate(b):
            a[s + i] = (a[s + i] - c * y) % p
        _poly_trim(a)
    return q, a


def f12_inv(F, a):
    """the extended Euclidean algorithm on a(w) and the minimal polynomial of w"""
    p = F.p
    m = [(-F.red0) % p] + [0] * 5 + [(-F.red6) % p] + [0] * 5 + [1]
    r0, r1 = m, _poly_trim([v % p for v in a])
    s0, s1 = [], [1]
    assert r1, "0 has no inverse"
    while len(r1) > 1:
        q, rem = _poly_divmod(F, r0, r1)
        prod = [0] * (len(q) + len(s1))
        for i, x in enumerate(q):
            for j, y in enumerate(s1):
                prod[i + j] = (prod[i + j] + x * y) % p
        n = max(len(s0), len(prod))
        s2 = _poly_trim([((s0[i] if i < len(s0) else 0) - (prod[i] if i < len(prod) else 0)) % p for i in range(n)])
        r0, r1, s0, s1 = r1, rem, s1, s2
    c = pow(r1[0], -1, p)
    out = [v * c % p for v in s1]
    return out + [0] * (12 - len(out))


def f12_from_f2(F, a, shift=0):
    """(a0 + a1 u) w^shift, shift < 6: u = w^6 (BLS12-377) or w^6 - 1 (BLS12-381)"""
    out = [0] * 12
    if F.xi == (0, 1):
        out[shift], out[shift + 6] = a[0] % F.p, a[1] % F.p
    else:
        out[shift], out[shift + 6] = (a[0] - a[1]) % F.p, a[1] % F.p
    return out


def f12_coeffs(F, a):
    """the six Fp2 coefficients of 1, w, ..., w^5"""
    out = []
    for k in range(6):
        y = a[k + 6]
        out.append(((a[k] + y) % F.p, y) if F.xi == (1, 1) else (a[k], y))
    return out


def f12_from_coeffs(F, cs):
    out = [0] * 12
    for k, c in enumerate(cs):
        t = f12_from_f2(F, c, k)
        out = [(x + y) % F.p for x, y in zip(out, t)]
    return out


def f12_conj(F, a):
    """a^(p^6): w -> -w"""
    return [(-v) % F.p if i & 1 else v for i, v in enumerate(a)]


def f12_frobenius(F, a, power):
    return f12_pow(F, a, F.p ** power)


# ---- the pairing -------------------------------------------------------------------------------------------------------------------
def untwist(F, Q):
    """E'(Fp2) -> E(Fp12): (x w^2, y w^3) for the D-type twist y^2 = x^3 + b / xi, (x / w^2, y / w^3) for the M-type y^2 = x^3 + b xi"""
    x, y = f12_from_f2(F, Q[0]), f12_from_f2(F, Q[1])
    w2, w3 = [0] * 12, [0] * 12
    w2[2] = 1
    w3[3] = 1
    if F.m_twist:
        w2, w3 = f12_inv(F, w2), f12_inv(F, w3)
    return f12_mul(F, x, w2), f12_mul(F, y, w3)


def miller(F, P, Q):
    """f_{|x|,Q}(P) in E(Fp12), conjugated when x is negative (arkworks); P in E(Fp), Q on the twist, neither infinity"""
    p = F.p
    sub = lambda a, b: [(s - t) % p for s, t in zip(a, b)]
    xq, yq = untwist(F, Q)
    xp, yp = [P[0]] + [0] * 11, [P[1]] + [0] * 11
    xt, yt = xq, yq
    f = f12_one()

    def step(lam, xa, ya, xb):
        """the line of slope lam through (xa, ya) at P, and the third point with second x coordinate xb"""
        line = sub(sub(yp, ya), f12_mul(F, lam, sub(xp, xa)))
        x3 = sub(sub(f12_mul(F, lam, lam), xa), xb)
        return line, x3, sub(f12_mul(F, lam, sub(xa, x3)), ya)

    for bit in bin(abs(F.x))[3:]:
        three = [3] + [0] * 11
        lam = f12_mul(F, f12_mul(F, three, f12_mul(F, xt, xt)), f12_inv(F, [(2 * v) % p for v in yt]))
        line, xt, yt = step(lam, xt, yt, xt)
        f = f12_mul(F, f12_mul(F, f, f), line)
        if bit == "1":
            lam = f12_mul(F, sub(yq, yt), f12_inv(F, sub(xq, xt)))
            line, xt, yt = step(lam, xt, yt, xq)
            f = f12_mul(F, f, line)
    return f12_conj(F, f) if F.x < 0 else f


def pairing(F, P, Q):
    if P is None or Q is None:
        return f12_one()
    return f12_pow(F, miller(F, P, Q), F.final_power)


def pairing_product(F, pairs):
    f = f12_one()
    for P, Q in pairs:
        if P is not None and Q is not None:
            f = f12_mul(F, f, miller(F, P, Q))
    return f12_pow(F, f, F.final_power)


# ---- images ----------------------------------------------------------------------------------------------------------------------
R384 = 1 << 384


def fp_bytes(F, v, canonical=False):
    return ((v % F.p) if canonical else (v * R384 % F.p)).to_bytes(48, "little")


def gt_image(F, a, canonical=False):
    cs = f12_coeffs(F, a)
    out = b""
    for h in (0, 1):
        for m in range(3):
            c = cs[2 * m + h]
            out += fp_bytes(F, c[0], canonical) + fp_bytes(F, c[1], canonical)
    return out


def gt_from_image(F, img, canonical=False):
    rinv = pow(R384, -1, F.p)
    vals = [int.from_bytes(img[48 * i:48 * i + 48], "little") for i in range(12)]
    if not canonical:
        vals = [v * rinv % F.p for v in vals]
    cs = [None] * 6
    for t in range(6):
        h, m = divmod(t, 3)
        cs[2 * m + h] = (vals[2 * t], vals[2 * t + 1])
    return f12_from_coeffs(F, cs)


def g1_image(F, P, junk=None):
    """arkworks Affine<G1>: x, y in Montgomery form, the infinity flag, padding to 104 bytes"""
    if P is None:
        body = junk if junk is not None else bytes(96)
        return body + b"\x01" + bytes(7)
    return fp_bytes(F, P[0]) + fp_bytes(F, P[1]) + bytes(8)


def g2_image(F, Q, junk=None):
    if Q is None:
        body = junk if junk is not None else bytes(192)
        return body + b"\x01" + bytes(7)
    return fp_bytes(F, Q[0][0]) + fp_bytes(F, Q[0][1]) + fp_bytes(F, Q[1][0]) + fp_bytes(F, Q[1][1]) + bytes(8)


# ---- golden cases --------------------------------------------------------------------------------------------------------------------
def golden_cases(F):
    """[(name, P, Q, g1 image, g2 image)]: 24 pairs a family"""
    rng = random.Random("pairing golden " + F.name)
    G1, G2 = F.g1, F.g2
    cases = [("generators", G1, G2)]
    pts = []
    for i in range(14):
        a, b = rng.randrange(1 << 252, F.r), rng.randrange(1 << 252, F.r)
        P, Q = g1_mul(F, G1, a), g2_mul(F, G2, b)
        pts.append((P, Q))
        cases.append(("random_%d" % i, P, Q))
    for i in range(3):
        cases.append(("neg_p_%d" % i, g1_neg(F, pts[i][0]), pts[i][1]))
    cases.append(("p_infinity", None, pts[3][1]))
    cases.append(("q_infinity", pts[3][0], None))
    cases.append(("both_infinity", None, None))
    out = [(n, P, Q, g1_image(F, P), g2_image(F, Q)) for n, P, Q in cases]
    # a flagged infinity with junk coordinates: the flag byte is authoritative
    out.append(("p_flagged_junk", None, pts[4][1], g1_image(F, None, junk=rng.randbytes(96)), g2_image(F, pts[4][1])))
    out.append(("q_flagged_junk", pts[4][0], None, g1_image(F, pts[4][0]), g2_image(F, None, junk=rng.randbytes(192))))
    out.append(("p_flagged_a_point", None, pts[5][1], g1_image(F, pts[5][0])[:96] + b"\x01" + bytes(7), g2_image(F, pts[5][1])))
    return out


GOLDEN_MAGIC = b"PAIRGOLD"


def golden_bytes(F):
    """the file of tools/gen_pairing_golden.py: magic, the count, then per case g1 (104), g2 (200), Gt Montgomery (576), Gt canonical (576)"""
    cases = golden_cases(F)
    out = GOLDEN_MAGIC + struct.pack("<II", len(cases), 0)
    for _, P, Q, i1, i2 in cases:
        e = pairing(F, P, Q)
        out += i1 + i2 + gt_image(F, e) + gt_image(F, e, True)
    return out


def golden_path(F):
    return os.path.join(GOLDEN, F.name + ".bin")


def load_golden(F):
    """(g1 images, g2 images, Gt Montgomery images, Gt canonical images), each a list of bytes"""
    raw = open(golden_path(F), "rb").read()
    assert raw[:8] == GOLDEN_MAGIC
    n = struct.unpack("<I", raw[8:12])[0]
    rec = 104 + 200 + 576 + 576
    assert len(raw) == 16 + n * rec
    g1, g2, em, ec = [], [], [], []
    for i in range(n):
        at = 16 + i * rec
        g1.append(raw[at:at + 104])
        g2.append(raw[at + 104:at + 304])
        em.append(raw[at + 304:at + 880])
        ec.append(raw[at + 880:at + 1456])
    return g1, g2, em, ec


# ---- the host build ----------------------------------------------------------------------------------------------------------------
_HT = None


def hosttest():
    global _HT
    if _HT is None:
        _HT = ctypes.CDLL(os.path.join(PKG, "libmsm_hosttest.so"))
        _HT.ht_check_failures.restype = ctypes.c_long
        _HT.ht_pairing_run.restype = ctypes.c_int
        _HT.ht_pairing_run.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                       ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int]
        _HT.ht_pairing_op.restype = ctypes.c_int
        _HT.ht_pairing_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint]
        _HT.ht_pairing_info.restype = ctypes.c_int
        _HT.ht_pairing_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    return _HT


FAMILY_ID = {"bls12_377": 0, "bls12_381": 1}


def host_pairing(F, g1, g2, group=1, canonical=False, check=False, g1_stride=104, g2_stride=200):
    """the host build of the three stages on concatenated images: n/group Gt images, or n/group check bytes"""
    n = len(g1) // g1_stride
    assert len(g2) == n * g2_stride and n % group == 0
    out = ctypes.create_string_buffer(max(1, (n // group) * (1 if check else 576)))
    rc = hosttest().ht_pairing_run(FAMILY_ID[F.name], out, g1, g1_stride, g2, g2_stride, n, group, 1 if canonical else 0, 1 if check else 0)
    assert rc == 0, rc
    return out.raw[:(n // group) * (1 if check else 576)]


# the tower routines of the host build (ht_pairing_op): operands and results are canonical Gt images (sparse operands with zeros)
OPS = {"mul": 0, "sqr": 1, "inv": 2, "mul_by_034": 3, "mul_by_014": 4, "cyclotomic_sqr": 5, "cyclotomic_exp": 6, "frobenius1": 7,
       "frobenius2": 8, "frobenius3": 9, "conjugate": 10, "fp6_mul": 11, "fp6_sqr": 12, "fp6_inv": 13}


def host_op(F, name, a, b=None, top=False):
    """top: the operands are stored at the top of the input class (the residue plus 2p in every coefficient)"""
    out = ctypes.create_string_buffer(576)
    rc = hosttest().ht_pairing_op(FAMILY_ID[F.name], OPS[name], out, gt_image(F, a, True), gt_image(F, b, True) if b is not None else None,
                                  1 if top else 0)
    assert rc == 0, rc
    return gt_from_image(F, out.raw, True)


def host_info(F):
    """Fp2 products of one Miller loop, one final exponentiation, one product step; operations of the first two programs; slots; block
    lanes; slots of a Miller lane; operations of the product step; lanes of a chunk"""
    v = (ctypes.c_uint64 * 10)()
    assert hosttest().ht_pairing_info(FAMILY_ID[F.name], v) == 0
    return list(v)
