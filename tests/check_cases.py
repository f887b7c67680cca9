"""Corpus for the base-point checks (status 0..3 of csrc/check_points.hpp), per curve.  The expected status comes from the Python
model ALONE: are the stored integers below p, is the point on the curve, is [r]P the point at infinity.

A case is (flag, x, y, lift_x, lift_y): x and y are tuples of normal-form components in [0, p) (one for G1, two for G2), lift_*
tuples of 0/1 that add p to the STORED integer of that component (the Montgomery image of an in-memory record, the plain integer
of a serialized one), which leaves the residue alone and makes the coordinate non-canonical.
"""
from __future__ import annotations

import functools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("oracle", "tools"):
    if os.path.join(ROOT, d) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, d))

import pymodel as pm  # noqa: E402
import subgroup_consts as sc  # noqa: E402
import te_model  # noqa: E402

VALID, NOT_CANONICAL, OFF_CURVE, OFF_SUBGROUP = 0, 1, 2, 3
CURVE_NAMES = ("bls12_377_g1", "bls12_381_g1", "bls12_377_g2", "bls12_381_g2")
R384 = 1 << 384


def family(curve):
    return curve.name[:9]


def comps(curve, v):
    return (v,) if curve.ext == 1 else (v.c0, v.c1)


def to_model(curve, x, y):
    return (curve.F(x[0] if curve.ext == 1 else x), curve.F(y[0] if curve.ext == 1 else y))


def model_status(curve, case):
    flag, x, y, lx, ly = case
    if flag:
        return VALID
    if any(lx) or any(ly):
        return NOT_CANONICAL
    P = to_model(curve, x, y)
    if not curve.on_curve(P):
        return OFF_CURVE
    return VALID if curve.mul(curve.r, P) is None else OFF_SUBGROUP


def encode(curve, case, serialized):
    """One record: the in-memory Affine image (affine_stride bytes) or the uncompressed CanonicalSerialize record."""
    flag, x, y, lx, ly = case
    p = curve.p
    out = bytearray()
    for v, l in zip(x + y, lx + ly):
        stored = (v if serialized else v * R384 % p) + l * p
        assert stored < (1 << (382 if serialized else 384))
        out += stored.to_bytes(48, "little")
    if serialized:
        if flag:
            out[-1] |= 0x40
        return bytes(out)
    return bytes(out) + bytes([1 if flag else 0]) + bytes(7)


def encode_all(curve, cases, serialized):
    return b"".join(encode(curve, c, serialized) for c in cases)


def _pt(curve, P, flag=0, lx=None, ly=None):
    z = (0,) * curve.ext
    return (flag, comps(curve, P[0]), comps(curve, P[1]), lx or z, ly or z)


def _sqrt_fq(curve):
    p = curve.p
    return te_model._sqrt if p == pm.BLS12_377_G1.p else (lambda a: pow(a, (p + 1) // 4, p))


def _is_sq(p, a):
    return a % p == 0 or pow(a % p, (p - 1) // 2, p) == 1


def curve_point_from_x(curve, start):
    """The first curve point with x = start + 1, start + 2, ... (x + u over Fq2), by solving for y."""
    p = curve.p
    sq = _sqrt_fq(curve)
    x0 = start
    while True:
        x0 += 1
        if curve.ext == 1:
            a = (x0 * x0 * x0 + curve.b) % p
            if a and _is_sq(p, a):
                P = (x0, sq(a))
                assert curve.on_curve(P)
                return P
            continue
        nr = curve.nonresidue % p
        X = pm.Fp2(x0, 1, p, nr)
        a = X * X * X + pm.Fp2(curve.b[0], curve.b[1], p, nr)
        norm = (a.c0 * a.c0 - nr * a.c1 * a.c1) % p
        if not _is_sq(p, norm):
            continue
        s = sq(norm)
        for t in ((a.c0 + s) * pow(2, -1, p) % p, (a.c0 - s) * pow(2, -1, p) % p):
            if t and _is_sq(p, t):
                y0 = sq(t)
                Y = pm.Fp2(y0, a.c1 * pow(2 * y0, -1, p) % p, p, nr)
                if Y * Y == a:
                    assert curve.on_curve((X, Y))
                    return (X, Y)


@functools.lru_cache(maxsize=None)
def small_prime_of_cofactor(name):
    """(cofactor h, its smallest prime factor below 2^20 or None)"""
    curve = pm.CURVES[name]
    h1, h2 = sc.cofactors(family(curve))
    h = h1 if curve.ext == 1 else h2
    for q in range(2, 1 << 20):
        if h % q == 0:
            return h, q
    return h, None


def small_order_points(curve):
    """Points of small prime order q | h: (h / q^e) r Q has q-power order; multiply by q until the next step would give O."""
    h, _ = small_prime_of_cofactor(curve.name)
    primes = []
    if curve.ext == 1:
        primes = [q for q in (2, 3) if h % q == 0]
    else:
        q = small_prime_of_cofactor(curve.name)[1]
        primes = [q] if q else []
    out = []
    for q in primes:
        e = 0
        while h % q ** (e + 1) == 0:
            e += 1
        start = 50
        for _ in range(8):
            Q = curve_point_from_x(curve, start)
            start = (Q[0] if curve.ext == 1 else Q[0].c0)
            T = curve.mul((h // q ** e) * curve.r, Q)      # of q-power order; the q-part of the group need not be cyclic
            if T is None:
                continue
            while curve.mul(q, T) is not None:
                T = curve.mul(q, T)
            out.append((q, T))
            break
    return out


@functools.lru_cache(maxsize=None)
def corpus(name):
    """(cases, statuses, labels) of one curve: at least 40 valid and 40 status-3 points, every status-1 and status-2 shape."""
    curve = pm.CURVES[name]
    p, r = curve.p, curve.r
    rng = random.Random(0xC0FFEE + curve.curve_id)
    G = curve.generator()
    one = (1,) + (0,) * (curve.ext - 1)
    zero = (0,) * curve.ext
    cases, labels = [], []

    def add(label, case):
        cases.append(case)
        labels.append(label)

    # ---- valid
    valid_pts = []
    for k in (1, 2, 3, 5, r - 1, r - 2):
        valid_pts.append(curve.mul(k, G))
    for _ in range(16):
        valid_pts.append(curve.mul(rng.randrange(1, r), G))
    for P in valid_pts:
        add("kG", _pt(curve, P))
        add("-kG", _pt(curve, curve.neg(P)))
    add("inf zero (0.4 style)", (1, zero, zero, zero, zero))
    add("inf (0, 1) (0.3 style)", (1, zero, one, zero, zero))
    junk = tuple(rng.randrange(p) for _ in range(curve.ext))
    add("inf junk", (1, junk, tuple(reversed(junk)), zero, zero))
    add("inf junk non-canonical", (1, junk, junk, one, zero))
    # ---- status 1
    P = valid_pts[7]
    for c in range(curve.ext):
        l = tuple(1 if i == c else 0 for i in range(curve.ext))
        add("x + p", _pt(curve, P, lx=l))
        add("y + p", _pt(curve, P, ly=l))
    f, x, y, _, _ = _pt(curve, P)
    add("x + p and off the curve", (0, x, ((y[0] + 1) % p,) + y[1:], one, zero))
    # ---- status 2
    for P in valid_pts[6:10]:
        f, x, y, _, _ = _pt(curve, P)
        add("y + 1", (0, x, ((y[0] + 1) % p,) + y[1:], zero, zero))
        add("x, y swapped", (0, y, x, zero, zero))
    add("(0, 0) without the flag", (0, zero, zero, zero, zero))
    for _ in range(6):
        add("random pair", (0, tuple(rng.randrange(p) for _ in range(curve.ext)), tuple(rng.randrange(p) for _ in range(curve.ext)), zero, zero))
    # ---- status 3
    off = []
    start = 1000
    for _ in range(32):
        Q = curve_point_from_x(curve, start)
        start = (Q[0] if curve.ext == 1 else Q[0].c0)
        off.append(Q)
        add("solved for y", _pt(curve, Q))
    for Q in off[:8]:
        add("[r]Q", _pt(curve, curve.mul(r, Q)))
    small = small_order_points(curve)
    if name == "bls12_377_g1":
        small.append((2, pm.EDGE_T))           # the FPGA harness's 2-torsion fixture (p - 1, 0)
    for q, T in small:
        add("T of order %d" % q, _pt(curve, T))
        for P in valid_pts[10:15]:
            add("P + T, T of order %d" % q, _pt(curve, curve.add(P, T)))
    statuses = [model_status(curve, c) for c in cases]
    assert statuses.count(VALID) >= 40 and statuses.count(OFF_SUBGROUP) >= 40, (name, statuses.count(VALID), statuses.count(OFF_SUBGROUP))
    assert all(l != "random pair" or s == OFF_CURVE for l, s in zip(labels, statuses))
    return tuple(cases), tuple(statuses), tuple(labels)


def by_status(name):
    cases, statuses, _ = corpus(name)
    out = {0: [], 1: [], 2: [], 3: []}
    for c, s in zip(cases, statuses):
        out[s].append(c)
    return out


BAD_POSITIONS = (0, 63, 64, 255, 256)


def placed(name, n, seed=0):
    """n cases: valid ones everywhere, bad ones (status 1, 2, 3 in turn) at index 0, 63, 64, 255, 256 and n - 1 where n has them.
    Returns (cases, statuses)."""
    bs = by_status(name)
    rng = random.Random(seed * 1000 + n)
    cases = [bs[0][rng.randrange(len(bs[0]))] for _ in range(n)]
    statuses = [0] * n
    k = 0
    for pos in sorted(set(q for q in BAD_POSITIONS + (n - 1,) if 0 <= q < n)):
        s = 1 + k % 3
        cases[pos] = bs[s][(k // 3) % len(bs[s])]
        statuses[pos] = s
        k += 1
    return cases, statuses


def summary(statuses, flags):
    """The out[0..5] words of mi355_msm_check_bases for these statuses: valid, of those flagged, status 1, 2, 3, first invalid."""
    n = len(statuses)
    first = next((i for i, s in enumerate(statuses) if s), n)
    return [sum(1 for s in statuses if s == 0), sum(1 for s, f in zip(statuses, flags) if s == 0 and f),
            sum(1 for s in statuses if s == 1), sum(1 for s in statuses if s == 2), sum(1 for s in statuses if s == 3), first]
