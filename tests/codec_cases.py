"""Model of arkworks' compressed point records (csrc/point_codec.hpp) in Python integers, and the cases the codec tests share.

  record   x as a little-endian normal-form integer (G2: c0 | c1); bit 6 of the last byte = infinity, bit 7 = y is the larger of
           y and -y
  larger   Fp: the integer exceeds (p - 1)/2.  Fp2: c1 decides unless it is zero, then c0.
  decode   y = sqrt(x^3 + b); the larger root iff bit 7.  Status 0 decoded or flagged infinity, 1 malformed (a component not below p
           after masking, or both flag bits), 2 no point has this x.  A failed record decodes to an all-zero record with flag 0.

Nothing here calls the code under test.
"""
from __future__ import annotations

import functools
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("oracle", "tools", "tests"):
    if os.path.join(ROOT, d) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, d))

import check_cases as cc  # noqa: E402
import pymodel as pm  # noqa: E402

OK, MALFORMED, NO_POINT, OFF_SUBGROUP = 0, 1, 2, 3
CURVE_NAMES = cc.CURVE_NAMES
R384 = 1 << 384


# ---- field level ---------------------------------------------------------------------------------------------------------------
def is_square_fp(p, a):
    return cc._is_sq(p, a)


def sqrt_fp(p, a):
    """A square root of a mod p, or None."""
    a %= p
    if not is_square_fp(p, a):
        return None
    if a == 0:
        return 0
    r = cc.te_model._sqrt(a) if p == pm.BLS12_377_G1.p else pow(a, (p + 1) // 4, p)
    assert r * r % p == a
    return r


def sqrt_fp2(p, nr, a0, a1):
    """A square root (c0, c1) of a0 + a1 u in Fp[u]/(u^2 - nr), or None."""
    a0, a1, nr = a0 % p, a1 % p, nr % p
    if a1 == 0:
        s = sqrt_fp(p, a0)
        if s is not None:
            return (s, 0)
        s = sqrt_fp(p, a0 * pow(nr, -1, p) % p)
        assert s is not None
        return (0, s)
    alpha = sqrt_fp(p, (a0 * a0 - nr * a1 * a1) % p)
    if alpha is None:
        return None
    inv2 = pow(2, -1, p)
    for delta in ((a0 + alpha) * inv2 % p, (a0 - alpha) * inv2 % p):
        c0 = sqrt_fp(p, delta)
        if c0 is not None and c0:
            c1 = a1 * pow(2 * c0, -1, p) % p
            assert (c0 * c0 + nr * c1 * c1) % p == a0 and 2 * c0 * c1 % p == a1
            return (c0, c1)
    raise AssertionError("norm is a square but no delta is")


def comps(curve, v):
    return cc.comps(curve, v)


def el_sqrt(curve, comp):
    """comp: tuple of components -> tuple of components of a root, or None."""
    if curve.ext == 1:
        s = sqrt_fp(curve.p, comp[0])
        return None if s is None else (s,)
    return sqrt_fp2(curve.p, curve.nonresidue, comp[0], comp[1])


def lex_largest(curve, y):
    """y: tuple of canonical components."""
    h = (curve.p - 1) // 2
    if curve.ext == 1:
        return y[0] > h
    return y[1] > h if y[1] else y[0] > h


def neg(curve, y):
    return tuple((-c) % curve.p for c in y)


def rhs(curve, x):
    """x^3 + b as a tuple of components."""
    X = curve.F(x[0] if curve.ext == 1 else x)
    return comps(curve, curve.f_add(curve.f_mul(curve.f_mul(X, X), X), curve.F(curve.b)))


def point_from_x(curve, x, larger):
    """(x, y) as component tuples with y the larger root iff `larger`, or None when x^3 + b has no root."""
    y = el_sqrt(curve, rhs(curve, x))
    if y is None:
        return None
    if lex_largest(curve, y) != bool(larger):
        y = neg(curve, y)
    return (tuple(x), y)


# ---- records -------------------------------------------------------------------------------------------------------------------
def _ints(stored):
    return b"".join(v.to_bytes(48, "little") for v in stored)


def compress(curve, P, lift=None):
    """P: (x, y) component tuples or None (infinity).  lift: per-component 0/1, adds p to the stored x."""
    if P is None:
        out = bytearray(curve.coord_bytes)
        out[-1] |= 0x40
        return bytes(out)
    x, y = P
    lift = lift or (0,) * curve.ext
    out = bytearray(_ints([v + l * curve.p for v, l in zip(x, lift)]))
    assert out[-1] < 0x40
    if lex_largest(curve, y):
        out[-1] |= 0x80
    return bytes(out)


def decode(curve, rec):
    """One compressed record -> (status, point): point is None for infinity AND for a failed record (status tells which)."""
    return _decode(curve.name, bytes(rec))


@functools.lru_cache(maxsize=None)
def _decode(name, rec):
    curve = pm.CURVES[name]
    assert len(rec) == curve.coord_bytes
    flags = rec[-1] >> 6
    if flags == 3:
        return MALFORMED, None
    if flags & 1:
        return OK, None
    body = bytearray(rec)
    body[-1] &= 0x3f
    x = tuple(int.from_bytes(body[48 * i:48 * i + 48], "little") for i in range(curve.ext))
    if any(v >= curve.p for v in x):
        return MALFORMED, None
    P = point_from_x(curve, x, flags >> 1)
    if P is None:
        return NO_POINT, None
    return OK, P


def uncompressed(curve, status, P):
    """What decoding writes as an uncompressed record: failed -> zeros; infinity -> (0, 1) with bit 6."""
    cb = curve.coord_bytes
    if status != OK:
        return bytes(2 * cb)
    if P is None:
        out = bytearray(2 * cb)
        out[cb] = 1
        out[-1] |= 0x40
        return bytes(out)
    return _ints(P[0] + P[1])


def image(curve, status, P, stride=None):
    """What decoding writes as an in-memory Affine image: failed -> zeros, flag 0; infinity -> zeros, flag 1."""
    stride = stride or curve.affine_stride
    cb = curve.coord_bytes
    if status != OK:
        return bytes(stride)
    if P is None:
        return bytes(2 * cb) + b"\x01" + bytes(stride - 2 * cb - 1)
    return _ints([v * R384 % curve.p for v in P[0] + P[1]]) + bytes(stride - 2 * cb)


def decode_all(curve, records):
    cb = curve.coord_bytes
    return [decode(curve, records[i:i + cb]) for i in range(0, len(records), cb)]


def expected(curve, records, serialized, stride=None):
    """(statuses, output bytes) of decoding `records`."""
    dec = decode_all(curve, records)
    f = (lambda s, P: uncompressed(curve, s, P)) if serialized else (lambda s, P: image(curve, s, P, stride))
    return [s for s, _ in dec], b"".join(f(s, P) for s, P in dec)


def _pt_of_case(curve, case):
    flag, x, y, _, _ = case
    return None if flag else (x, y)


def x_without_point(curve, rng):
    while True:
        x = tuple(rng.randrange(curve.p) for _ in range(curve.ext))
        if el_sqrt(curve, rhs(curve, x)) is None:
            return x


@functools.lru_cache(maxsize=None)
def corpus(name):
    """(records, statuses, labels, subgroup): compressed records of one curve, the decode status of each, and whether the decoded
    point lies in the order-r subgroup (True for infinity and for failed records: only status 0 can turn into 3)."""
    curve = pm.CURVES[name]
    p = curve.p
    rng = random.Random(0xC0DEC + curve.curve_id)
    recs, labels, sub = [], [], []

    def add(label, rec, in_subgroup=True):
        recs.append(rec)
        labels.append(label)
        sub.append(in_subgroup)

    G = curve.generator()
    g = (comps(curve, G[0]), comps(curve, G[1]))
    gl = point_from_x(curve, g[0], True)
    gs = point_from_x(curve, g[0], False)
    assert {gl[1], gs[1]} == {g[1], neg(curve, g[1])}
    add("generator, bit 7 set", compress(curve, gl))
    add("generator, bit 7 clear", compress(curve, gs))
    for _ in range(12):
        P = curve.mul(rng.randrange(1, curve.r), G)
        add("kG", compress(curve, (comps(curve, P[0]), comps(curve, P[1]))))
    cases, statuses, clabels = cc.corpus(name)
    n3 = 0
    for c, s, l in zip(cases, statuses, clabels):
        if s == cc.OFF_SUBGROUP and (n3 < 10 or l.startswith("T of order")):
            n3 += 1
            add("off subgroup: " + l, compress(curve, _pt_of_case(curve, c)), False)
    # x = 0 without the flag is a real point, (0, +-sqrt b)
    zero = (0,) * curve.ext
    # (where b is a square, which it is on both G1 curves; on a twist whose b is none the record has status 2 -- in no case is an
    #  unflagged zero the point at infinity)
    for larger in (True, False):
        P = point_from_x(curve, zero, larger)
        if P is None:
            assert curve.ext == 2
            add("x = 0 without the flag", bytes(curve.coord_bytes - 1) + (b"\x80" if larger else b"\x00"))
            continue
        Pm = (curve.F(P[0][0] if curve.ext == 1 else P[0]), curve.F(P[1][0] if curve.ext == 1 else P[1]))
        add("x = 0 without the flag", compress(curve, P), curve.mul(curve.r, Pm) is None)
    if name == "bls12_377_g1":
        body = bytearray((p - 1).to_bytes(48, "little"))
        add("x = p - 1 (y = 0), bit 7 clear", bytes(body), False)
        body[-1] |= 0x80
        add("x = p - 1 (y = 0), bit 7 set", bytes(body), False)
    for _ in range(6):
        x = x_without_point(curve, rng)
        rec = bytearray(_ints(x))
        if rng.random() < 0.5:
            rec[-1] |= 0x80
        add("no point has this x", bytes(rec))
    P = (comps(curve, G[0]), comps(curve, G[1]))
    for c in range(curve.ext):
        lift = tuple(1 if i == c else 0 for i in range(curve.ext))
        if P[0][c] + p < (1 << 382):
            add("x + p stored", compress(curve, P, lift))
    top = bytearray(_ints(tuple(p for _ in range(curve.ext))))
    add("x = p stored", bytes(top))
    both = bytearray(compress(curve, gl))
    both[-1] |= 0xc0
    add("both flag bits over a valid x", bytes(both))
    both = bytearray(curve.coord_bytes)
    both[-1] = 0xc0
    add("both flag bits over zero", bytes(both))
    add("infinity over zero", compress(curve, None))
    junk = bytearray(rng.randrange(256) for _ in range(curve.coord_bytes))
    junk[-1] = (junk[-1] & 0x3f) | 0x40
    add("infinity over garbage", bytes(junk))
    junk2 = bytearray(b"\xff" * curve.coord_bytes)
    junk2[-1] = 0x7f
    add("infinity over all ones", bytes(junk2))
    statuses = [decode(curve, r)[0] for r in recs]
    assert statuses.count(OK) >= 20 and statuses.count(MALFORMED) >= 4 and statuses.count(NO_POINT) >= 6
    return tuple(recs), tuple(statuses), tuple(labels), tuple(sub)


def fixture_records(name):
    """The 64 records of tests/golden/compressed/<name>.bin: the corpus, cut or filled with random subgroup points to 64."""
    curve = pm.CURVES[name]
    recs, _, _, _ = corpus(name)
    rng = random.Random(0xF1C5 + curve.curve_id)
    G = curve.generator()
    out = list(recs[:64])
    while len(out) < 64:
        P = curve.mul(rng.randrange(1, curve.r), G)
        out.append(compress(curve, (comps(curve, P[0]), comps(curve, P[1]))))
    rng.shuffle(out)
    return out


def placed(name, n, seed=0):
    """n records: valid ones everywhere, failing ones (status 1, 2 in turn) at cc.BAD_POSITIONS and n - 1 where n has them."""
    recs, statuses, _, _ = corpus(name)
    by = {0: [], 1: [], 2: []}
    for r, s in zip(recs, statuses):
        by[s].append(r)
    rng = random.Random(seed * 1000 + n)
    out = [by[0][rng.randrange(len(by[0]))] for _ in range(n)]
    st = [0] * n
    k = 0
    for pos in sorted(set(q for q in cc.BAD_POSITIONS + (n - 1,) if 0 <= q < n)):
        s = 1 + k % 2
        out[pos] = by[s][(k // 2) % len(by[s])]
        st[pos] = s
        k += 1
    return out, st
