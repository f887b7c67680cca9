"""Records at the corners of the stored-point contract of csrc/curve.hpp, and a model that can judge them.

The XYZZ laws (madd-2008-s, add-2008-s, dbl-2008-s-1, mdbl-2008-s-1) run on 14 limbs of 28 bits and are correct only while every
intermediate stays inside a limb / value bound.  What they require of their inputs -- and promise of their outputs -- is

    Xyzz.x, .y       limbs 0..12 <= 2^28 + 15, value < 16p            ("stored coordinate")
    Xyzz.zz, .zzz    normalized, value < 1.5p                         ("class M", csrc/fp28.hpp)
    Affine.x, .y     class M

A record with every limb at such a maximum is not a curve point, and the affine model (oracle/pymodel.py) cannot judge it.  It does
not have to be one: as curve.hpp performs them the laws are polynomial maps that use neither the curve equation nor ZZ^3 = ZZZ^2.  The
reference here is therefore a FORMULA MODEL: the same polynomials on residues mod p with Python integers, and the branches of the code
(infinity operands, acc_inf, the same-x split into doubling / infinity).  All values are Montgomery residues, R = 2^392:
mul(a, b) = a b R^-1 mod p;  Fp2 = Fp[u] / (u^2 + 5) for BLS12-377 and / (u^2 + 1) for BLS12-381.

Also here: the record generators (per Fp component; an Fp2 element takes one draw per component, and the structured records include the
same extreme in both), the same-x constructions (the base is DERIVED from an accumulator of any class, so doubling, cancellation and
"same x, other y" happen at extreme limbs too), and the block-wise mixing that puts several kinds of record into every wave.

A helper module, not a test (tests/test_gpu_xyzz_edges.py and tests/test_xyzz_edges_host.py use it)."""
import random

import numpy as np

from skew_cases import P as _P

NL, LB = 14, 28
LMASK = (1 << LB) - 1
R392 = 1 << (NL * LB)
TOP_SHIFT = LB * (NL - 1)
STORED_LIMB = (1 << LB) + 15          # the largest limb 0..12 of a stored coordinate (what fe_carry can leave)
NEG_BETA = {2: 5, 3: 1}
_SHIFTS = [LB * i for i in range(NL)]


def limbs_of(v):
    """Normalized radix-2^28 limbs of a non-negative integer (the top limb takes what is left)."""
    out = [(v >> s) & LMASK for s in _SHIFTS[:-1]]
    out.append(v >> TOP_SHIFT)
    assert out[-1] < (1 << 32)
    return out


def value_of(l):
    return sum(int(x) << s for x, s in zip(l, _SHIFTS))


# ---- the coordinate field on residues ---------------------------------------------------------------------------------------
class Fld:
    """Fp (curve ids 0, 1) or Fp2 (2, 3) on tuples of residues mod p.  mul() is the Montgomery product the device computes;
    pmul() / pinv() are the plain ones, used only to CONSTRUCT records."""

    def __init__(self, cid):
        self.cid = cid
        self.p = _P[cid & 1]
        self.ext = 2 if cid >= 2 else 1
        self.ew = NL * self.ext
        self.nb = NEG_BETA.get(cid, 0)
        self.rinv = pow(R392, -1, self.p)
        self.one = (R392 % self.p,) + (0,) * (self.ext - 1)      # F::ONE: the Montgomery image of 1
        self.zero = (0,) * self.ext

    def val(self, limbs):
        return tuple(value_of(limbs[j * NL:(j + 1) * NL]) % self.p for j in range(self.ext))

    def pmul(self, a, b):
        p = self.p
        if self.ext == 1:
            return (a[0] * b[0] % p,)
        return ((a[0] * b[0] - self.nb * a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)

    def mul(self, a, b):
        return tuple(x * self.rinv % self.p for x in self.pmul(a, b))

    def pinv(self, a):
        p = self.p
        if self.ext == 1:
            return (pow(a[0], -1, p),)
        ni = pow((a[0] * a[0] + self.nb * a[1] * a[1]) % p, -1, p)
        return (a[0] * ni % p, -a[1] * ni % p)

    def add(self, a, b):
        return tuple((x + y) % self.p for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.p for x, y in zip(a, b))

    def neg(self, a):
        return tuple(-x % self.p for x in a)

    def is_zero(self, a):
        return not any(a)

    def limbs(self, a, k=0):
        """canonical residues -> limbs, each component lifted by k p (k may be a tuple, one per component)"""
        ks = k if isinstance(k, tuple) else (k,) * self.ext
        return sum((limbs_of(x + kk * self.p) for x, kk in zip(a, ks)), [])

    def point(self, rec, k=4):
        """the first k elements of a record as residues"""
        return [self.val(rec[i * self.ew:(i + 1) * self.ew]) for i in range(k)]


# ---- the formula model ------------------------------------------------------------------------------------------------------
# A point is (x, y, zz, zzz) in residues; None is infinity.  A result whose zz is 0 (mod p) is infinity as well and is compared
# by that alone (same_result).
def _tail(f, P, R, PP, u1, s1):
    """X3 = R^2 - PPP - 2Q,  Y3 = R (Q - X3) - S1 PPP,  Q = U1 PP"""
    ppp, q = f.mul(P, PP), f.mul(u1, PP)
    x3 = f.sub(f.sub(f.mul(R, R), ppp), f.add(q, q))
    y3 = f.sub(f.mul(R, f.sub(q, x3)), f.mul(s1, ppp))
    return x3, y3, ppp


def model_dbl(f, a):
    """dbl-2008-s-1 as xyzz_dbl performs it (no infinity test: zz = 0 gives zz3 = 0)"""
    x, y, zz, zzz = a
    u = f.add(y, y)
    v = f.mul(u, u)
    w = f.mul(u, v)
    s = f.mul(x, v)
    xx = f.mul(x, x)
    m = f.add(f.add(xx, xx), xx)
    x3 = f.sub(f.mul(m, m), f.add(s, s))
    y3 = f.sub(f.mul(m, f.sub(s, x3)), f.mul(y, w))
    return x3, y3, f.mul(v, zz), f.mul(w, zzz)


def model_dbl_affine(f, x, y):
    """mdbl-2008-s-1 (xyzz_dbl_affine): the double of an affine point"""
    u = f.add(y, y)
    v = f.mul(u, u)
    w = f.mul(u, v)
    s = f.mul(x, v)
    xx = f.mul(x, x)
    m = f.add(f.add(xx, xx), xx)
    x3 = f.sub(f.mul(m, m), f.add(s, s))
    y3 = f.sub(f.mul(m, f.sub(s, x3)), f.mul(w, y))
    return x3, y3, v, w


def model_madd(f, acc, base, negate, acc_inf):
    """xyzz_madd: -> (result, same_x).  same_x is what xyzz_madd_common returns (it then leaves the accumulator untouched)."""
    x1, y1, zz, zzz = acc
    x2, y2 = base
    if negate:
        y2 = f.neg(y2)
    if acc_inf or f.is_zero(zz):
        return (x2, y2, f.one, f.one), False
    P = f.sub(f.mul(x2, zz), x1)
    PP = f.mul(P, P)
    if f.is_zero(PP):
        R = f.sub(f.mul(y2, zzz), y1)
        return (model_dbl_affine(f, x2, y2) if f.is_zero(f.mul(R, R)) else None), True
    R = f.sub(f.mul(y2, zzz), y1)
    x3, y3, ppp = _tail(f, P, R, PP, x1, y1)
    return (x3, y3, f.mul(zz, PP), f.mul(zzz, ppp)), False


def model_add(f, a, b):
    """xyzz_add / xyzz_add_quad"""
    x1, y1, zz1, zzz1 = a
    x2, y2, zz2, zzz2 = b
    if f.is_zero(zz2):
        return None if f.is_zero(zz1) else a
    if f.is_zero(zz1):
        return b
    u1, u2, s1, s2 = f.mul(x1, zz2), f.mul(x2, zz1), f.mul(y1, zzz2), f.mul(y2, zzz1)
    P, R = f.sub(u2, u1), f.sub(s2, s1)
    PP = f.mul(P, P)
    if f.is_zero(PP):
        return model_dbl(f, a) if f.is_zero(f.mul(R, R)) else None
    x3, y3, ppp = _tail(f, P, R, PP, u1, s1)
    return x3, y3, f.mul(f.mul(zz1, zz2), PP), f.mul(f.mul(zzz1, zzz2), ppp)


def same_result(f, got, exp):
    """got: four residues;  exp: four residues or None (infinity)"""
    if exp is None or f.is_zero(exp[2]):
        return f.is_zero(got[2])
    return tuple(got) == tuple(exp)


# ---- per-component generators -----------------------------------------------------------------------------------------------
def stored_cap(p):
    """the largest top limb of a stored coordinate whose other limbs are all maximal: keeps the value < 16p"""
    return ((16 * p) >> TOP_SHIFT) - 2


STORED_STRUCTURED = [("max", None), ("zero", None)] + [("cold", i) for i in range(NL)] + [("hot", i) for i in range(NL)]
STORED_RANDOM = ("near", "kp", "carry", "uniform")
STORED_EXTREME = ("max", "cold", "hot", "near", "carry")
M_EXTREME = ("max", "cold", "val", "random")


def stored(p, rng, cls, arg=None):
    """One Fp component of a stored X / Y: limbs 0..12 <= 2^28 + 15, value < 16p."""
    lim, cap = STORED_LIMB, stored_cap(p)
    if cls == "max":
        return [lim] * (NL - 1) + [cap]
    if cls == "zero":
        return [0] * NL
    if cls == "cold":          # one limb zero, the rest maximal
        r = [lim] * (NL - 1) + [cap]
        r[rng.randrange(NL) if arg is None else arg] = 0
        return r
    if cls == "hot":           # one limb maximal, the rest zero
        i = rng.randrange(NL) if arg is None else arg
        r = [0] * NL
        r[i] = cap if i == NL - 1 else lim
        return r
    if cls == "near":          # within 40 of the maximum
        return [rng.randrange(lim - 40, lim + 1) for _ in range(NL - 1)] + [rng.randrange(cap - 40, cap + 1)]
    if cls == "kp":            # canonical + k p, normalized
        return limbs_of(rng.randrange(p) + (rng.randrange(16) if arg is None else arg) * p)
    if cls == "carry":         # what fe_carry leaves: a normalized value with an excess < 16 on every limb below the top
        v = limbs_of(rng.randrange(15 * p))
        return [x + rng.randrange(16) for x in v[:-1]] + [v[-1]]
    assert cls == "uniform"
    return [rng.randrange(lim + 1) for _ in range(NL - 1)] + [rng.randrange(cap + 1)]


def m_values(p):
    return (0, 1, p - 1, p, p + 1, 3 * p // 2 - 1)


def m_structured(p, zero_too):
    """the structured class-M records; 0 and p (infinity as a ZZ) only on request"""
    return [("max", None)] + [("val", v) for v in m_values(p) if zero_too or v % p] + [("cold", i) for i in range(NL - 1)]


def class_m(p, rng, cls, arg=None):
    """One Fp component of class M: normalized, value < 1.5p."""
    top = (3 * p // 2) >> TOP_SHIFT
    if cls == "max":           # limbs 2^28 - 1 under the top limb of 1.5p, less one
        return [LMASK] * (NL - 1) + [top - 1]
    if cls == "val":
        return limbs_of(rng.choice(m_values(p)) if arg is None else arg)
    if cls == "cold":
        r = [LMASK] * (NL - 1) + [top - 1]
        r[rng.randrange(NL - 1) if arg is None else arg] = 0
        return r
    assert cls == "random"
    return limbs_of(rng.randrange(3 * p // 2))


class Gen:
    """Element and point draws for one curve.  cls=None draws a class per COMPONENT; a named class puts that extreme into every
    component (both=True) or into component 0 only, the other one drawn freely."""

    def __init__(self, cid, seed):
        self.f = Fld(cid)
        self.rng = random.Random(seed)

    def st(self, cls=None, arg=None, both=True, pool=None):
        f, rng = self.f, self.rng
        out = []
        for j in range(f.ext):
            if cls is not None and (both or j == 0):
                out += stored(f.p, rng, cls, arg)
            else:
                out += stored(f.p, rng, rng.choice(pool or ("max", "zero", "cold", "hot") + STORED_RANDOM))
        return out

    def cm(self, cls=None, arg=None, both=True, nonzero=False, pool=None):
        f, rng = self.f, self.rng
        while True:
            out = []
            for j in range(f.ext):
                if cls is not None and (both or j == 0):
                    out += class_m(f.p, rng, cls, arg)
                else:
                    out += class_m(f.p, rng, rng.choice(pool or ("max", "val", "cold", "random", "random", "random")))
            if not nonzero or not f.is_zero(f.val(out)):
                return out

    def inf_zz(self):
        """ZZ == 0 (mod p): each component 0 or p"""
        return sum((limbs_of(self.rng.choice((0, self.f.p))) for _ in range(self.f.ext)), [])

    def acc(self, invertible=False):
        """an accumulator of any class, extremes included, not at infinity; invertible: ZZZ != 0 (mod p) too"""
        x = self.st(*self._pick_stored())
        y = self.st(*self._pick_stored())
        return x + y + self.cm(nonzero=True) + self.cm(nonzero=invertible)

    def _pick_stored(self):
        rng = self.rng
        if rng.randrange(3) == 0:
            return rng.choice(STORED_STRUCTURED)       # the same extreme in every component
        return (None, None)

    def extreme_acc(self):
        """a starting point for the trajectories: X, Y from the classes at the limb / value caps, ZZ, ZZZ mostly at class M's"""
        return self.st(pool=STORED_EXTREME) + self.st(pool=STORED_EXTREME) + self.cm(nonzero=True, pool=M_EXTREME) + self.cm(nonzero=True, pool=M_EXTREME)

    def max_acc(self):
        return self.st("max") + self.st("max") + self.cm("max") + self.cm("max")

    def base_repr(self, a):
        """class-M limbs of canonical residues: + p where that stays below 1.5p, at random"""
        f, rng = self.f, self.rng
        return f.limbs(a, tuple(1 if 2 * x < f.p - 2 and rng.randrange(2) else 0 for x in a))

    def stored_repr(self, a):
        """stored-coordinate limbs of canonical residues: + k p, k = 0..15"""
        return self.f.limbs(a, tuple(self.rng.randrange(16) for _ in a))

    def other(self, a, *avoid):
        """a residue different from every one of `avoid`, near or far from a"""
        f, rng = self.f, self.rng
        while True:
            d = tuple(rng.choice((0, 1, f.p - 1, rng.randrange(f.p))) for _ in a)
            r = f.add(a, d)
            if all(r != v for v in avoid):
                return r


def structured_points(g, second_family):
    """accumulators at every (stored structured class) x (class-M structured class): X, Y of the one, ZZ, ZZZ of the other, the same
    extreme in both Fp2 components;  second_family: Y and ZZZ of the NEXT class, and the extreme in component 0 only."""
    f = g.f
    ms = m_structured(f.p, zero_too=False)
    out = []
    for i, (sc, sa) in enumerate(STORED_STRUCTURED):
        for j, (mc, ma) in enumerate(ms):
            if not second_family:
                out.append(g.st(sc, sa) + g.st(sc, sa) + g.cm(mc, ma) + g.cm(mc, ma))
            else:
                sc2, sa2 = STORED_STRUCTURED[(i + 1) % len(STORED_STRUCTURED)]
                mc2, ma2 = ms[(j + 1) % len(ms)]
                out.append(g.st(sc, sa, both=False) + g.st(sc2, sa2, both=False) + g.cm(mc, ma, both=False, nonzero=True) + g.cm(mc2, ma2, both=False))
    return out


def half_zero_zz(g):
    """Fp2 only: ZZ with exactly one component 0 (mod p) -- NOT infinity"""
    f = g.f
    out = []
    for z in (0, f.p):
        nz = class_m(f.p, g.rng, "random")
        while value_of(nz) % f.p == 0:
            nz = class_m(f.p, g.rng, "random")
        out += [limbs_of(z) + nz, nz + limbs_of(z)]
    return out


# ---- records for the four ops -----------------------------------------------------------------------------------------------
MADD_SPECIAL = ("double", "cancel", "same_x_inf", "near_miss", "inf_zz", "fresh")
ADD_SPECIAL = ("double", "cancel", "same_x_inf", "near_miss", "inf_b", "inf_a")


def madd_general(g, n):
    """-> n MADD records [acc | base | flags], the structured ones first, and how many are structured"""
    f, rng = g.f, g.rng
    ms = m_structured(f.p, zero_too=True)
    recs = []
    for fam in (False, True):
        for i, acc in enumerate(structured_points(g, fam)):
            mc, ma = ms[(i + i // len(ms)) % len(ms)]
            if not fam:
                base = g.cm(mc, ma) + g.cm(mc, ma)
            else:
                base = g.cm(mc, ma, both=False) + g.cm()
            recs.append(acc + base + [(i + fam) & 1])
    if f.ext == 2:
        for zz in half_zero_zz(g):
            recs.append(g.st() + g.st() + zz + g.cm() + g.cm() + g.cm() + [rng.randrange(2)])
    n_struct = len(recs)
    assert n_struct <= n, (n_struct, n)
    while len(recs) < n:
        recs.append(g.acc() + g.cm() + g.cm() + [rng.randrange(2)])
    return recs, n_struct


def madd_special(g, kind):
    f, rng = g.f, g.rng
    neg = rng.randrange(2)
    if kind == "inf_zz":
        return g.st() + g.st() + g.inf_zz() + g.cm() + g.cm() + g.cm() + [neg | (rng.randrange(4) == 0) << 1]
    if kind == "fresh":            # acc_inf: the caller says the accumulator is empty, whatever it holds
        return g.acc() + g.cm() + g.cm() + [neg | 2]
    acc = g.acc(invertible=True)
    x1, y1, zz, zzz = f.point(acc)
    x2 = f.pmul(f.pmul(x1, f.pinv(zz)), f.one)        # mul(x2, zz) == x1 whatever representation x1 has
    yd = f.pmul(f.pmul(y1, f.pinv(zzz)), f.one)       # mul(yd, zzz) == y1
    if kind == "double":
        y_eff = yd
    elif kind == "cancel":
        y_eff = f.neg(yd)
    elif kind == "same_x_inf":
        y_eff = g.other(yd, yd, f.neg(yd))
    else:
        assert kind == "near_miss"
        j = rng.randrange(f.ext)
        x2 = tuple((x + rng.choice((1, -1))) % f.p if i == j else x for i, x in enumerate(x2))
        y_eff = rng.choice((yd, f.neg(yd)))
    y2 = f.neg(y_eff) if neg else y_eff                # either sign is reached through the negate flag as well
    return acc + g.base_repr(x2) + g.base_repr(y2) + [neg]


def add_general(g, n):
    """-> n ADD records [acc | b], the structured ones first, and how many are structured"""
    f, rng = g.f, g.rng
    recs = []
    for fam in (False, True):
        a = structured_points(g, fam)
        b = structured_points(g, fam)
        step = 1 + len(m_structured(f.p, False))
        for i, acc in enumerate(a):
            # even records: the same classes on both sides (extremes against extremes); odd ones: against another pair of classes
            recs.append(acc + (b[i] if i % 2 == 0 else b[(i + step) % len(b)]))
    if f.ext == 2:
        hz = half_zero_zz(g)
        for k, zz in enumerate(hz):
            recs.append(g.st() + g.st() + zz + g.cm() + g.acc())
            recs.append(g.acc() + g.st() + g.st() + zz + g.cm())
            recs.append(g.st() + g.st() + zz + g.cm() + g.st() + g.st() + hz[(k + 1) % len(hz)] + g.cm())
    n_struct = len(recs)
    assert n_struct <= n, (n_struct, n)
    while len(recs) < n:
        recs.append(g.acc() + g.acc())
    return recs, n_struct


def add_special(g, kind):
    f, rng = g.f, g.rng
    if kind == "inf_b":            # b at infinity; one time in four the accumulator too
        acc = g.st() + g.st() + g.inf_zz() + g.cm() if rng.randrange(4) == 0 else g.acc()
        return acc + g.st() + g.st() + g.inf_zz() + g.cm()
    if kind == "inf_a":
        return g.st() + g.st() + g.inf_zz() + g.cm() + g.acc()
    acc = g.acc(invertible=True)
    x1, y1, zz1, zzz1 = f.point(acc)
    zz2l, zzz2l = g.cm(nonzero=True), g.cm(nonzero=True)
    zz2, zzz2 = f.val(zz2l), f.val(zzz2l)
    x2 = f.pmul(x1, f.pmul(zz2, f.pinv(zz1)))          # mul(x2, zz1) == mul(x1, zz2)
    yd = f.pmul(y1, f.pmul(zzz2, f.pinv(zzz1)))        # mul(yd, zzz1) == mul(y1, zzz2)
    if kind == "double":
        y2 = yd
    elif kind == "cancel":
        y2 = f.neg(yd)
    elif kind == "same_x_inf":
        y2 = g.other(yd, yd, f.neg(yd))
    else:
        assert kind == "near_miss"
        j = rng.randrange(f.ext)
        x2 = tuple((x + rng.choice((1, -1))) % f.p if i == j else x for i, x in enumerate(x2))
        y2 = rng.choice((yd, f.neg(yd)))
    return acc + g.stored_repr(x2) + g.stored_repr(y2) + zz2l + zzz2l


def dbl_general(g, n):
    """-> n DBL records, the structured ones first (both families, ZZ at 0 and p, Fp2 half-zero ZZ), and how many those are"""
    f = g.f
    recs = structured_points(g, False) + structured_points(g, True)
    for _ in range(8):
        recs.append(g.st() + g.st() + g.inf_zz() + g.cm())
    if f.ext == 2:
        recs += [g.st() + g.st() + zz + g.cm() for zz in half_zero_zz(g)]
    n_struct = len(recs)
    assert n_struct <= n, (n_struct, n)
    while len(recs) < n:
        recs.append(g.acc())
    return recs, n_struct


# ---- lane mixing --------------------------------------------------------------------------------------------------------------
BLOCK, SPECIALS_PER_BLOCK = 8, 3


def mixed(g, n, general, special_kinds, make_special):
    """n records in blocks of 8: five general ones (drawn from `general` by a seeded permutation) and three special ones of three
    different kinds, at seeded positions; the kinds rotate, so two neighbouring blocks hold all six.  Any aligned run of 16 records
    -- a wave of the four-lane form -- therefore holds general records and at least three special kinds.
    -> (records, kinds, index of each general record in `general` or -1)"""
    rng = g.rng
    assert n % BLOCK == 0 and len(general) == n // BLOCK * (BLOCK - SPECIALS_PER_BLOCK)
    order = list(range(len(general)))
    rng.shuffle(order)
    recs, kinds, src = [], [], []
    k = rng.randrange(len(special_kinds))
    for b in range(n // BLOCK):
        where = dict(zip(rng.sample(range(BLOCK), SPECIALS_PER_BLOCK), range(SPECIALS_PER_BLOCK)))
        for pos in range(BLOCK):
            if pos in where:
                kind = special_kinds[(k + where[pos]) % len(special_kinds)]
                recs.append(make_special(g, kind))
                kinds.append(kind)
                src.append(-1)
            else:
                i = order.pop()
                recs.append(general[i])
                kinds.append("general")
                src.append(i)
        k += SPECIALS_PER_BLOCK
    return recs, kinds, src


def n_general(n):
    return n // BLOCK * (BLOCK - SPECIALS_PER_BLOCK)


def assert_waves_are_mixed(kinds, waves=32):
    """at least three kinds of record in each of the first `waves` waves: 64 records per wave in the one-lane form, 32 in the paired
    form, 16 in the four-lane form"""
    for per_wave in (64, 32, 16):
        assert len(kinds) >= waves * per_wave
        for w in range(waves):
            seen = set(kinds[w * per_wave:(w + 1) * per_wave])
            assert len(seen) >= 3, (per_wave, w, sorted(seen))


# ---- checks on outputs ------------------------------------------------------------------------------------------------------
def raw_values(f, out):
    """uint32 [n, >= 4 ew] -> per record the 4 * ext integer values of X, Y, ZZ, ZZZ (not reduced)"""
    return [[value_of(r[j * NL:(j + 1) * NL]) for j in range(4 * f.ext)] for r in out[:, :4 * f.ew].tolist()]


def assert_stored_point_invariant(f, out, vals, tag):
    """EVERY record of `out` is a stored point again: X, Y limbs < 2^28 + 16 and value < 16p; ZZ, ZZZ normalized and value < 1.5p"""
    n = out.shape[0]
    pt = out[:, :4 * f.ew].reshape(n, 4 * f.ext, NL)
    bad = np.nonzero((pt[:, :2 * f.ext, :NL - 1] > STORED_LIMB).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"{tag}: X / Y limbs above 2^28 + 15 in {bad.size} records, first {bad[0]}: {out[bad[0]].tolist()}"
    bad = np.nonzero((pt[:, 2 * f.ext:, :NL - 1] > LMASK).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"{tag}: ZZ / ZZZ not normalized in {bad.size} records, first {bad[0]}: {out[bad[0]].tolist()}"
    p16, p3 = 16 * f.p, 3 * f.p
    for i, v in enumerate(vals):
        assert all(x < p16 for x in v[:2 * f.ext]), f"{tag}: record {i}: X / Y value >= 16p: {out[i].tolist()}"
        assert all(2 * x < p3 for x in v[2 * f.ext:]), f"{tag}: record {i}: ZZ / ZZZ value >= 1.5p: {out[i].tolist()}"


def residues(f, v):
    """the values of one record (raw_values) as four residues"""
    return [tuple(x % f.p for x in v[k * f.ext:(k + 1) * f.ext]) for k in range(4)]
