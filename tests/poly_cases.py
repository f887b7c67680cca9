"""Big-integer model and case lists for the tests of csrc/poly.hpp (batch inversion, evaluation, division by X - z, Lagrange
coefficients, element-wise calls), next to the helpers of ntt_cases.py.  Nothing here comes from the code under test: inverses are
pow(x, -1, r), evaluation is Horner, division is synthetic division."""
import random

import ntt_cases as nc

RUN = 4   # the neighbours a lane owns (POLY_RUN)


def multiples_of_r(field):
    """every 256-bit byte pattern that is 0 modulo r: 14 for BLS12-377 (0 .. 13r), 3 for BLS12-381"""
    r = nc.modulus(field)
    return [k * r for k in range((1 << 256) // r + 1)]


def to_raw(ints):
    return b"".join(v.to_bytes(32, "little") for v in ints)


def lengths(tile_log):
    T = 1 << tile_log
    return [0, 1, 2, T - 1, T, T + 1, T * T - 1, T * T, T * T + T + 1]


def vector(field, n, tile_log, seed, zeros=True):
    """n raw 256-bit patterns: random ones, r - 1, 2^256 - 1, and (zeros=True) every multiple of r planted at the first and last
    position of a lane run and of a tile and over one whole tile"""
    rng = random.Random(seed)
    r = nc.modulus(field)
    T = 1 << tile_log
    raw = [rng.getrandbits(256) if i % 3 else rng.randrange(r) for i in range(n)]
    for pos, v in ((1, r - 1), (2, (1 << 256) - 1), (n - 2, r + 1)):
        if 0 <= pos < n:
            raw[pos] = v
    if zeros:
        mult = multiples_of_r(field)
        spots = [0, RUN - 1, RUN, 2 * RUN - 1, T - 1, T, 2 * T - 1, n - 1, n - RUN, n - T]
        if n >= 3 * T:
            spots += list(range(2 * T, 3 * T))           # a tile of zeros
        if n > 2 * T:
            spots += [5 * RUN + j for j in range(RUN)]   # a lane run of zeros
        for j, pos in enumerate(spots):
            if 0 <= pos < n:
                raw[pos] = mult[j % len(mult)]
    return raw


def values(field, raw, normal):
    """what raw patterns stand for in the form of the call"""
    r = nc.modulus(field)
    f = 1 if normal else pow(nc.MONT, -1, r)
    return [x * f % r for x in raw]


def scalars(field, seed):
    """z / tau: 0, 1, r - 1, w, w^(n/2) of a domain of 64 points (= r - 1 again, by another route), a random value"""
    r = nc.modulus(field)
    w = nc.root_of_unity(field, 6)
    return [0, 1, r - 1, w, pow(w, 32, r), random.Random(seed).randrange(r)]


def ref_inverse(vals, coeff, r):
    return [coeff * pow(v, -1, r) % r if v else 0 for v in vals]


def ref_evaluate(vals, z, r):
    acc = 0
    for c in reversed(vals):
        acc = (acc * z + c) % r
    return acc


def ref_divide(vals, z, r):
    """(quotient of p by X - z: len(vals) - 1 coefficients, remainder p(z))"""
    n = len(vals)
    q = [0] * max(n - 1, 0)
    acc = 0
    for i in range(n - 1, 0, -1):
        acc = (acc * z + vals[i]) % r
        q[i - 1] = acc
    return q, ((acc * z + vals[0]) % r if n else 0)


def ref_lagrange(field, k, tau):
    r = nc.modulus(field)
    n = 1 << k
    w = nc.root_of_unity(field, k)
    zt = (pow(tau, n, r) - 1) % r
    ws = [1] * n
    for i in range(1, n):
        ws[i] = ws[i - 1] * w % r
    if zt == 0:
        return [1 if x == tau % r else 0 for x in ws]
    c = zt * pow(n, -1, r) % r
    return [c * x * pow(tau - x, -1, r) % r for x in ws]
