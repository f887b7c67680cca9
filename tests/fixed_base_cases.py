"""Inputs shared by the fixed-base tests (host build and GPU): the bases a table is built for and the scalar edge list.  Expected
values come from the Python model alone."""
from __future__ import annotations

import functools
import random

import check_cases as cc
import pymodel as pm

CURVE_NAMES = cc.CURVE_NAMES
M256 = (1 << 256) - 1


@functools.lru_cache(maxsize=None)
def bases(name):
    """[(label, model point or None)]: the generator, a point off the subgroup, the points of small order, infinity."""
    curve = pm.CURVES[name]
    out = [("generator", curve.generator())]
    Q = cc.curve_point_from_x(curve, 1000)
    assert curve.mul(curve.r, Q) is not None
    out.append(("off the subgroup", Q))
    for q, T in cc.small_order_points(curve):
        out.append(("order %d" % q, T))
    if name == "bls12_377_g1":
        assert curve.mul(2, pm.EDGE_T) is None
        out.append(("order 2 (p - 1, 0)", pm.EDGE_T))
    out.append(("infinity", None))
    return out


def edge_scalars(curve, w):
    """0, 1, 2, 2^w - 1, 2^w, every digit at its maximum, r - 1, r, r + 1, 2^253, 2^255, 2^256 - 1"""
    r = curve.r
    return [0, 1, 2, (1 << w) - 1, 1 << w, M256, r - 1, r, r + 1, 1 << 253, 1 << 255, M256]


def random_scalars256(n, seed):
    rng = random.Random(seed)
    return [rng.getrandbits(256) for _ in range(n)]


def base_image(curve, P):
    """The Affine image of a base; infinity carries junk coordinates (the flag byte is authoritative)."""
    if P is None:
        junk = curve.encode_affine(curve.generator())
        return junk[:2 * curve.coord_bytes] + b"\x01" + bytes(7)
    return curve.encode_affine(P)


class Expect:
    """k * P for many k through the model, 16-25 ms each: memoised per base."""

    def __init__(self, curve, P):
        self.curve, self.P, self.memo = curve, P, {}

    def __call__(self, k):
        if k not in self.memo:
            self.memo[k] = None if self.P is None else self.curve.mul(k, self.P)
        return self.memo[k]

    def affine(self, ks):
        return b"".join(self.curve.encode_affine(self(k)) for k in ks)

    def projective(self, ks):
        return b"".join(self.curve.encode_projective_normalized(self(k)) for k in ks)
