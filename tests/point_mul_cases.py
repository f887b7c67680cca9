"""Inputs shared by the point-multiplication tests (host build and GPU): the base kinds of fixed_base_cases.bases(name) -- the generator,
a point off the subgroup, the points of small order, EDGE_T, infinity with junk coordinates -- and the scalar edge lists.  Expected
values come from the Python model alone (fixed_base_cases.Expect, memoised per base)."""
from __future__ import annotations

import functools
import os
import random
import sys

import fixed_base_cases as fc
import pymodel as pm
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import subgroup_consts as sc  # noqa: E402

CURVE_NAMES = fc.CURVE_NAMES
M256 = fc.M256
EIGHTS = int("88" * 32, 16)   # every signed digit of every window size at an extreme, with a full carry chain
SEVENS = int("77" * 32, 16)


def cofactor(curve):
    family = "bls12_377" if "377" in curve.name else "bls12_381"
    return sc.cofactors(family)[0 if curve.ext == 1 else 1]


def pairwise_edge_scalars(curve):
    r = curve.r
    return [0, 1, 2, 7, 8, 9, 15, 16, EIGHTS, SEVENS, r - 1, r, r + 1, 1 << 255, M256]


def uniform_edge_scalars(curve):
    """[(k, byte length)]: 0, 1, 2, 3, r - 1, r, the cofactor, a 4-byte k, a 64-byte k with bit 511 set"""
    r = curve.r
    h = cofactor(curve)
    rng = random.Random(0x511 + curve.curve_id)
    return ([(k, 32) for k in (0, 1, 2, 3, r - 1, r)] + [(h, 64 if curve.ext == 2 else 16), (0xC0FFEE11, 4),
                                                         ((1 << 511) | rng.getrandbits(511), 64)])


@functools.lru_cache(maxsize=None)
def expects(name):
    """[(label, model point, Expect)] for every base kind"""
    curve = pm.CURVES[name]
    return [(label, P, fc.Expect(curve, P)) for label, P in fc.bases(name)]


def point_images(curve, points):
    return b"".join(fc.base_image(curve, P) for P in points)


def want_images(curve, values, projective=False):
    enc = curve.encode_projective_normalized if projective else curve.encode_affine
    return b"".join(enc(v) for v in values)
