"""Inputs and expectations shared by the segmented-MSM tests (host build and GPU).  Nothing here needs a GPU to import.

Bases are h_i * G with known logs h_i = h0 + i d (mod r), made by one model addition each, with planted rows: infinities (flag byte
set, junk coordinates), a base equal to its left neighbour, a base opposite to its left neighbour.  Two references give the expected
sums:
  naive   pymodel.Curve.msm_naive over the model points -- about 10 ms a term, for segments of up to 64 points;
  dlog    the identity of distinct_cases.py: sum s_i (h_i G) = ((sum s_i h_i) mod r) G, one multiplication per segment.
tests/test_segments_reference.py holds the two to each other.

The digit edges.  Under Booth's rule digit j is b(cj - 1) + sum_{k < c-1} b(cj + k) 2^k - b(cj + c - 1) 2^(c-1): +2^(c-1) needs the top
bit of window j clear and the top bit of window j - 1 set, -2^(c-1) the top bit of window j set and that of window j - 1 clear.  So no
scalar has every digit at one extreme; alternating_extremes(c) gives the two scalars whose digits are +2^(c-1) and -2^(c-1) in turn,
starting with either sign (window 0 has no carry-in and comes out one short)."""
from __future__ import annotations

import functools
import random

import numpy as np

import pymodel as pm

CURVE_NAMES = ("bls12_377_g1", "bls12_381_g1", "bls12_377_g2", "bls12_381_g2")
M256 = (1 << 256) - 1
KINDS = ("distinct", "same", "pairs", "planted")


def booth_digits(s, c):
    """the signed digits the kernels use, from the definition"""
    nd = (257 + c - 1) // c
    bit = lambda i: (s >> i) & 1 if 0 <= i < 256 else 0
    return [bit(c * j - 1) + sum(bit(c * j + k) << k for k in range(c - 1)) - (bit(c * j + c - 1) << (c - 1)) for j in range(nd)]


def alternating_extremes(c):
    """(s_plus_first, s_minus_first): windows alternate between 0 1..1 (digit +2^(c-1) given the carry) and 1 0..0 (digit -2^(c-1))"""
    out = []
    for first in (0, 1):
        s = 0
        for j in range(256 // c):
            top_clear = (j + first) % 2 == 0
            w = ((1 << (c - 1)) - 1) if top_clear else (1 << (c - 1))
            s |= w << (c * j)
        out.append(s & M256)
    return tuple(out)


def edge_scalars(curve):
    r = curve.r
    edges = [0, 1, 2, r - 1, r, 1 << 255, M256, int("55" * 32, 16), int("aa" * 32, 16), int("80" * 32, 16), int("88" * 32, 16)]
    for c in range(4, 10):
        edges += list(alternating_extremes(c))
    return edges


def random_scalars(n, seed, curve=None):
    """any 256 bits; with a curve, uniform below r"""
    rng = random.Random(seed)
    return [rng.randrange(curve.r) if curve else rng.getrandbits(256) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _progression(name, n, seed):
    curve = pm.CURVES[name]
    rng = random.Random(0x5E6 + seed + 16 * curve.curve_id)
    h0, d = rng.randrange(1, curve.r), rng.randrange(1, curve.r)
    G = curve.generator()
    P, D = curve.mul(h0, G), curve.mul(d, G)
    logs, pts = [], []
    for i in range(n):
        logs.append((h0 + i * d) % curve.r)
        pts.append(P)
        P = curve.add(P, D)
    return logs, pts


def base_set(name, kind, n, seed=1):
    """(logs, model points, Affine images): n bases of one kind.  "distinct": the progression.  "same": one point n times.  "pairs":
    P, -P, P, -P, ..  "planted": the progression with row 16 k + 3 an infinity, 16 k + 7 equal to its left neighbour, 16 k + 11
    opposite to it (and row 1 an infinity, row 2 equal, so that the shortest segments hold them too)."""
    curve = pm.CURVES[name]
    logs, pts = _progression(name, max(n, 1), seed)
    logs, pts = list(logs[:n]), list(pts[:n])
    junk = False
    for i in range(n):
        if kind == "same":
            logs[i], pts[i] = logs[0], pts[0]
        elif kind == "pairs" and i % 2:
            logs[i], pts[i] = (curve.r - logs[i - 1]) % curve.r, curve.neg(pts[i - 1])
        elif kind == "planted" and i > 0:
            if i % 16 == 3 or i == 1:
                logs[i], pts[i] = 0, None
            elif (i % 16 == 7 or i == 2) and pts[i - 1] is not None:
                logs[i], pts[i] = logs[i - 1], pts[i - 1]
            elif i % 16 == 11 and pts[i - 1] is not None:
                logs[i], pts[i] = (curve.r - logs[i - 1]) % curve.r, curve.neg(pts[i - 1])
    imgs = []
    for i, P in enumerate(pts):
        if P is None:
            # the flag byte is authoritative: every other infinity carries the coordinates of a real point
            img = bytearray(curve.encode_affine(pts[0] if junk and pts[0] is not None else None))
            img[2 * curve.coord_bytes] = 1
            imgs.append(bytes(img))
            junk = not junk
        else:
            imgs.append(curve.encode_affine(P))
    return logs, pts, b"".join(imgs)


def expected_naive(curve, pts, scalars, offsets):
    """model points: one msm_naive per segment over its finite bases"""
    out = []
    for a, b in zip(offsets, offsets[1:]):
        pairs = [(pts[i], scalars[i]) for i in range(a, b) if pts[i] is not None]
        out.append(curve.msm_naive([p for p, _ in pairs], [s for _, s in pairs]) if pairs else None)
    return out


def segment_logs(curve, logs, scalars, offsets):
    """[(sum_i s_i h_i) mod r] per segment"""
    return [sum(scalars[i] * logs[i] for i in range(a, b)) % curve.r for a, b in zip(offsets, offsets[1:])]


def expected_dlog(curve, logs, scalars, offsets):
    """model points by the discrete-log identity: one model multiplication per segment"""
    G = curve.generator()
    return [curve.mul(k, G) if k else None for k in segment_logs(curve, logs, scalars, offsets)]


def images(curve, values, projective=False, stride=None):
    enc = curve.encode_projective_normalized if projective else curve.encode_affine
    size = curve.projective_bytes if projective else curve.affine_stride
    stride = stride or size
    return b"".join(enc(v) + bytes(stride - size) for v in values)


def offsets_of(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


def scalar_bytes(scalars):
    return pm.encode_scalars(scalars)


def scalar_words(scalars):
    """(n, 4) uint64, the layout of distinct_cases"""
    return np.frombuffer(scalar_bytes(scalars), dtype=np.uint64).reshape(-1, 4).copy()


SMALL_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 0)


@functools.lru_cache(maxsize=None)
def small_case(name):
    """The one call of the smallest shapes: segments of SMALL_LENGTHS over planted bases, edge scalars first, then random ones.
    (logs, images, scalars, offsets, expected model points by the discrete-log identity)"""
    curve = pm.CURVES[name]
    offsets = offsets_of(SMALL_LENGTHS)
    n = offsets[-1]
    logs, pts, imgs = base_set(name, "planted", n)
    edges = edge_scalars(curve)
    scalars = (edges + random_scalars(n, 0xA11 + curve.curve_id))[:n]
    return logs, imgs, scalars, offsets, expected_dlog(curve, logs, scalars, offsets)
