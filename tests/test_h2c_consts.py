"""CPU: csrc/h2c_consts.inc is what tools/gen_h2c_consts.py writes -- the generator derives every isogeny coefficient from the suite
parameters and picks the one scaling of six that reproduces the recorded Q0, Q1 -- and what it derived has the properties the map
relies on: the kernel points have the right order, the codomain is the curve, the image of a random point of E' is on E, and the
sqrt_ratio roots square to what the header of the generator says."""
import os
import random
import subprocess
import sys

import pytest

import h2c_cases as hc
from conftest import ROOT

INC = os.path.join(ROOT, "2022-entries_amd", "csrc", "h2c_consts.inc")
gen = hc.gen


def test_the_committed_file_is_the_generated_one():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_h2c_consts.py")], capture_output=True, text=True, check=True).stdout
    assert out == open(INC).read()


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_the_derived_isogeny(group):
    S, iso = hc.suite(group)
    F = S.F
    assert len(iso["kernel"]) == (S.ell - 1) // 2 and len(iso["h"]) - 1 == (S.ell - 1) // 2
    assert F.pow(iso["s2"], 3) == F.sqr(iso["s3"]) == F.div(S.B_E, iso["b_star"])
    for xq, _, u in iso["kernel"]:
        assert gen.p_eval(F, iso["h"], xq) == F.zero
        assert u == F.muli(S.g(xq), 4)
    if group == "g1":
        xq = iso["kernel"][0][0]
        T = (xq, F.sqrt(S.g(xq)))
        assert T[1] is not None and gen.ec_mul(F, S.A, 11, T) is None           # a rational point of order 11
    rng = random.Random("iso " + group)
    for _ in range(4):
        u = tuple(rng.randrange(hc.P) for _ in range(F.m))
        pt = gen.sswu(S, u)
        assert F.sqr(pt[1]) == S.g(pt[0])
        img = gen.isogeny(S, iso, pt)
        assert hc.on_curve(group, img)
        # the polynomial form the kernels evaluate agrees with Velu's sums
        h = gen.p_eval(F, iso["h"], pt[0])
        x = F.div(F.mul(iso["s2"], gen.p_eval(F, iso["x_num"], pt[0])), F.sqr(h))
        y = F.div(F.mul(F.mul(iso["s3"], pt[1]), gen.p_eval(F, iso["y_num"], pt[0])), F.mul(F.sqr(h), h))
        assert (x, y) == img


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_the_sqrt_ratio_roots(group):
    S, _ = hc.suite(group)
    F = S.F
    s, sq, non = gen.sqrt_ratio_roots(S)
    assert s == (1 if group == "g1" else 3) and sq[0] == F.one
    assert sorted(F.pow(F.sqr(c), 1 << (s - 1)) == F.one for c in sq) == [True] * len(sq)
    for c in non:
        w = F.div(S.Z, F.sqr(c))                                             # a primitive 2^s-th root of unity
        assert F.pow(w, 1 << (s - 1)) == F.neg(F.one)
    assert len({F.sqr(c) for c in sq + non}) == 2 * len(sq)
    assert not F.is_square(S.Z)
