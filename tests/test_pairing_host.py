"""CPU: the host build of csrc/pairing.hpp (libmsm_hosttest.so, ht_pairing_*) -- the same programs and the same three stage bodies the
kernels run, lane by lane, with the limb-bound checker armed (class W on every load, the columns of every product) and no failure at the
end of any test.  All golden cases byte-equal in both output forms; groups of 1, 2, 3 and n with infinities at the first, middle and last
place and an all-infinity group; every tower routine against the big-integer model on random operands and on operands at the top of
its input class; and tests/asan_pairing.cpp, a stand-alone program over the same host code, under -fsanitize=address,undefined."""
import os
import random
import subprocess

import pytest

import pairing_cases as pc
from conftest import ROOT

FAMS = sorted(pc.FAMILIES)


@pytest.fixture(autouse=True)
def armed(built):
    ht = pc.hosttest()
    ht.ht_reset_checks()
    yield
    assert ht.ht_check_failures() == 0


@pytest.mark.parametrize("fam", FAMS)
def test_golden_cases_in_both_forms(fam):
    F = pc.FAMILIES[fam]
    g1, g2, em, ec = pc.load_golden(F)
    assert pc.host_pairing(F, b"".join(g1), b"".join(g2)) == b"".join(em)
    assert pc.host_pairing(F, b"".join(g1), b"".join(g2), canonical=True) == b"".join(ec)
    # other strides: the bytes behind an image are not read
    pad1, pad2 = b"".join(g + b"\xee" * 8 for g in g1), b"".join(g + b"\xdd" * 12 for g in g2)
    assert pc.host_pairing(F, pad1, pad2, canonical=True, g1_stride=112, g2_stride=212) == b"".join(ec)


@pytest.mark.parametrize("fam", FAMS)
def test_groups_and_infinities(fam):
    F = pc.FAMILIES[fam]
    g1, g2, _, ec = pc.load_golden(F)
    vals = [pc.gt_from_image(F, e, True) for e in ec]
    one = pc.f12_one()
    inf1, inf2 = pc.g1_image(F, None), pc.g2_image(F, None)

    def product(idx):
        out = one
        for i in idx:
            out = pc.f12_mul(F, out, vals[i])
        return pc.gt_image(F, out, True)

    for group in (1, 2, 3, 12):
        idx = list(range(12))
        got = pc.host_pairing(F, b"".join(g1[i] for i in idx), b"".join(g2[i] for i in idx), group=group, canonical=True)
        assert got == b"".join(product(idx[j:j + group]) for j in range(0, 12, group)), group
    # a group larger than the serial walk: the product tree (13 parts: two levels would need more than 8)
    idx = list(range(13))
    assert pc.host_pairing(F, b"".join(g1[i] for i in idx), b"".join(g2[i] for i in idx), group=13, canonical=True) == product(idx)
    # an infinity at the first, the middle and the last place of a group of 3, and a group of infinities only
    a = [g1[1], g1[2], g1[3]]
    b = [g2[1], g2[2], g2[3]]
    for place in range(3):
        aa, bb = list(a), list(b)
        if place == 1:
            bb[place] = inf2
        else:
            aa[place] = inf1
        assert pc.host_pairing(F, b"".join(aa), b"".join(bb), group=3, canonical=True) == product([i for i in (1, 2, 3) if i != place + 1]), place
    assert pc.host_pairing(F, inf1 * 3, b"".join(b), group=3, canonical=True) == pc.gt_image(F, one, True)
    assert pc.host_pairing(F, inf1 * 3, b"".join(b), group=3, check=True) == b"\x01"


@pytest.mark.parametrize("fam", FAMS)
def test_check_bytes(fam):
    F = pc.FAMILIES[fam]
    g1, g2, _, _ = pc.load_golden(F)
    # cases 1..3 and their negations 15..17: (P, Q), (-P, Q) multiply to one
    a = b"".join(g1[i] + g1[14 + i] for i in (1, 2, 3))
    b = b"".join(g2[i] + g2[14 + i] for i in (1, 2, 3))
    assert pc.host_pairing(F, a, b, group=2, check=True) == b"\x01\x01\x01"
    assert pc.host_pairing(F, a, b, group=1, check=True) == bytes(6)
    wrong = b"".join(g2[i] + g2[15 + i] for i in (1, 2, 3))
    assert pc.host_pairing(F, a, wrong, group=2, check=True) == bytes(3)


@pytest.mark.parametrize("top", [False, True])
@pytest.mark.parametrize("fam", FAMS)
def test_tower_routines_against_the_model(fam, top):
    F = pc.FAMILIES[fam]
    rng = random.Random("tower %s %d" % (fam, top))
    rnd = lambda: [rng.randrange(F.p) for _ in range(12)]
    sparse = lambda places: pc.f12_from_coeffs(F, [(rng.randrange(F.p), rng.randrange(F.p)) if k in places else (0, 0) for k in range(6)])
    a, b = rnd(), rnd()
    assert pc.host_op(F, "mul", a, b, top) == pc.f12_mul(F, a, b)
    assert pc.host_op(F, "sqr", a, top=top) == pc.f12_mul(F, a, a)
    assert pc.host_op(F, "inv", a, top=top) == pc.f12_inv(F, a)
    assert pc.host_op(F, "conjugate", a, top=top) == pc.f12_conj(F, a)
    for j in (1, 2, 3):
        assert pc.host_op(F, "frobenius%d" % j, a, top=top) == pc.f12_frobenius(F, a, j), j
    # the lines' places: arkworks' (c0, c3, c4) are the coefficients of 1, w, w^3, its (c0, c1, c4) those of 1, w^2, w^3
    for name, places in (("mul_by_034", (0, 1, 3)), ("mul_by_014", (0, 2, 3)), ("fp6_mul", (0, 2, 4))):
        s = sparse(places)
        assert pc.host_op(F, name, a, s, top) == pc.f12_mul(F, a, s), name
    s, t = sparse((0, 2, 4)), sparse((0, 2, 4))
    assert pc.host_op(F, "fp6_mul", s, t, top) == pc.f12_mul(F, s, t)
    assert pc.host_op(F, "fp6_sqr", s, top=top) == pc.f12_mul(F, s, s)
    assert pc.host_op(F, "fp6_inv", s, top=top) == pc.f12_inv(F, s)
    c = pc.f12_pow(F, a, (F.p ** 6 - 1) * (F.p ** 2 + 1))          # an element of the cyclotomic subgroup
    assert pc.host_op(F, "cyclotomic_sqr", c, top=top) == pc.f12_mul(F, c, c)
    e = pc.f12_pow(F, c, abs(F.x))
    assert pc.host_op(F, "cyclotomic_exp", c, top=top) == (pc.f12_conj(F, e) if F.x < 0 else e)
    # the edges of the ring
    one, zero = pc.f12_one(), [0] * 12
    assert pc.host_op(F, "mul", a, one, top) == a and pc.host_op(F, "mul", a, zero, top) == zero
    assert pc.host_op(F, "inv", one, top=top) == one


def test_counts_of_the_programs():
    """the Fp2 products a lane executes (four Fp products each) and the lengths of the programs: DESIGN.md 4m states them"""
    assert pc.host_info(pc.F377)[:3] == [3565, 4062, 36]
    assert pc.host_info(pc.F381)[:3] == [3532, 3936, 36]
    # the lengths of the programs (operations): Miller loop, final exponentiation, product step
    assert [pc.host_info(pc.F377)[i] for i in (3, 4, 8)] == [6165, 19218, 53]
    assert [pc.host_info(pc.F381)[i] for i in (3, 4, 8)] == [6118, 19052, 53]
    for F in pc.FAMILIES.values():
        v = pc.host_info(F)
        assert v[5] == 101 and v[6] == 64 and v[7] == 53 and v[9] == 131072


def test_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """tests/asan_pairing.cpp, a program with its own main over the same host code, built with -fsanitize=address,undefined and run as
    it is (no Python in the process, nothing preloaded): exact-size heap buffers, so a read or write past the images, the outputs, the
    programs or a workspace is an error"""
    exe = str(tmp_path / "asan_pairing")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "asan_pairing.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, pc.GOLDEN], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-1000:] + r.stderr[-3000:]
