"""CPU: the host build of csrc/h2c.hpp (libmsm_hosttest.so, ht_h2c_*) -- the same MSM_HD functions the kernels wrap -- against the
big-integer model of tests/h2c_cases.py, with the limb-bound checker armed and no failure at the end of any test.  SHA-256 at total
lengths 55, 56, 63, 0 (mod 64); DSTs of 1, 38, 255 and 256 bytes; the reduction (h2c_reduce, the function the kernel calls) of all-ones
and of p-adjacent 64-byte strings; sqrt_ratio on squares, non-squares and zero; the map at u = 0 and at the u with
Z^2 u^4 + Z u^2 = 0 where the field has one; the isogeny at a kernel abscissa; (u, u) and (u, -u); G2 cofactor clearing against plain
double-and-add by h_eff on 16 points off the subgroup; the offset checks; and tests/asan_h2c.cpp under -fsanitize=address,undefined."""
import hashlib
import os
import random
import subprocess

import pytest

import h2c_cases as hc
from conftest import ROOT

GROUPS = ("g1", "g2")


@pytest.fixture(autouse=True)
def armed(built):
    ht = hc.hosttest()
    ht.ht_reset_checks()
    yield
    assert ht.ht_check_failures() == 0


def test_sha256_around_the_block_boundary():
    rng = random.Random("sha")
    for n in [0, 1, 3, 54, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 183, 184, 191, 192, 517, 1000]:
        data = bytes(rng.randrange(256) for _ in range(n))
        assert hc.host_sha256(data) == hashlib.sha256(data).digest(), n


@pytest.mark.parametrize("dst_len", [1, 38, 255, 256, 300])
def test_dst_prime_and_the_zero_block(dst_len):
    dst = bytes((3 * i + 1) & 0xff for i in range(dst_len))
    prime, z = hc.host_dst(dst)
    assert prime == hc.dst_prime(dst)
    # the state after 64 zero bytes does not depend on the tag (every hash_to_field test depends on its value)
    assert len(z) == 32 and z == hc.host_dst(b"another tag")[1] and z != bytes(32)


@pytest.mark.parametrize("dst_len", [1, 38, 255, 256])
@pytest.mark.parametrize("group", GROUPS)
def test_hash_to_field_at_every_padding_position(group, dst_len):
    dst = bytes((5 * i + dst_len) & 0xff for i in range(dst_len))
    lens = hc.boundary_lengths(dst_len)
    tail = 64 + 3 + (32 if dst_len > 255 else dst_len) + 1
    assert sorted({(tail + n) % 64 for n in lens}) == [0, 55, 56, 63]
    msgs = hc.random_messages(len(lens) + 3, "field %d" % dst_len, lens + [0, 1, 200])
    for count in (1, 2):
        got = hc.host_field(group, msgs, dst, count)
        assert got == hc.u_images([u for x in msgs for u in hc.hash_to_field(group, x, dst, count)]), count


@pytest.mark.parametrize("group", GROUPS)
def test_the_fixture_vectors(group):
    d = hc.fixture("BLS12381%s_XMD-SHA-256_SSWU_RO_.json" % group.upper())
    dst = d["dst"].encode()
    msgs = [v["msg"].encode() for v in d["vectors"]]
    u = hc.host_field(group, msgs, dst)
    assert u == hc.u_images([hc.parse_el(group, t) for v in d["vectors"] for t in v["u"]])
    assert hc.points(group, hc.host_map(group, u)) == [hc.parse_point(group, v[k]) for v in d["vectors"] for k in ("Q0", "Q1")]
    assert hc.points(group, hc.host_hash(group, msgs, dst)) == [hc.parse_point(group, v["P"]) for v in d["vectors"]]
    # Projective images and a stride of the caller's
    padded = hc.host_map(group, u, 4, stride=hc.STRIDE[group] + 12)
    plain = hc.host_map(group, u, 4)
    s = hc.STRIDE[group]
    assert [padded[i * (s + 12):i * (s + 12) + s] for i in range(5)] == [plain[i * s:(i + 1) * s] for i in range(5)]


def test_the_reduction_of_all_ones_and_of_p_adjacent_strings():
    """h2c_reduce, the function the kernel calls, on raw 64-byte strings hi || lo: all ones, all zeros, p and p +- 1, the multiples of
    p next to 2^256, to 2^511 and to 2^512 and their neighbours, halves of all ones, and random ones.  (2^256 p does not fit 64 bytes:
    p has 381 bits.)  The checker is armed: the extreme limbs are where the bounds of the conversions and of the sum bite."""
    P = hc.P
    vals = [(1 << 512) - 1, 0, 1, P - 1, P, P + 1, (1 << 256) - 1, 1 << 256, (1 << 256) + 1, ((1 << 256) - 1) << 256, (1 << 511), (1 << 511) - 1]
    for bound in (1 << 256, 1 << 384, 1 << 511, (1 << 512) - 1):
        k = bound // P
        vals += [k * P - 1, k * P, k * P + 1] if k else []
        vals += [(k + 1) * P - 1, (k + 1) * P, (k + 1) * P + 1] if (k + 1) * P < 1 << 512 else []
    rng = random.Random("reduce")
    vals += [rng.randrange(1 << 512) for _ in range(32)]
    assert all(0 <= v < 1 << 512 for v in vals)
    got = hc.host_reduce([v.to_bytes(64, "big") for v in vals])
    assert got == b"".join(hc.el_image((v % P,)) for v in vals)


def _wide(group, raw64s):
    """64-byte strings -> field element, as hash_to_field reduces them"""
    return tuple(int.from_bytes(b, "big") % hc.P for b in raw64s)


@pytest.mark.parametrize("group", GROUPS)
def test_sqrt_ratio(group):
    S, _ = hc.suite(group)
    F = S.F
    rng = random.Random("sqrt_ratio " + group)
    rnd = lambda: tuple(rng.randrange(hc.P) for _ in range(F.m))
    edge = [_wide(group, [b"\xff" * 64] * F.m), _wide(group, [(hc.P + 1).to_bytes(64, "big")] * F.m), _wide(group, [(hc.P - 1).to_bytes(64, "big")] * F.m)]
    cases = [(F.zero, rnd()), (F.one, F.one), (F.sqr(rnd()), F.one), (S.Z, F.one)] + [(e, rnd()) for e in edge]
    for _ in range(12):
        v = rnd()
        r = rnd()
        cases.append((F.mul(F.sqr(r), v), v))                   # u / v a square
        cases.append((F.mul(F.mul(F.sqr(r), S.Z), v), v))       # and none
        cases.append((rnd(), v))
    squares = 0
    for u, v in cases:
        sq, y = hc.host_sqrt_ratio(group, u, v)
        ratio = F.div(u, v)
        assert sq == F.is_square(ratio), (u, v)
        assert F.sqr(y) == (ratio if sq else F.mul(S.Z, ratio)), (u, v)
        squares += sq
    assert 13 <= squares < len(cases) - 12


@pytest.mark.parametrize("group", GROUPS)
def test_the_map_at_its_special_cases(group):
    S, iso = hc.suite(group)
    F = S.F
    us = [F.zero, F.one, F.neg(F.one)]
    # Z^2 u^4 + Z u^2 = 0 with u != 0 means u^2 = -1/Z: in the field only when -1/Z is a square
    root = F.sqrt(F.neg(F.inv(S.Z)))
    if root is not None:
        us += [root, F.neg(root)]
    # Z is no square; -1 is none in Fp (p = 3 mod 4), so -1/11 is one, and -1 is a square in Fp2, so -1/Z is none there
    assert (root is None) == (group == "g2")
    rng = random.Random("map " + group)
    us += [tuple(rng.randrange(hc.P) for _ in range(F.m)) for _ in range(6)]
    got = hc.points(group, hc.host_map(group, hc.u_images(us)))
    assert got == [hc.map_to_curve(group, u) for u in us]
    assert all(hc.on_curve(group, p) for p in got)
    proj = hc.host_map(group, hc.u_images(us[:2]), 8)
    assert len(proj) == 2 * 144 * F.m and proj[:96 * F.m] == hc.host_map(group, hc.u_images(us[:1]))[:96 * F.m]


@pytest.mark.parametrize("group", GROUPS)
def test_the_isogeny_at_a_kernel_abscissa(group):
    S, iso = hc.suite(group)
    F = S.F
    rng = random.Random("iso " + group)
    for xq, _, u in iso["kernel"]:
        y = F.sqrt(S.g(xq))
        if group == "g1":
            assert y is not None                                 # G1: the kernel points are rational
        y = y if y is not None else F.one                        # G2: no such point; the abscissa alone decides
        assert hc.host_iso(group, xq, F.one, y) is None
        k = tuple(rng.randrange(1, hc.P) for _ in range(F.m))
        assert hc.host_iso(group, F.mul(xq, k), k, y) is None    # the same abscissa as xn / xd
    pt = hc.gen.sswu(S, F.el(5))
    k = tuple(rng.randrange(1, hc.P) for _ in range(F.m))
    assert hc.host_iso(group, F.mul(pt[0], k), k, pt[1]) == hc.gen.isogeny(S, iso, pt) == hc.host_iso(group, pt[0], F.one, pt[1])


@pytest.mark.parametrize("group", GROUPS)
def test_pairs_that_double_and_pairs_that_cancel(group):
    F = hc.suite(group)[0].F
    rng = random.Random("pairs " + group)
    u, v = (tuple(rng.randrange(hc.P) for _ in range(F.m)) for _ in range(2))
    seq = [u, u, u, F.neg(u), u, v, F.zero, F.zero]
    got = hc.points(group, hc.host_map(group, hc.u_images(seq), 4))
    assert got == [hc.map_pair(group, seq[2 * j], seq[2 * j + 1]) for j in range(4)]
    assert got[1] is None and got[0] is not None and got[0] == hc.clear_cofactor(group, hc.mul(group, 2, hc.map_to_curve(group, u)))
    one = hc.points(group, hc.host_map(group, hc.u_images([u, v]), 1))      # encode: each cleared on its own
    assert one == [hc.clear_cofactor(group, hc.map_to_curve(group, x)) for x in (u, v)]


@pytest.mark.parametrize("group", GROUPS)
def test_cofactor_clearing_against_double_and_add_off_the_subgroup(group):
    F = hc.suite(group)[0].F
    rng = random.Random("clear " + group)
    pts = [hc.map_to_curve(group, tuple(rng.randrange(hc.P) for _ in range(F.m))) for _ in range(16)]
    r = hc.gen.R_ORDER
    assert all(hc.mul(group, r, p) is not None for p in pts[:3])             # off the subgroup
    pts[7] = None
    imgs = hc.images(group, pts)
    fast, plain = hc.host_clear(group, imgs), hc.host_clear(group, imgs, hc.H_EFF[group])
    assert fast == plain
    got = hc.points(group, fast)
    assert got[7] is None and got[0] == hc.clear_cofactor(group, pts[0]) and hc.mul(group, r, got[0]) is None
    assert hc.H_EFF["g2"].bit_length() == 636 and hc.H_EFF["g1"] == 1 - hc.gen.Z_CURVE


def test_offset_checks():
    assert hc.host_check_offsets([0], 0) == (0, "")
    assert hc.host_check_offsets([0, 3, 3, 10], 10) == (0, "")
    assert hc.host_check_offsets([5, 3], 10)[1] == "the offsets decrease"
    assert hc.host_check_offsets([0, 4, 11], 10)[1] == "the last offset lies outside the message buffer"
    assert hc.host_check_offsets([0, 1 << 28], 1 << 30)[1] == "a message of 2^28 bytes or more"
    assert hc.host_check_offsets([1 << 63, 1 << 62], 10)[0] == -1


def test_host_code_under_address_and_undefined_sanitizers(tmp_path):
    """tests/asan_h2c.cpp, a program with its own main over the offset checks, the create-time host code and the host build of the
    kernels' functions, built with -fsanitize=address,undefined and run as it is (no Python in the process, nothing preloaded)"""
    exe = str(tmp_path / "asan_h2c")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "asan_h2c.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-1000:] + r.stderr[-3000:]
