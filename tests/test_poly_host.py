"""CPU: the per-element steps and the chains of launches of csrc/poly.hpp, compiled for the host with the limb-bound checker armed
(libmsm_hosttest.so, ht_poly_*: a block's loops run in order), against Python big integers.  Both fields, both element forms, tiles of
16, 32 and 1024 elements; the lengths cross all three levels of the scans below 400 elements at the small tiles."""
import ctypes
import os
import subprocess
import sys

import pytest

import ntt_cases as nc
import poly_cases as pc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    cp, ci, cu = ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.ht_poly_batch_inverse.argtypes = [ci, cu, cu, cp, cp, U64, cp]
    lib.ht_poly_evaluate.argtypes = [ci, cu, cu, cp, U64, cp, cp]
    lib.ht_poly_divide_by_linear.argtypes = [ci, cu, cu, cp, U64, cp, cp, cp]
    lib.ht_poly_vec_op.argtypes = [ci, cu, cu, cp, cp, cp, U64, cp]
    lib.ht_poly_lagrange.argtypes = [ci, cu, cu, cu, cp, cp]
    lib.ht_poly_vanishing.argtypes = [ci, cu, cu, cp, cp]
    lib.ht_poly_coset_factor.argtypes = [ci, cu, cu, cp, cp]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def no_check_failures(ht):
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def cases(field, tile_log):
    """(n, raw patterns) for every length of the issue's list, plus an all-zero vector"""
    out = [(n, pc.vector(field, n, tile_log, 0xA0 + n)) for n in pc.lengths(tile_log)] if tile_log < 10 else []
    if tile_log == 10:
        out = [(n, pc.vector(field, n, tile_log, 0xB0 + n)) for n in (0, 1, 2, 1023, 1024, 1025, 3 * 1024 + 5)]
    T = 1 << tile_log
    mult = pc.multiples_of_r(field)
    out.append((T + 5, [mult[i % len(mult)] for i in range(T + 5)]))
    return out


@pytest.mark.parametrize("tile_log", [4, 5, 10])
@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_batch_inverse(ht, field, normal, tile_log):
    r, fid = nc.modulus(field), nc.FIELD_IDS[field]
    for n, raw in cases(field, tile_log):
        vals = pc.values(field, raw, normal)
        out = ctypes.create_string_buffer(max(n, 1) * 32)
        for coeff in (None, 0, r - 1, 0x1234567):
            cb = None if coeff is None else nc.encode(field, [coeff], normal)
            assert ht.ht_poly_batch_inverse(fid, tile_log, normal, cb, pc.to_raw(raw), U64(n), out) == 0
            assert out.raw[:n * 32] == nc.encode(field, pc.ref_inverse(vals, 1 if coeff is None else coeff, r), normal), (n, coeff)
    no_check_failures(ht)


@pytest.mark.parametrize("tile_log", [4, 5, 10])
@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_and_divide_by_linear(ht, field, normal, tile_log):
    r, fid = nc.modulus(field), nc.FIELD_IDS[field]
    for n, raw in cases(field, tile_log):
        vals = pc.values(field, raw, normal)
        q = ctypes.create_string_buffer(max(n, 1) * 32)
        o32, rem = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        for z in pc.scalars(field, n):
            zb = nc.encode(field, [z], normal)
            want_q, want_rem = pc.ref_divide(vals, z, r)
            assert want_rem == pc.ref_evaluate(vals, z, r)
            assert ht.ht_poly_evaluate(fid, tile_log, normal, pc.to_raw(raw), U64(n), zb, o32) == 0
            assert o32.raw == nc.encode(field, [want_rem], normal), (n, z)
            assert ht.ht_poly_divide_by_linear(fid, tile_log, normal, pc.to_raw(raw), U64(n), zb, q, rem) == 0
            assert rem.raw == nc.encode(field, [want_rem], normal), (n, z)
            assert q.raw[:max(n - 1, 0) * 32] == nc.encode(field, want_q, normal), (n, z)
        if n:
            assert ht.ht_poly_evaluate(fid, tile_log, normal, pc.to_raw(raw), U64(n), nc.encode(field, [0], normal), o32) == 0
            assert o32.raw == nc.encode(field, vals[:1], normal)           # z = 0 gives c[0]
    no_check_failures(ht)


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_lagrange_and_vanishing(ht, field, normal):
    r, fid = nc.modulus(field), nc.FIELD_IDS[field]
    o32 = ctypes.create_string_buffer(32)
    for k, tile_log in ((0, 4), (1, 4), (4, 4), (6, 4), (6, 5), (9, 4), (11, 10)):
        n = 1 << k
        w = nc.root_of_unity(field, k)
        out = ctypes.create_string_buffer(n * 32)
        for tau in pc.scalars(field, k) + [w, pow(w, 5, r), pow(w, n // 2, r)]:
            tb = nc.encode(field, [tau], normal)
            assert ht.ht_poly_lagrange(fid, k, tile_log, normal, tb, out) == 0
            assert out.raw == nc.encode(field, pc.ref_lagrange(field, k, tau), normal), (k, tau)
            assert ht.ht_poly_vanishing(fid, k, normal, tb, o32) == 0
            assert o32.raw == nc.encode(field, [pow(tau, n, r) - 1], normal)
    no_check_failures(ht)


@pytest.mark.parametrize("field", FIELDS)
def test_coset_factor_refuses_an_offset_in_the_domain(ht, field):
    r, fid, g = nc.modulus(field), nc.FIELD_IDS[field], nc.generator(field)
    o32 = ctypes.create_string_buffer(32)
    for k in (0, 3, 12):
        n = 1 << k
        w = nc.root_of_unity(field, k)
        for normal in (0, 1):
            assert ht.ht_poly_coset_factor(fid, k, normal, None, o32) == 0
            assert o32.raw == nc.encode(field, [pow(pow(g, n, r) - 1, -1, r)], normal)
            assert ht.ht_poly_coset_factor(fid, k, normal, nc.encode(field, [5], normal), o32) == 0
            assert o32.raw == nc.encode(field, [pow(pow(5, n, r) - 1, -1, r)], normal)
            for bad in (0, 1, w, pow(w, n - 1, r), r):
                assert ht.ht_poly_coset_factor(fid, k, normal, nc.encode(field, [bad], normal), o32) == -1, (k, bad)
    no_check_failures(ht)


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_vec_op(ht, field, normal):
    r, fid = nc.modulus(field), nc.FIELD_IDS[field]
    edges = pc.multiples_of_r(field) + [1, r - 1, r + 1, (1 << 256) - 1]
    a = edges * len(edges) + pc.vector(field, 300, 4, 1, zeros=False)
    b = [e for e in edges for _ in edges] + pc.vector(field, 300, 4, 2, zeros=False)
    c = list(reversed(a))
    n = len(a)
    va, vb, vc = (pc.values(field, x, normal) for x in (a, b, c))
    out = ctypes.create_string_buffer(n * 32)
    for op, want in ((0, [x + y for x, y in zip(va, vb)]), (1, [x - y for x, y in zip(va, vb)]),
                     (2, [x * y - z for x, y, z in zip(va, vb, vc)])):
        assert ht.ht_poly_vec_op(fid, normal, op, pc.to_raw(a), pc.to_raw(b), pc.to_raw(c), U64(n), out) == 0
        assert out.raw == nc.encode(field, want, normal), op
    for s in edges[:4] + [r - 1, (1 << 256) - 1, 0xABCDEF]:
        sv = pc.values(field, [s], normal)[0]
        assert ht.ht_poly_vec_op(fid, normal, 3, pc.to_raw(a), pc.to_raw([s]), None, U64(n), out) == 0
        assert out.raw == nc.encode(field, [sv * x for x in va], normal), s
    no_check_failures(ht)


def test_bounds_tool_poly_mode():
    """the margins of the new chains (products of products, Horner steps, the scans) are positive for both fields"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "limb_bounds_fr.py"), "--poly"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all margins positive" in r.stdout and "BAD" not in r.stdout
    for what in ("Bls12_377_Fr29", "Bls12_381_Fr29", "Horner", "product of class-M", "scan"):
        assert what in r.stdout, what
