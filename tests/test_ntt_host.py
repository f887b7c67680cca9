"""CPU: the scalar-field arithmetic of csrc/fr.hpp and the transform passes of csrc/ntt.hpp, compiled for the host with the limb-bound
checker armed (libmsm_hosttest.so, ht_fr_* / ht_ntt_*), against the big-integer model of tests/ntt_cases.py."""
import ctypes
import os
import random

import pytest

import ntt_cases as nc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    cp, ci, cu = ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.ht_fr_op.argtypes = [ci, ci, cp, cp, ci, cp]
    lib.ht_fr_extreme.argtypes = [ci]
    lib.ht_ntt_transform.argtypes = [ci, cu, cu, cu, cu, cp, cp, cu, cu, cp]
    lib.ht_ntt_element.argtypes = [ci, cu, ctypes.c_uint64, cp]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def no_check_failures(ht):
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def run(ht, field, k, pass_log, kind, flags, raw, in_len, batch=1, offset=None):
    out = ctypes.create_string_buffer(batch * (32 << k))
    assert ht.ht_ntt_transform(nc.FIELD_IDS[field], k, pass_log, kind, flags, offset, raw, in_len, batch, out) == 0
    return out.raw


def test_model_is_the_direct_sum():
    """the iterative model against the definition, n <= 64, and the inverse against the forward"""
    for field in FIELDS:
        r = nc.modulus(field)
        for k in range(7):
            x = nc.random_values(field, 1 << k, 0x100 + k)
            w = nc.root_of_unity(field, k)
            assert pow(w, 1 << k, r) == 1 and (k == 0 or pow(w, 1 << (k - 1), r) == r - 1)
            assert nc.ntt(x, w, r) == nc.dft_direct(x, w, r)
            assert nc.transform(field, k, nc.INVERSE, nc.transform(field, k, nc.FORWARD, x)) == x
            assert nc.transform(field, k, nc.COSET_INVERSE, nc.transform(field, k, nc.COSET_FORWARD, x)) == x
            g = nc.generator(field)
            assert nc.transform(field, k, nc.COSET_FORWARD, x) == [sum(v * pow(g * pow(w, i, r), j, r) for j, v in enumerate(x)) % r for i in range(1 << k)]


@pytest.mark.parametrize("field", FIELDS)
def test_elementwise(ht, field):
    """product, sum and difference on the corners of the 256-bit input range and on random pairs, both forms"""
    r = nc.modulus(field)
    rng = random.Random(0xF2)
    edges = nc.edge_values(field)
    pairs = [(a, b) for a in edges for b in edges] + [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(2000)]
    out = ctypes.create_string_buffer(32)
    minv = pow(nc.MONT, -1, r)
    for a, b in pairs:
        ra, rb = a.to_bytes(32, "little"), b.to_bytes(32, "little")
        for normal in (0, 1):
            f = 1 if normal else minv
            va, vb = a * f % r, b * f % r
            for op, want in ((0, va * vb), (1, va + vb), (2, va - vb)):
                assert ht.ht_fr_op(nc.FIELD_IDS[field], op, ra, rb, normal, out) == 0
                assert out.raw == nc.encode(field, [want], normal), (hex(a), hex(b), normal, op)
    assert ht.ht_fr_extreme(nc.FIELD_IDS[field]) == 0
    no_check_failures(ht)


@pytest.mark.parametrize("field", FIELDS)
def test_elements_are_powers_of_the_root(ht, field):
    r = nc.modulus(field)
    out = ctypes.create_string_buffer(32)
    for k in (0, 1, 5, 12, 28, nc.FIELDS[field][2]):
        w = nc.root_of_unity(field, k)
        for i in (0, 1, 2, (1 << k) - 1, (1 << k) // 2):
            assert ht.ht_ntt_element(nc.FIELD_IDS[field], k, i, out) == 0
            assert out.raw == nc.encode(field, [pow(w, i, r)], False)
    no_check_failures(ht)


_MODEL = {}


def model(field, k, kind, order, in_len, seed):
    key = (field, k, kind, order, in_len, seed)
    if key not in _MODEL:
        x = nc.random_values(field, 1 << k, seed)
        _MODEL[key] = (x, nc.transform(field, k, kind, [v if i < in_len else 0 for i, v in enumerate(x)], order_flags=order))
    return _MODEL[key]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", range(13))
def test_transforms(ht, field, k):
    """every pass_log in 1..6 at this size: the four kinds, with the form, the order and in_len going round so that each meets each
    kind; a batch of three distinct vectors, the bound checker armed"""
    n = 1 << k
    in_lens = [0, 1, n // 2 + 1, n]
    for pass_log in range(1, 7):
        for kind in range(4):
            turn = pass_log + kind + k
            normal = turn & 1
            reordered = (turn >> 1) & 1
            order = 0 if not reordered else (nc.FLAG_RN if kind & 1 else nc.FLAG_NR)
            in_len = min(in_lens[(turn >> 2) & 3], n)   # (with a bit-reversed input, in_len cuts the stored order)
            vecs = [model(field, k, kind, order, in_len, 0x5EED + 3 * k + b) for b in range(3)]
            raw = b"".join(nc.encode(field, x, normal) for x, _ in vecs)
            got = run(ht, field, k, pass_log, kind, order | normal, raw, in_len, batch=3)
            want = b"".join(nc.encode(field, y, normal) for _, y in vecs)
            assert got == want, (field, k, pass_log, kind, normal, order, in_len)
    no_check_failures(ht)


@pytest.mark.parametrize("field", FIELDS)
def test_every_option_at_one_size(ht, field):
    """k = 6, pass_log 2 (three passes) and 4 (a ragged pair): the full product of kind, form, order and in_len"""
    k, n = 6, 64
    for pass_log in (2, 4):
        for kind in range(4):
            for normal in (0, 1):
                for order in (0, nc.FLAG_RN if kind & 1 else nc.FLAG_NR):
                    for in_len in (0, 1, n // 2 + 1, n):
                        x, y = model(field, k, kind, order, in_len, 0xA11)
                        got = run(ht, field, k, pass_log, kind, order | normal, nc.encode(field, x, normal), in_len)
                        assert got == nc.encode(field, y, normal), (pass_log, kind, normal, order, in_len)
    no_check_failures(ht)


@pytest.mark.parametrize("field", FIELDS)
def test_arkworks_domain_property(ht, field):
    """ARK poly/src/domain/radix2/mod.rs:348-388: fft is evaluation at element(i), coset_fft at GENERATOR * element(i)"""
    r = nc.modulus(field)
    out = ctypes.create_string_buffer(32)
    for k in range(6):
        n = 1 << k
        coeffs = nc.random_values(field, n, 0xE7A1 + k)
        raw = nc.encode(field, coeffs, False)
        plain = nc.decode(field, run(ht, field, k, 3, nc.FORWARD, 0, raw, n), False)
        coset = nc.decode(field, run(ht, field, k, 3, nc.COSET_FORWARD, 0, raw, n), False)
        for i in range(n):
            assert ht.ht_ntt_element(nc.FIELD_IDS[field], k, i, out) == 0
            e = nc.decode(field, out.raw, False)[0]
            assert plain[i] == sum(c * pow(e, j, r) for j, c in enumerate(coeffs)) % r
            assert coset[i] == sum(c * pow(nc.generator(field) * e, j, r) for j, c in enumerate(coeffs)) % r
    no_check_failures(ht)


@pytest.mark.parametrize("field", FIELDS)
def test_inputs_above_the_modulus_and_offsets(ht, field):
    """any 256-bit input stands for its residue; offset 1 is the plain transform; a custom offset"""
    r = nc.modulus(field)
    k, n = 5, 32
    raw_vals = (nc.edge_values(field) * 6)[:n]
    raw = b"".join(v.to_bytes(32, "little") for v in raw_vals)
    for normal in (0, 1):
        vals = nc.decode(field, raw, normal)
        for kind in range(4):
            got = run(ht, field, k, 2, kind, normal, raw, n)
            assert got == nc.encode(field, nc.transform(field, k, kind, vals), normal)
    x = nc.random_values(field, n, 77)
    one = nc.encode(field, [1], False)
    assert run(ht, field, k, 3, nc.COSET_FORWARD, 0, nc.encode(field, x, False), n, offset=one) == run(ht, field, k, 3, nc.FORWARD, 0, nc.encode(field, x, False), n)
    assert run(ht, field, k, 3, nc.COSET_INVERSE, 0, nc.encode(field, x, False), n, offset=one) == run(ht, field, k, 3, nc.INVERSE, 0, nc.encode(field, x, False), n)
    off = 0xC0FFEE * 31 % r
    for kind in (nc.COSET_FORWARD, nc.COSET_INVERSE):
        got = run(ht, field, k, 3, kind, 0, nc.encode(field, x, False), n, offset=nc.encode(field, [off], False))
        assert got == nc.encode(field, nc.transform(field, k, kind, x, offset=off), False)
    no_check_failures(ht)


@pytest.mark.parametrize("field", FIELDS)
def test_wide_passes(ht, field):
    """pass_log 7 .. 10 (the default is 8): tiles of 8, 4, 2 and 1 columns, the deepest butterfly chains the bound analysis covers"""
    for k, pass_log in ((7, 7), (10, 8), (12, 8), (11, 9), (10, 10), (13, 10)):
        for kind in (nc.FORWARD, nc.COSET_INVERSE):
            x, y = model(field, k, kind, 0, 1 << k, 0xB16)
            got = run(ht, field, k, pass_log, kind, 0, nc.encode(field, x, False), 1 << k)
            assert got == nc.encode(field, y, False), (k, pass_log, kind)
    no_check_failures(ht)
