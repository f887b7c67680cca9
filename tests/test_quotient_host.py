"""CPU: the rows of the Plonk quotient and the linear combination of csrc/quotient.hpp, compiled for the host with the limb-bound
checker armed (libmsm_hosttest.so, ht_quotient_*: the chain of launches the engine runs, a block's loops in order), against the Python
big-integer model of tests/quotient_cases.py.  Both fields, both element forms, inversion tiles of 16 and 1024 elements; every row of
every case is compared."""
import ctypes
import os
import subprocess
import sys

import pytest

import ntt_cases as nc
import poly_cases as pc
import quotient_cases as qc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    cp, ci, cu = ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.ht_quotient_rows.argtypes = [ci, cu, cu, cu, cu, cu, U64] + [cp] * 11
    lib.ht_quotient_linear_combination.argtypes = [ci, cu, cu, ctypes.POINTER(cp), ctypes.POINTER(U64), cp, ci, cp]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def no_check_failures(ht):
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def rows_call(ht, c, normal, tile_log, stride):
    enc = lambda vals: nc.encode(c.field, vals, normal)
    out = ctypes.create_string_buffer(c.M * 32)
    rc = ht.ht_quotient_rows(nc.FIELD_IDS[c.field], c.K, c.n.bit_length() - 1, tile_log, normal, c.m, U64(stride), c.columns(c.wires, stride),
                             c.columns(c.sigmas, stride), None if c.selectors is None else c.columns(c.selectors, stride), pc.to_raw(c.raw_z(normal)),
                             None if c.pi is None else pc.to_raw(c.pi), enc(c.ks), enc([c.alpha]), enc([c.beta]), enc([c.gamma]),
                             None if c.offset is None else enc([c.offset]), out)
    assert rc == 0
    return out.raw


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_quotient_rows(ht, field, normal):
    for name, c, tile_logs in qc.row_cases(field):
        want = nc.encode(field, c.model(normal), normal)
        for tile_log in tile_logs:
            for stride in (c.M, c.M + 3):
                got = rows_call(ht, c, normal, tile_log, stride)
                bad = [i for i in range(c.M) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
                assert not bad, (name, tile_log, stride, bad[:8])
        no_check_failures(ht)


@pytest.mark.parametrize("field", FIELDS)
def test_quotient_rows_refuse_an_offset_that_zeroes_the_vanishing_polynomial(ht, field):
    """an offset of 0 (as bytes of 0 and of r) and offsets inside the quotient domain, whose n-th power is a root of unity of order
    `ratio`: -1, as the engine refuses them -- the check that keeps x - 1 away from 0"""
    r = nc.modulus(field)
    c = qc.Rows(field, 5, 4, 5, 77)
    om = nc.root_of_unity(field, 5)
    for offset in (0, r, 1, pow(om, 3, r), pow(om, 31, r)):    # (g^n in H_ratio exactly when g is in H_M: the fourth roots of 1 are)
        enc = lambda vals: nc.encode(field, vals, 0)
        out = ctypes.create_string_buffer(c.M * 32)
        raw_off = offset.to_bytes(32, "little") if offset in (0, r) else enc([offset])
        rc = ht.ht_quotient_rows(nc.FIELD_IDS[field], c.K, 2, 4, 0, c.m, U64(c.M), c.columns(c.wires, c.M), c.columns(c.sigmas, c.M),
                                 c.columns(c.selectors, c.M), pc.to_raw(c.raw_z(0)), pc.to_raw(c.pi), enc(c.ks), enc([c.alpha]), enc([c.beta]),
                                 enc([c.gamma]), raw_off, out)
        assert rc == -1, offset


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_linear_combination(ht, field, normal):
    r = nc.modulus(field)
    for cols, coeffs in qc.lincomb_cases(field):
        m = len(cols)
        want = nc.encode(field, qc.ref_lincomb([pc.values(field, c, normal) for c in cols], coeffs, r), normal)
        n = len(want) // 32
        bufs = [ctypes.create_string_buffer(pc.to_raw(c), max(len(c), 1) * 32) for c in cols]
        ptrs = (ctypes.c_char_p * m)(*[ctypes.cast(b, ctypes.c_char_p) for b in bufs])
        lens = (U64 * m)(*[len(c) for c in cols])
        for in_place in (0, 1):
            out = ctypes.create_string_buffer(b"\x55" * (max(n, 1) * 32), max(n, 1) * 32)
            assert ht.ht_quotient_linear_combination(nc.FIELD_IDS[field], normal, m, ptrs, lens, nc.encode(field, coeffs, normal), in_place, out) == 0
            assert out.raw[:n * 32] == want, (m, [len(c) for c in cols], in_place)
            if n == 0:
                assert out.raw == b"\x55" * 32          # nothing is written
    no_check_failures(ht)


def test_bounds_tool_quotient_mode():
    """the chain's largest column stays below 2^64 for both fields, every other margin is positive, and the other modes print what they
    printed"""
    tool = os.path.join(ROOT, "tools", "limb_bounds_fr.py")
    r = subprocess.run([sys.executable, tool, "--quotient"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all margins positive" in r.stdout and "BAD" not in r.stdout
    for what in ("Bls12_377_Fr29", "Bls12_381_Fr29", "the chain's largest column against 2^64", "gate + t_perm1 times 1 / Z_H", "linear combination of 32 columns"):
        assert what in r.stdout, what
    for mode in ((), ("--scan",), ("--poly",)):
        plain = subprocess.run([sys.executable, tool, *mode], capture_output=True, text=True)
        assert plain.returncode == 0 and "quotient.hpp" not in plain.stdout
