"""CPU: the per-element steps and the chains of launches of csrc/scan.hpp, compiled for the host with the limb-bound checker armed
(libmsm_hosttest.so, ht_scan_*: a block's loops run in order), against Python big integers.  Both fields, both element forms, tiles of
16, 32 and 1024 elements; the lengths cross all three levels of the scans below 1100 elements at the small tiles."""
import ctypes
import os
import subprocess
import sys

import pytest

import ntt_cases as nc
import poly_cases as pc
import scan_cases as sc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    cp, ci, cu = ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.ht_scan_scan.argtypes = [ci, cu, cu, cu, ci, cp, U64, cp, cp]
    lib.ht_scan_permutation_product.argtypes = [ci, cu, cu, cu, cu, U64, cp, cp, cp, cp, cp, cp, cp]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def no_check_failures(ht):
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def lengths(tile_log):
    return pc.lengths(tile_log) if tile_log < 10 else [0, 1, 1023, 1024, 1025, 3 * 1024 + 5]


def vectors(field, n, tile_log, op):
    """the raw inputs of one length: with the multiples of r planted, and for the product also without any zero and with a single one"""
    out = [(sc.vector(field, n, tile_log, 0xC0 + n), None)]
    if op == sc.PRODUCT:
        out.append((sc.vector(field, n, tile_log, 0xD0 + n, zeros=False), None))
        out.append(sc.single_zero(field, n, tile_log, 0xE0 + n, which=n))
    return out


@pytest.mark.parametrize("tile_log", [4, 5, 10])
@pytest.mark.parametrize("op", [sc.PRODUCT, sc.SUM])
@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_scan(ht, field, normal, op, tile_log):
    r, fid = nc.modulus(field), nc.FIELD_IDS[field]
    identity = nc.encode(field, [1 if op == sc.PRODUCT else 0], normal)
    for n in lengths(tile_log):
        for raw, zero_at in vectors(field, n, tile_log, op):
            vals = pc.values(field, raw, normal)
            for inclusive in (0, 1):
                want, want_total = sc.ref_scan(vals, op, inclusive, r)
                if zero_at is not None:            # everything after the zero is zero and nothing before it is
                    assert all(v == 0 for v in want[zero_at + 1:]) and want_total == 0 and all(v != 0 for v in want[:zero_at])
                flags = normal | (sc.FLAG_INCLUSIVE if inclusive else 0)
                for in_place in (0, 1):
                    for with_total in (0, 1):
                        out = ctypes.create_string_buffer(b"\x55" * (max(n, 1) * 32), max(n, 1) * 32)
                        tot = ctypes.create_string_buffer(b"\x55" * 32, 32) if with_total else None
                        assert ht.ht_scan_scan(fid, tile_log, flags, op, in_place, pc.to_raw(raw), U64(n), out, tot) == 0
                        assert out.raw[:n * 32] == nc.encode(field, want, normal), (n, inclusive, in_place)
                        if n == 0:
                            assert out.raw == b"\x55" * 32          # nothing else is written
                        if with_total:
                            assert tot.raw == (nc.encode(field, [want_total], normal) if n else identity), (n, inclusive)
    no_check_failures(ht)


def perm_call(ht, p, normal, tile_log, stride):
    fid = nc.FIELD_IDS[p.field]
    out, tot = ctypes.create_string_buffer(p.n * 32), ctypes.create_string_buffer(32)
    rc = ht.ht_scan_permutation_product(fid, p.k, tile_log, normal, p.m, U64(stride), p.columns(p.wires, normal, stride), p.columns(p.sigmas, normal, stride),
                                        nc.encode(p.field, p.ks, normal), nc.encode(p.field, [p.beta], normal), nc.encode(p.field, [p.gamma], normal),
                                        out, tot)
    assert rc == 0
    return out.raw, nc.decode(p.field, tot.raw, normal)[0], tot.raw


@pytest.mark.parametrize("m", [1, 3, 5, 8])
@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_permutation_product(ht, field, normal, m):
    for k, tile_log in ((4, 4), (5, 4), (6, 4), (7, 4), (8, 4), (9, 4), (11, 10)):
        if k == 11 and m not in (1, 5):
            continue                                # (the tile of 1024 changes nothing in the rows: two column counts are enough)
        good = sc.permutation(field, k, m, 0x5000 + 16 * k + m)
        bad = sc.broken(good, k)
        zden, zrow = sc.zero_denominator(good)
        z, total = good.model()
        assert total == 1 and z[0] == 1            # the model itself: the copy constraints hold
        zb, tb = bad.model()
        assert tb != 1
        zz, tz = zden.model()
        assert tz == 0 and zz[zrow] != 0 and all(v == 0 for v in zz[zrow + 1:])
        for stride in (good.n, good.n + 3):
            for p, want_z, want_total in ((good, z, 1), (bad, zb, tb), (zden, zz, 0)):
                raw, tot, tot_raw = perm_call(ht, p, normal, tile_log, stride)
                assert raw == nc.encode(field, want_z, normal), (k, stride)
                assert tot == want_total and tot_raw == nc.encode(field, [want_total], normal), (k, stride)
    no_check_failures(ht)


def test_bounds_tool_scan_mode():
    """the margins of the sum scan (a reduction on every odd step) and of the permutation product's factors are positive for both
    fields, and the other modes print what they printed"""
    tool = os.path.join(ROOT, "tools", "limb_bounds_fr.py")
    r = subprocess.run([sys.executable, tool, "--scan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all margins positive" in r.stdout and "BAD" not in r.stdout
    for what in ("Bls12_377_Fr29", "Bls12_381_Fr29", "sum scan", "permutation product"):
        assert what in r.stdout, what
    plain = subprocess.run([sys.executable, tool], capture_output=True, text=True)
    assert plain.returncode == 0 and "sum scan" not in plain.stdout
