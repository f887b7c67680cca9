"""CPU: fix_variables, the eq table and the sumcheck round of csrc/mle.hpp, compiled for the host with the limb-bound checker armed
(libmsm_hosttest.so, ht_mle_*: the chains of launches the engine runs, every block lane by lane), against the Python big-integer model
of tests/mle_cases.py.  Both fields, both forms of the call, tiles of 16 and 1024 elements; random values, all r - 1, zeros and the byte
patterns r, 2r and 2^256 - 1 read as residues; every output element is compared."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mle_cases as mc
import ntt_cases as nc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    vp, ci, cu, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_char_p
    lib.ht_mle_fix.argtypes = [ci, cu, cu, cu, cu, cp, cp, cp]
    lib.ht_mle_eq.argtypes = [ci, cu, cu, cp, cp]
    lib.ht_mle_round.argtypes = [ci, cu, cu, cu, cu, cp, cu, cp, vp, vp, cp, cp, cp]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def host_round(ht, c, normal, fused, tile_log):
    """(evals as residues, folded tables as bytes or None, launches)"""
    d = mc.degree(c.terms())
    nfs = np.array([len(f) for f in c.factors], dtype=np.uint32)
    fac = np.zeros((len(c.factors), mc.MAX_FACTORS), dtype=np.uint32)
    for j, f in enumerate(c.factors):
        fac[j, :len(f)] = f
    half = (1 << c.nv) // 2
    folded = ctypes.create_string_buffer(max(c.m * half * 32, 32)) if fused else None
    evals = ctypes.create_string_buffer(32 * (d + 1))
    levels = ht.ht_mle_round(nc.FIELD_IDS[c.field], tile_log, normal, c.m, c.nv, b"".join(mc.raw_bytes(t) for t in c.tables), len(c.coeffs),
                             nc.encode(c.field, c.coeffs, normal), nfs.ctypes.data, fac.ctypes.data,
                             mc.raw_bytes([c.r_prev]) if fused else None, folded, evals)
    assert levels >= 1, c.name
    got = nc.decode(c.field, evals.raw, normal)
    ftabs = [folded.raw[i * half * 32:(i + 1) * half * 32] for i in range(c.m)] if fused else None
    return got, ftabs, levels


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_fix_variables_against_the_model(ht, field, normal):
    r = nc.modulus(field)
    rng = random.Random(0x4D4C45 + normal)
    for tile_log in (4, 10):
        for nv, k in mc.fix_cases(tile_log):
            for name, only in mc.fills(field) if (nv, k) in ((tile_log + 1, tile_log + 1), (2, 1)) else [("random", None)]:
                table = mc.raw_values(field, 1 << nv, rng, only)
                point = mc.raw_values(field, k, rng, only)
                want = nc.encode(field, mc.fix_variables(r, nc.decode(field, mc.raw_bytes(table), normal), nc.decode(field, mc.raw_bytes(point), normal)), normal)
                out = ctypes.create_string_buffer(32 << (nv - k))
                assert ht.ht_mle_fix(nc.FIELD_IDS[field], tile_log, normal, nv, k, mc.raw_bytes(table), mc.raw_bytes(point) if k else None, out) == 0
                assert out.raw == want, (tile_log, nv, k, name)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_eq_table_against_the_model(ht, field, normal):
    r = nc.modulus(field)
    rng = random.Random(0xE9 + normal)
    for k in (0, 1, 2, 3, 6, 9, 10):
        for name, only in mc.fills(field) if k == 3 else [("random", None)]:
            point = mc.raw_values(field, k, rng, only)
            want = mc.eq_table(r, nc.decode(field, mc.raw_bytes(point), normal))
            out = ctypes.create_string_buffer(32 << k)
            assert ht.ht_mle_eq(nc.FIELD_IDS[field], normal, k, mc.raw_bytes(point) if k else None, out) == 0
            assert out.raw == nc.encode(field, want, normal), (k, name)
            assert sum(want) % r == 1
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_sumcheck_round_against_the_model(ht, field, normal):
    rng = random.Random(0x5C + normal)
    for name in ("one table of degree 1", "spartan", "hyperplonk", "worst"):
        for nv, tile_log in ((1, 10), (2, 4), (5, 4), (7, 4), (7, 10)):
            for fused in (False, True):
                if fused and nv < 2:
                    continue
                c = mc.RoundCase(field, name, nv, rng)
                want, wfold = c.expected(normal, fused)
                got, gfold, _ = host_round(ht, c, normal, fused, tile_log)
                assert got == want, (name, nv, tile_log, fused)
                assert gfold == wfold, (name, nv, tile_log, fused)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("field", FIELDS)
def test_the_worst_term_list_on_every_fill(ht, field):
    """8 terms of 5 factors over 12 tables, one a fifth power, on all r - 1, zeros and the patterns r, 2r, 2^256 - 1: the lane
    accumulators carry 32 products and the block tree runs two and three levels under the checker"""
    rng = random.Random(0xF111)
    for fill, only in mc.fills(field):
        for nv, fused in ((6, False), (7, True)):
            c = mc.RoundCase(field, "worst", nv, rng, only)
            assert len(c.coeffs) == mc.MAX_TERMS and c.m == mc.MAX_TABLES and [0] * 5 in c.factors
            want, wfold = c.expected(0, fused)
            got, gfold, levels = host_round(ht, c, 0, fused, 4)
            assert got == want and gfold == wfold, (fill, nv, fused)
            assert levels == 2
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_the_reduction_levels_are_reached(ht):
    rng = random.Random(3)
    for nv, levels in ((5, 1), (9, 2), (10, 3)):
        c = mc.RoundCase("bls12_381", "spartan", nv, rng)
        got, _, lv = host_round(ht, c, 0, False, 4)
        assert lv == levels and got == c.expected(0, False)[0]
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_host_build_refuses_a_bad_term_list(ht):
    c = mc.RoundCase("bls12_381", "spartan", 2, random.Random(1))
    c.factors[0][0] = c.m
    nfs = np.array([len(f) for f in c.factors], dtype=np.uint32)
    fac = np.zeros((len(c.factors), mc.MAX_FACTORS), dtype=np.uint32)
    for j, f in enumerate(c.factors):
        fac[j, :len(f)] = f
    ev = ctypes.create_string_buffer(32 * 6)
    assert ht.ht_mle_round(1, 10, 0, c.m, c.nv, b"".join(mc.raw_bytes(t) for t in c.tables), len(c.coeffs), nc.encode(c.field, c.coeffs, 0),
                           nfs.ctypes.data, fac.ctypes.data, None, None, ev) == -1


def test_bounds_tool_mle_mode():
    """every margin is positive for both fields, the chain named in the issue is carried out (the fold, the extrapolation to t = 5,
    five-factor products, the lane accumulators with their carry passes, the block tree), and the other modes print what they printed"""
    tool = os.path.join(ROOT, "tools", "limb_bounds_fr.py")
    r = subprocess.run([sys.executable, tool, "--mle"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all margins positive" in r.stdout and "BAD" not in r.stdout
    for what in ("Bls12_377_Fr29", "Bls12_381_Fr29", "the fold (1 - r) x + r y", "e_5", "factor 5 of a term at t = 5", "the lane accumulator, add 32",
                 "the block tree, level 8", "the chain's largest column against 2^64"):
        assert what in r.stdout, what
    cols = [int(m) for m in re.findall(r"largest column: (\d+)", r.stdout)]
    assert len(cols) == 2 and all(0 < c < 1 << 64 for c in cols)
    for mode in ((), ("--sparse",)):
        plain = subprocess.run([sys.executable, tool, *mode], capture_output=True, text=True)
        assert plain.returncode == 0 and "mle.hpp" not in plain.stdout


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/asan_mle.cpp, a program with its own main over the same host code, built with -fsanitize=address,undefined and run as it
    is (no Python in the process, nothing preloaded): exact-size heap buffers, so a read or write past a table, a folded table, the
    work memory or the partial rows is an error"""
    exe = str(tmp_path / "asan_mle")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "asan_mle.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-1000:] + r.stderr[-3000:]
