"""CPU: the expression compiler and the interpreter of csrc/expr.hpp, compiled for the host with the limb-bound checker armed
(libmsm_hosttest.so, ht_expr: the same expr_row with one lane's slots in a plain array), against the big-integer evaluator of
tests/expr_cases.py.  Both fields: random DAGs with shared sub-expressions, the chains that force reductions, SQR towers, the slot limit
and one above it, edge-value inputs, rotations that wrap both ways, periodic columns, odd lengths, both forms.  Also here:
tests/asan_expr.cpp."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import expr_cases as xc
import ntt_cases as nc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")
U64 = ctypes.c_uint64
INFO = ("nodes", "instructions", "slots", "products", "reduces", "lds_bytes", "used_cols", "rot0_only")


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    vp, ci, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    lib.ht_expr.argtypes = [ci, cu, vp, U64, vp, U64, U64, U64, vp, vp, U64, U64, vp, vp, vp, vp, U64]
    lib.ht_expr_max_slots.restype = cu
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def host_expr(ht, field, normal, case, cols_raw=None, chals=(), length=0):
    """(rc, message, info, out bytes or None)"""
    flat = np.array(case.flat(), dtype=np.uint32)
    consts = np.frombuffer(nc.encode(field, case.consts, True) if case.consts else b"\0" * 32, dtype=np.uint8).copy()   # plain integers
    info = np.zeros(8, dtype=np.uint64)
    msg = ctypes.create_string_buffer(256)
    keep, ptrs, lens, out, cb = [], None, None, None, None
    if cols_raw is not None:
        keep = [np.frombuffer(c, dtype=np.uint8).copy() for c in cols_raw]
        ptrs = (ctypes.c_void_p * max(len(keep), 1))(*[k.ctypes.data for k in keep])
        lens = (U64 * max(len(keep), 1))(*[len(c) // 32 for c in cols_raw])
        out = np.full(max(length, 1) * 32, 0xA5, dtype=np.uint8)
        cb = np.frombuffer(nc.encode(field, list(chals), normal) if chals else b"\0" * 32, dtype=np.uint8).copy()
    # the constants of create are always given as plain integers here when normal, as images otherwise
    cimg = np.frombuffer(nc.encode(field, case.consts, normal) if case.consts else b"\0" * 32, dtype=np.uint8).copy()
    rc = ht.ht_expr(nc.FIELD_IDS[field], 1 if normal else 0, flat.ctypes.data, len(case.nodes), cimg.ctypes.data, len(case.consts), case.n_chal, case.n_cols,
                    ptrs, lens, length, case.rot_step, cb.ctypes.data if cb is not None else None, out.ctypes.data if out is not None else None,
                    info.ctypes.data, msg, 256)
    del consts
    return rc, msg.value.decode(), dict(zip(INFO, (int(v) for v in info))), (out[:length * 32].tobytes() if out is not None else None)


def run_case(ht, field, normal, case, length):
    raws, chals, want = xc.inputs(case, field, length, normal)
    rc, msg, info, got = host_expr(ht, field, normal, case, raws, chals, length)
    assert rc == 0, (case.name, msg)
    assert got == want, (case.name, field, normal, length)
    return info


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_random_dags(ht, field, normal):
    for case in xc.dags():
        for length in (1, 63, 65):
            run_case(ht, field, normal, case, length)
    run_case(ht, field, normal, xc.random_dag(14, 50), 1000)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("field", FIELDS)
def test_chains_force_reductions(ht, field):
    for case in xc.chains():
        for length in (1, 65):
            info = run_case(ht, field, 0, case, length)
        if case.name != "add_chain200" or field == "bls12_381":
            assert info["reduces"] > 0, (case.name, info)
    # the doubling chain and the SUB chain must force reductions in BOTH fields
    for case in (xc.doubling_chain(64), xc.sub_chain(64)):
        assert host_expr(ht, field, 0, case)[2]["reduces"] > 0
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("field", FIELDS)
def test_sqr_towers_and_a_single_leaf(ht, field):
    for normal in (0, 1):
        info = run_case(ht, field, normal, xc.sqr_tower(24), 63)
        assert info["slots"] == 0                      # a chain lives in the accumulator
        info = run_case(ht, field, normal, xc.single_leaf(), 65)
        assert info["instructions"] == 1 and info["products"] == 2 and info["slots"] == 0
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("field", FIELDS)
def test_slot_limit(ht, field):
    limit = ht.ht_expr_max_slots()
    assert limit == xc.MAX_SLOTS
    at = xc.slot_program(limit - 1)
    rc, msg, info, _ = host_expr(ht, field, 0, at)
    assert rc == 0 and info["slots"] == limit and info["lds_bytes"] == limit * 8 * 4 * 64, (msg, info)
    run_case(ht, field, 0, at, 65)
    run_case(ht, field, 1, at, 1)
    rc, msg, info, _ = host_expr(ht, field, 0, xc.slot_program(limit))
    assert rc == -1 and info["slots"] == limit + 1
    assert "S = %d" % (limit + 1) in msg and "limit is %d" % limit in msg, msg
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_edge_values_rotations_periods_lengths(ht, field, normal):
    for length in (1, 63, 65, 1000):
        run_case(ht, field, normal, xc.edge_program(), length)
        run_case(ht, field, normal, xc.rotation_program(8), length)
        run_case(ht, field, normal, xc.rotation_program(1), length)
    for length in (1, 2, 64, 1000):
        run_case(ht, field, normal, xc.periodic_program((1, 2)), length)
        run_case(ht, field, normal, xc.periodic_program((1, 8)), length)
    run_case(ht, field, normal, xc.wide_program(64), 65)
    run_case(ht, field, normal, xc.long_program(200), 63)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_queries_of_the_compiler(ht):
    """dead nodes cost nothing; a column operand pays a conversion at every use; rotation-0-only columns are known"""
    c = xc.Case("t", [(xc.COL, 0, 0), (xc.COL, 1, xc.u32(1)), (xc.MUL, 0, 1), (xc.SQR, 2, 0), (xc.COL, 0, 0), (xc.ADD, 2, 4)], n_cols=2)
    rc, msg, info, _ = host_expr(ht, "bls12_377", 0, c)
    assert rc == 0, msg
    assert info["nodes"] == 6 and info["instructions"] == 2          # the SQR is dead
    assert info["products"] == 3 + 1 + 1                              # three column uses, the MUL, the result
    assert info["used_cols"] == 0b11 and info["rot0_only"] == 0b01


def test_create_limits(ht):
    def refused(case, word):
        rc, msg, _, _ = host_expr(ht, "bls12_381", 0, case)
        assert rc == -1 and word in msg, (case.name, msg)
    refused(xc.Case("fwd", [(xc.COL, 0, 0), (xc.ADD, 0, 1)]), "topological")
    refused(xc.Case("op", [(9, 0, 0)]), "unknown op")
    refused(xc.Case("col", [(xc.COL, 1, 0)], n_cols=1), "column 1 of 1")
    refused(xc.Case("const", [(xc.CONST, 0, 0)]), "constant 0 of 0")
    refused(xc.Case("chal", [(xc.CHAL, 2, 0)], n_chal=2), "challenge 2 of 2")
    refused(xc.Case("rot", [(xc.COL, 0, xc.u32((1 << 15) + 1))]), "rotation")
    refused(xc.Case("rot", [(xc.COL, 0, xc.u32(-(1 << 15) - 1))]), "rotation")
    refused(xc.Case("cols", [(xc.COL, 0, 0)], n_cols=65), "columns exceed 64")
    refused(xc.Case("chals", [(xc.COL, 0, 0)], n_chal=65), "challenges exceed 64")
    refused(xc.Case("nodes", [(xc.COL, 0, 0)] * 65536), "nodes exceed 65535")
    refused(xc.Case("none", []), "at least one node")
    ok = xc.Case("rot", [(xc.COL, 0, xc.u32(-(1 << 15)))])
    assert host_expr(ht, "bls12_381", 0, ok)[0] == 0


def test_asan_program(built, tmp_path):
    """tests/asan_expr.cpp, a program with its own main over the same host code, built with -fsanitize=address,undefined and run as it is
    (no Python in the process, nothing preloaded): exact-size heap buffers for the nodes, the columns, the challenges and the output, so a
    read past a periodic column or a write past the slots of a program is an error"""
    exe = str(tmp_path / "asan_expr")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "asan_expr.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-1000:] + r.stderr[-3000:]
