"""CPU: y = M z of csrc/sparse.hpp, compiled for the host with the limb-bound checker armed (libmsm_hosttest.so, ht_sparse_apply: the
plan create derives, the coefficients slot by slot and the chain of launches the engine runs, every lane in order), against the Python
big-integer model of tests/sparse_cases.py.  Both fields, both forms of the coefficients and of the call, scan tiles of 16 and 1024
elements; every row of every case is compared."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ntt_cases as nc
import sparse_cases as sp
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    vp, ci, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    lib.ht_sparse_apply.argtypes = [ci, cu, cu, cu, U64, U64, vp, vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.ht_sparse_entries_per_lane.restype = cu
    lib.ht_sparse_block_lanes.restype = cu
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def host_apply(ht, c, create_normal, normal, tile_log):
    rp = np.array(c.row_ptr, dtype=np.uint64)
    ci = np.array(c.col_idx, dtype=np.uint32)
    out = ctypes.create_string_buffer(max(c.rows, 1) * 32)
    rc = ht.ht_sparse_apply(nc.FIELD_IDS[c.field], tile_log, create_normal, normal, c.rows, c.cols, rp.ctypes.data, ci.ctypes.data if c.nnz else None,
                            c.values_raw() if c.nnz else None, c.z_raw(), out)
    assert rc == 0, c.name
    return out.raw[:c.rows * 32]


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_apply_against_the_model(ht, field, normal):
    E, L = ht.ht_sparse_entries_per_lane(), ht.ht_sparse_block_lanes()
    for c in sp.cases(field, E, L):
        for create_normal in (0, 1):
            want = c.expected(create_normal, normal)
            for tile_log in (4, 10) if c.tile4 else (10,):
                got = host_apply(ht, c, create_normal, normal, tile_log)
                bad = [i for i in range(c.rows) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
                assert not bad, (c.name, create_normal, tile_log, bad[:8])
        assert ht.ht_check_failures() == 0, (c.name, ht.ht_first_failure())


def test_the_cases_reach_what_they_are_named_for(ht):
    """the generator against the constants of the kernels: a row ends on a lane and on a block boundary, one entry before and one
    after; one row crosses several lanes from a first to a last entry; the prefix sum over the lanes gets a second and a third level"""
    E, L = ht.ht_sparse_entries_per_lane(), ht.ht_sparse_block_lanes()
    cs = {c.name: c for c in sp.cases("bls12_381", E, L)}
    ends = set(cs["short rows that end at, before and after a lane boundary"].row_ptr)
    assert {E, 2 * E - 1, 3 * E + 1} <= ends
    ends = set(cs["short rows that end at, before and after a block boundary"].row_ptr)
    assert {E * L, 2 * E * L - 1, 3 * E * L + 1} <= ends
    assert cs["a row from a lane's first entry to another lane's last"].row_ptr[1:3] == [E, 4 * E]
    assert cs["one row of %d" % (256 * E + 3)].nnz > 256 * E and cs["one row of %d" % (16 * E + 1)].tile4
    c = cs["power-law row lengths, 3000 rows"]
    lens = [b - a for a, b in zip(c.row_ptr, c.row_ptr[1:])]
    assert c.rows == 3000 and max(lens) > 4 * E and sorted(lens)[len(lens) // 2] <= 3 and 0 in lens
    assert c.nnz % E
    d = cs["duplicate columns in a row"]
    assert any(len(set(d.col_idx[a:b])) < b - a for a, b in zip(d.row_ptr, d.row_ptr[1:]))


def test_host_build_refuses_a_broken_structure(ht):
    rp = np.array([0, 2, 1], dtype=np.uint64)
    ci = np.array([0, 0], dtype=np.uint32)
    out = ctypes.create_string_buffer(64)
    assert ht.ht_sparse_apply(1, 10, 0, 0, 2, 1, rp.ctypes.data, ci.ctypes.data, bytes(64), bytes(32), out) == -1


def test_bounds_tool_sparse_mode(ht):
    """every margin is positive, the chain's largest column stays below 2^64 for both fields, the tool counts the entries a lane sums
    as the kernels do, and the other modes print what they printed"""
    tool = os.path.join(ROOT, "tools", "limb_bounds_fr.py")
    r = subprocess.run([sys.executable, tool, "--sparse"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all margins positive" in r.stdout and "BAD" not in r.stdout
    for what in ("Bls12_377_Fr29", "Bls12_381_Fr29", "the chain's largest column against 2^64", "the running sum as the first operand",
                 "a crossing row: bend + 4r - bstart", "%d entries a lane" % ht.ht_sparse_entries_per_lane()):
        assert what in r.stdout, what
    cols = [int(m) for m in re.findall(r"largest column: (\d+)", r.stdout)]
    assert len(cols) == 2 and all(0 < c < 1 << 64 for c in cols)
    for mode in ((), ("--scan",), ("--poly",), ("--quotient",)):
        plain = subprocess.run([sys.executable, tool, *mode], capture_output=True, text=True)
        assert plain.returncode == 0 and "sparse.hpp" not in plain.stdout
