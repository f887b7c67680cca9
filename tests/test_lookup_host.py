"""CPU: the lookup table, plookup's sorted vector and the logUp sum of csrc/lookup.hpp, compiled for the host with the limb-bound checker
armed (libmsm_hosttest.so, ht_lookup and ht_logup_sum: the same bodies lane by lane, the atomics as plain sequential operations), against
the integer model of tests/lookup_cases.py.  Both fields, both forms, every case the GPU tests run.  Also here: the quality of the hash
as a condition, a plookup identity computed from the library's s that shares nothing with the model, and tests/asan_lookup.cpp."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import lookup_cases as lc
import ntt_cases as nc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    vp, ci, cu, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_char_p
    lib.ht_lookup.argtypes = [ci, cu, vp, U64, vp, U64, vp, vp, vp, vp, vp]
    lib.ht_logup_sum.argtypes = [ci, cu, cu, cp, cp, cp, cu, U64, U64, cp, vp, vp, vp]
    lib.ht_lookup_hash.argtypes = [cp]
    lib.ht_lookup_hash.restype = cu
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


PATTERN = 0xA5


def host_lookup(ht, field, normal, table_raw, values_raw):
    """every output of the host build; s is pre-filled with a pattern"""
    n_t, n_f = len(table_raw) // 32, len(values_raw) // 32
    t = np.frombuffer(table_raw, dtype=np.uint8).copy()
    v = np.frombuffer(values_raw, dtype=np.uint8).copy() if n_f else np.zeros(1, dtype=np.uint8)
    mult = np.zeros(n_t * 32, dtype=np.uint8)
    index = np.zeros(max(n_f, 1), dtype=np.uint32)
    stats, info = np.zeros(2, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    s = np.full((n_t + n_f) * 32, PATTERN, dtype=np.uint8)
    rc = ht.ht_lookup(nc.FIELD_IDS[field], normal, t.ctypes.data, n_t, v.ctypes.data if n_f else None, n_f, mult.ctypes.data, index.ctypes.data,
                      stats.ctypes.data, s.ctypes.data, info.ctypes.data)
    assert rc == 0
    return {"mult": mult.tobytes(), "index": index[:n_f].tolist(), "missing": int(stats[0]), "first": int(stats[1]), "sorted": s.tobytes(),
            "slots": int(info[0]), "distinct": int(info[1]), "max_probe": int(info[2])}


def check_case(got, c):
    want = c.expected
    assert got["index"] == want["index"], c.name
    assert got["mult"] == want["mult"], c.name
    assert (got["missing"], got["first"]) == (want["missing"], want["first"]), c.name
    if want["sorted"] is None:
        assert got["sorted"] == bytes([PATTERN]) * len(got["sorted"]), c.name   # nothing was written
    else:
        assert got["sorted"] == want["sorted"], c.name


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_every_case_against_the_model(ht, field, normal):
    for c in lc.cases(field, normal).values():
        got = host_lookup(ht, field, normal, c.table_raw, c.values_raw)
        check_case(got, c)
        slots = 2
        while slots < 2 * c.n_t:
            slots *= 2
        assert got["slots"] == slots and got["distinct"] == len(set(lc.model_count(field, c.table_raw, c.table_raw)[0])), c.name
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_the_cases_reach_what_they_are_named_for():
    for field in FIELDS:
        cs = lc.cases(field, 0)
        r = nc.modulus(field)
        assert cs["dup_1000_equal"].expected["counts"] == [77] + [0] * 999
        assert cs["missing_first"].expected["first"] == 0 and cs["missing_first"].expected["missing"] == 1
        assert cs["missing_last"].expected["first"] == cs["missing_last"].n_f - 1
        assert cs["missing_many"].expected["missing"] == 120 and cs["missing_none"].expected["missing"] == 0
        assert all(v >= r for v in lc.rows(cs["table_v_values_v_plus_r"].values_raw)) and cs["table_v_values_v_plus_r"].expected["missing"] == 0
        assert cs["skew_all_on_last"].expected["counts"][-1] == 1 << 16
        assert cs["block_edges"].n_t == (1 << 16) + 1 and cs["block_edges"].n_f == (1 << 16) + 3
        if field == "bls12_381":
            assert all(v >= 2 * r for v in lc.rows(cs["values_v_plus_2r"].values_raw)) and cs["values_v_plus_2r"].expected["missing"] == 0
        kmax = 13 if field == "bls12_377" else 2
        assert (kmax + 1) * r + (1 << 200) > 1 << 256                      # no larger multiple fits
        c = cs["values_v_plus_%dr" % kmax if kmax != 2 else "values_v_plus_2r_again"]
        assert all(v >= kmax * r for v in lc.rows(c.values_raw)) and c.expected["missing"] == 0
        c = cs["table_v_plus_%dr_values_v" % kmax]
        assert all(v >= kmax * r for v in lc.rows(c.table_raw)) and c.expected["missing"] == 0
        assert all(v < r for v in lc.rows(c.expected["sorted"]))           # s is canonical in the model, so byte equality checks it
        c = cs["one_residue_every_multiple"]
        assert c.n_t == kmax + 1 and c.expected["counts"] == [3 * (kmax + 1)] + [0] * kmax
        if field == "bls12_377":
            assert "values_v_plus_8r" in cs and "table_v_plus_8r_values_v" in cs


@pytest.mark.parametrize("field", FIELDS)
def test_medium_against_numpy_unique(ht, field):
    table, values, pick = lc.medium_case(field, 0)
    got = host_lookup(ht, field, 0, table.tobytes(), values.tobytes())
    uniq, inverse, counts = np.unique(values, axis=0, return_inverse=True, return_counts=True)
    assert got["missing"] == 0 and got["index"] == pick.tolist()
    mult = np.frombuffer(got["mult"], dtype=np.uint8).reshape(-1, 32)
    want = np.bincount(pick, minlength=1 << 16)
    assert nc.decode(field, got["mult"], 0) == want.tolist()
    assert int(want.sum()) == 1 << 20 and len(uniq) == int((want > 0).sum()) and mult.shape[0] == 1 << 16
    s = np.frombuffer(got["sorted"], dtype=np.uint32).reshape(-1, 8)
    assert np.array_equal(s, np.repeat(table, 1 + want, axis=0))


@pytest.mark.parametrize("field", FIELDS)
def test_hash_quality_is_a_condition(ht, field):
    """eight families of 2^16 keys, family w varying ONLY in 32-bit word w of the canonical key: a hash that ignores a word puts a whole
    family into one chain (max_probe about n_t); a mixing hash at load <= 1/2 stays in the tens.  The cap is n_t / 16."""
    n_t = 1 << 16
    rng = random.Random(11)
    vary = np.arange(n_t, dtype=np.uint64)
    seen = []
    for kind in ("sequential", "spread"):
        for w in range(8):
            base = np.array([rng.getrandbits(32) for _ in range(8)], dtype=np.uint32)
            base[7] &= (1 << 27) - 1                       # canonical: the top word of r is above 2^28 for both fields
            table = np.tile(base, (n_t, 1))
            table[:, w] = (vary if kind == "sequential" or w == 7 else (vary * 2654435761) & 0xFFFFFFFF).astype(np.uint32)
            assert len(np.unique(table[:, w])) == n_t
            got = host_lookup(ht, field, 1, table.tobytes(), table[:16].tobytes())
            assert got["distinct"] == n_t and got["index"] == list(range(16))
            assert got["max_probe"] <= n_t // 16, (kind, w, got["max_probe"])
            seen.append(got["max_probe"])
    print("max_probe per family (%s): %s" % (field, seen))


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_plookup_identity_from_the_librarys_s(ht, field, normal):
    """prod (1 + b)(g + f_j) * prod (g (1 + b) + t_i + b t_(i+1)) == prod (g (1 + b) + s_i + b s_(i+1)) in integers, n = 64: with
    |t| = n and |f| = n - 1, s has 2n - 1 elements and h1 = s[:n], h2 = s[n-1:] overlap in one; this shares nothing with the model"""
    n = 64
    rng = random.Random(3)
    r = nc.modulus(field)
    t = sorted({rng.randrange(r) for _ in range(n + 8)})[:n]
    f = [t[rng.randrange(n)] for _ in range(n - 1)]
    got = host_lookup(ht, field, normal, nc.encode(field, t, normal), nc.encode(field, f, normal))
    assert got["missing"] == 0
    s = nc.decode(field, got["sorted"], normal)
    assert len(s) == 2 * n - 1
    b, g = rng.randrange(r), rng.randrange(r)
    lhs = pow(1 + b, n - 1, r)
    for x in f:
        lhs = lhs * (g + x) % r
    for i in range(n - 1):
        lhs = lhs * (g * (1 + b) + t[i] + b * t[i + 1]) % r
    h1, h2 = s[:n], s[n - 1:]
    rhs = 1
    for h in (h1, h2):
        for i in range(n - 1):
            rhs = rhs * (g * (1 + b) + h[i] + b * h[i + 1]) % r
    assert lhs == rhs
    # one value changed to another table entry breaks it
    s2 = list(s)
    at = next(i for i in range(1, len(s)) if s[i] != s[i - 1])
    s2[at] = s[at - 1]
    bad = 1
    for h in (s2[:n], s2[n - 1:]):
        for i in range(n - 1):
            bad = bad * (g * (1 + b) + h[i] + b * h[i + 1]) % r
    assert bad != lhs


def host_logup(ht, field, normal, case, m, stride, n, helpers, tile_log=10):
    out, total = ctypes.create_string_buffer(max(n, 1) * 32), ctypes.create_string_buffer(32)
    hb = ctypes.create_string_buffer((m + 1) * n * 32) if helpers else None
    rc = ht.ht_logup_sum(nc.FIELD_IDS[field], tile_log, normal, case["table"], case["mult"], case["values"], m, stride, n, case["beta"], out, total, hb)
    assert rc == 0
    return out.raw[:n * 32], total.raw, hb.raw if helpers else None


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_logup_against_the_model(ht, field, normal):
    zero = bytes(32)
    for n in (1, 8, 1025):
        for m in (1, 8):
            for stride in (n, n + 3):
                case = lc.logup_case(field, normal, n, m, stride, 1)
                want = lc.model_logup(field, case["table"], case["mult"], case["values"], m, stride, n, case["beta"], normal)
                for tile_log in (4, 10):
                    got = host_logup(ht, field, normal, case, m, stride, n, True, tile_log)
                    assert got == want, (n, m, stride, tile_log)
                assert host_logup(ht, field, normal, case, m, stride, n, False)[:2] == want[:2]
                assert want[1] == zero                       # the multiset relation holds
                # one multiplicity changed by one: the total is not zero
                counts = list(case["counts"])
                counts[0] += 1
                off = dict(case, mult=nc.encode(field, counts, normal))
                got = host_logup(ht, field, normal, off, m, stride, n, False)
                assert got[1] != zero and got[1] == lc.model_logup(field, off["table"], off["mult"], off["values"], m, stride, n, off["beta"], normal)[1]
    # a zero denominator contributes 0
    case = lc.logup_case(field, normal, 8, 2, 8, 2, zero_den=True)
    want = lc.model_logup(field, case["table"], case["mult"], case["values"], 2, 8, 8, case["beta"], normal)
    assert host_logup(ht, field, normal, case, 2, 8, 8, True) == want
    assert want[2][(2 * 8 + 3) * 32:(2 * 8 + 4) * 32] == zero
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_end_to_end_multiplicities_into_logup(ht):
    """LookupTable -> multiplicities -> logup_sum on the host build: the total is zero from the library's own multiplicities"""
    for field in FIELDS:
        for normal in (0, 1):
            n = 100
            rng = random.Random(8)
            t = lc.distinct_small(n, 90, rng)
            f = [t[rng.randrange(n)] for _ in range(n)]
            traw, fraw = nc.encode(field, t, normal), nc.encode(field, f, normal)
            mult = host_lookup(ht, field, normal, traw, fraw)["mult"]
            case = {"table": traw, "mult": mult, "values": fraw, "beta": nc.encode(field, [rng.randrange(1 << 200)], normal)}
            assert host_logup(ht, field, normal, case, 1, n, n, False)[1] == bytes(32)


def test_asan_program(built, tmp_path):
    """tests/asan_lookup.cpp, a program with its own main over the same host code, built with -fsanitize=address,undefined and run as it
    is (no Python in the process, nothing preloaded): exact-size heap buffers, so a read or write past index_out (n_f u32), s_out
    (n_t + n_f elements), helpers ((m + 1) n elements), the slots or the scan levels is an error"""
    exe = str(tmp_path / "asan_lookup")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "asan_lookup.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-1000:] + r.stderr[-3000:]
