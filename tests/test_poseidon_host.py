"""CPU: the kernel bodies of csrc/poseidon.hpp, compiled for the host with the limb-bound checker armed (libmsm_hosttest.so,
ht_poseidon_*: the table create derives, then every lane in order), against the big-integer model of tests/poseidon_cases.py: the 100
recorded transcripts, every shape at which the sponge takes another path at rates 2, 3, 4 and 8, the inputs 0, r - 1, r and 2^256 - 1,
both forms of the call, the sparse form against the dense one, Merkle trees; the bounds proved by tools/limb_bounds_fr.py --poseidon;
and a stand-alone program over the same host code under the sanitizers."""
import os
import random
import subprocess
import sys

import pytest

import ntt_cases as nc
import poseidon_cases as pc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")


@pytest.fixture(scope="module")
def ht(built):
    return pc.host_lib(ROOT)


def test_the_recorded_transcripts(ht):
    m = pc.Model.generated("bls12_377", 2)
    for absorb in range(10):
        for squeeze in range(10):
            want = pc.snapshot("test_sponge", "absorb_%d_squeeze_%d.snap" % (absorb, squeeze))
            for montgomery, sparse in ((True, 1), (False, 0)):
                got, _ = pc.host_hash(ht, m, [[pc.SPONGE_INPUT] * absorb], squeeze, montgomery, sparse)
                assert got == [want], (absorb, squeeze, montgomery, sparse)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("rate", [2, 3, 4, 8])
@pytest.mark.parametrize("field", FIELDS)
def test_every_shape_against_the_model(ht, field, rate):
    m = pc.Model.generated(field, rate)
    rng = random.Random(0x905E1D + rate)
    for in_len in pc.in_lens(rate):
        for n_out in pc.out_lens(rate):
            rows = [[rng.randrange(m.p) for _ in range(in_len)] for _ in range(2)]
            want = [m.sponge(r, n_out) for r in rows]
            montgomery = (in_len + n_out) % 2 == 0
            got, raw1 = pc.host_hash(ht, m, rows, n_out, montgomery, 1)
            assert got == want, (in_len, n_out)
            _, raw0 = pc.host_hash(ht, m, rows, n_out, montgomery, 0)
            assert raw0 == raw1, (in_len, n_out)
    # hash_many's preimage form: the header in front of the row
    rows = [[rng.randrange(m.p) for _ in range(rate + 1)] for _ in range(2)]
    for montgomery in (True, False):
        got, _ = pc.host_hash(ht, m, rows, 2, montgomery, 1, header=m.header(0xD0, rate + 1))
        assert got == [m.hash_many(0xD0, r, 2) for r in rows]
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("field", FIELDS)
def test_edge_inputs_are_read_as_residues(ht, field):
    """0, r - 1, r and 2^256 - 1 in every cell of a row, as they are, in both forms; rate 8 on BLS12-381 carries the most reductions"""
    for rate in (2, 8):
        m = pc.Model.generated(field, rate)
        words = pc.edge_words(field)
        rows = [[w] * (rate + 1) for w in words] + [[words[(i + j) % 4] for j in range(rate + 1)] for i in range(2)]
        raw = pc.raw_words(pc.flat(rows))
        for montgomery in (True, False):
            meant = pc.decode(field, raw, montgomery)
            want = [m.sponge(meant[i * (rate + 1):(i + 1) * (rate + 1)], rate + 1) for i in range(len(rows))]
            for sparse in (1, 0):
                got, out = pc.host_hash(ht, m, rows, rate + 1, montgomery, sparse, raw=raw)
                assert got == want, (rate, montgomery, sparse)
                assert out == pc.encode(field, pc.flat(want), montgomery)          # canonical
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_other_parameters(ht):
    m = pc.Model.generated("bls12_381", 4, **pc.ALT_381)
    rng = random.Random(5)
    rows = [[rng.randrange(m.p) for _ in range(9)] for _ in range(3)]
    for sparse in (0, 1):
        got, _ = pc.host_hash(ht, m, rows, 5, True, sparse)
        assert got == [m.sponge(r, 5) for r in rows]
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("field", FIELDS)
def test_merkle_trees_against_the_model(ht, field):
    import ctypes

    m = pc.Model.generated(field, 4 if field == "bls12_377" else 2)
    rng = random.Random(0x7EE)
    dom = pc.domain_element("AleoMerkle0", m.p)
    for n_leaves, leaf_len in ((1, 1), (2, 4), (3, 1), (5, 4), (9, 0)):
        leaves = [[rng.randrange(m.p) for _ in range(leaf_len)] for _ in range(n_leaves)]
        want, empty = m.merkle(dom, leaves)
        for montgomery, sparse in ((True, 1), (False, 0)):
            out = ctypes.create_string_buffer(32 * len(want))
            rc = ht.ht_poseidon_merkle(nc.FIELD_IDS[field], 1, 0 if montgomery else 1, m.rate, m.alpha, m.full_rounds, m.partial_rounds,
                                       pc.encode(field, pc.flat(m.ark), False), pc.encode(field, pc.flat(m.mds), False), sparse, n_leaves, leaf_len,
                                       pc.encode(field, [dom], montgomery), pc.encode(field, pc.flat(leaves), montgomery) if leaf_len else None, out)
            assert rc == 0
            got = pc.decode(field, out.raw, montgomery)
            assert got == want, (n_leaves, leaf_len, montgomery)
            P = (len(want) + 1) // 2
            assert got[P - 1 + n_leaves:] == [empty] * (P - n_leaves)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_limb_bounds_tool():
    tool = os.path.join(ROOT, "tools", "limb_bounds_fr.py")
    r = subprocess.run([sys.executable, tool, "--poseidon"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all margins positive" in r.stdout and "BAD" not in r.stdout
    for what in ("Bls12_377_Fr29", "Bls12_381_Fr29", "poseidon.hpp", "t = 9", "the first square of an S-box", "products per permutation"):
        assert what in r.stdout, what
    plain = subprocess.run([sys.executable, tool], capture_output=True, text=True)
    assert plain.returncode == 0 and "poseidon.hpp" not in plain.stdout


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/asan_poseidon.cpp, a program with its own main over the same host code, built with -fsanitize=address,undefined and run as
    it is (no Python in the process, nothing preloaded): exact-size heap buffers, so a read or write past the rows, the outputs, the
    table or the tree is an error"""
    exe = str(tmp_path / "asan_poseidon")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                        os.path.join(ROOT, "tests", "asan_poseidon.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-1000:] + r.stderr[-3000:]
