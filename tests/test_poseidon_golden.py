"""CPU: snarkVM's recorded Poseidon results for BLS12-377 Fr (tests/golden/poseidon, one archive of the unchanged files: 14 parameter files, 100 sponge transcripts at rate
2, two samples of the Grain LFSR) against the package's parameter generator and against the big-integer model of
tests/poseidon_cases.py, which the other Poseidon tests use as their oracle; and the sparse form of the partial rounds, built by the
host entry point in the host arithmetic create uses, against the plain permutation on random states."""
import ctypes
import random

import pytest

import ntt_cases as nc
import poseidon_cases as pc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}


@pytest.mark.parametrize("rate", range(2, 9))
def test_the_generator_reproduces_the_parameter_snapshots(ea, rate):
    ark, mds = ea.poseidon_parameters("bls12_377_g1", rate, 17, 8, 31)
    assert ark == pc.snapshot("test_parameters", "rate_%d_ark.snap" % rate)
    assert mds == pc.snapshot("test_parameters", "rate_%d_mds.snap" % rate)
    assert (ark, mds) == pc.parameters("bls12_377", rate)          # the model's own generator agrees


def test_the_generator_reproduces_the_lfsr_samples(ea):
    # PoseidonGrainLFSR::new(false, 253, 3, 8, 31): the first two constants of rate 2
    ark, _ = ea.poseidon_parameters("bls12_377_g1", 2, 17, 8, 31)
    assert [ark[0][0]] == pc.snapshot("test_grain_lfsr", "first_sample.snap")
    assert [ark[0][1]] == pc.snapshot("test_grain_lfsr", "second_sample.snap")
    g = pc.GrainLFSR(253, 3, 8, 31)
    p = nc.modulus("bls12_377")
    assert [g.sample(p)] == pc.snapshot("test_grain_lfsr", "first_sample.snap")
    assert [g.sample(p)] == pc.snapshot("test_grain_lfsr", "second_sample.snap")


def test_the_generator_on_the_other_field_and_with_skipped_matrices(ea):
    for rate, skip in ((2, 0), (3, 1), (8, 2)):
        assert ea.poseidon_parameters("bls12_381_g1", rate, 5, 6, 11, skip) == pc.parameters("bls12_381", rate, 5, 6, 11, skip)
    a0 = ea.poseidon_parameters("bls12_381_g1", 3, 5, 6, 11, 0)
    a1 = ea.poseidon_parameters("bls12_381_g1", 3, 5, 6, 11, 1)
    assert a0[0] == a1[0] and a0[1] != a1[1]
    with pytest.raises(ValueError):
        ea.poseidon_parameters("bls12_381_g1", 9, 5, 6, 11)
    with pytest.raises(ValueError):
        ea.poseidon_parameters("bls12_381_g1", 2, 4, 6, 11)


def test_the_model_reproduces_the_sponge_snapshots():
    m = pc.Model.generated("bls12_377", 2)
    for absorb in range(10):
        for squeeze in range(10):
            assert m.sponge([pc.SPONGE_INPUT] * absorb, squeeze) == pc.snapshot("test_sponge", "absorb_%d_squeeze_%d.snap" % (absorb, squeeze)), (absorb, squeeze)


@pytest.mark.parametrize("rate", [2, 4, 8])
@pytest.mark.parametrize("field", FIELDS)
def test_the_sparse_form_equals_the_dense_permutation(built, field, rate):
    """t = 3, 5, 9: the table pos_build derives, run by the kernel's permutation on the host under the bound checker"""
    lib = pc.host_lib(ROOT)
    sets = [dict(pc.SNARKVM)] + ([dict(pc.ALT_381)] if field == "bls12_381" else [])
    rng = random.Random(0x5BA25E + rate)
    for kw in sets:
        m = pc.Model.generated(field, rate, **kw)
        ark, mds = pc.encode(field, pc.flat(m.ark), False), pc.encode(field, pc.flat(m.mds), False)
        info = (ctypes.c_uint64 * 4)()
        t = rate + 1
        for state in ([0] * t, [m.p - 1] * t, [rng.randrange(m.p) for _ in range(t)], [rng.randrange(m.p) for _ in range(t)]):
            want = m.permute(state)
            for sparse in (0, 1):
                out = ctypes.create_string_buffer(32 * t)
                assert lib.ht_poseidon_permute(nc.FIELD_IDS[field], 1, rate, m.alpha, m.full_rounds, m.partial_rounds, ark, mds, sparse,
                                               pc.encode(field, state, False), out, info) == 0
                assert pc.decode(field, out.raw, False) == want, (kw, sparse)
        # the products of the two forms: the S-boxes, t^2 or 2t - 1 per linear layer, and the scheduled reductions on top
        sbox = bin(m.alpha).count("1") + m.alpha.bit_length() - 2
        dense = m.full_rounds * (t * sbox + t * t) + m.partial_rounds * (sbox + t * t)
        sparse_ = m.full_rounds * (t * sbox + t * t) + m.partial_rounds * (sbox + 2 * t - 1)
        assert dense <= info[0] <= dense + (m.full_rounds + m.partial_rounds) * t
        assert sparse_ <= info[1] <= sparse_ + (m.full_rounds + m.partial_rounds) * t and info[1] < info[0]
        if field == "bls12_377":
            assert info[0] == dense and info[1] <= sparse_ + t         # 2^261 / r = 447: one reduction behind the partial rounds
    assert lib.ht_check_failures() == 0, lib.ht_first_failure()


def test_singular_parameters_are_refused(built):
    """a matrix whose minor without row and column 0 is singular has no sparse form: create says so (-2 from the host entry point)"""
    lib = pc.host_lib(ROOT)
    m = pc.Model.generated("bls12_381", 2)
    mds = [[1, 2, 3], [4, 5, 6], [7, 10, 12]]                          # the minor [[5, 6], [10, 12]] is singular
    out = ctypes.create_string_buffer(32 * 3)
    rc = lib.ht_poseidon_permute(1, 1, 2, 17, 8, 31, pc.encode(m.field, pc.flat(m.ark), False), pc.encode(m.field, pc.flat(mds), False), 1,
                                 bytes(96), out, None)
    assert rc == -2
