"""CPU: the plain NTT of the CPU oracle (oracle/ntt_oracle.c: 4 x 64-bit CIOS, decimation in time behind a bit reversal, one flat
twiddle table) against the big-integer model of tests/ntt_cases.py at k <= 12 and against Horner at 2^18; then the oracle as the
judge of the host build of csrc/ntt.hpp (libmsm_hosttest.so, the limb-bound checker armed) at k = 15 .. 17, where the two-level
twiddle table has more than one HI entry."""
import ctypes
import os
import random

import numpy as np
import pytest

import ntt_cases as nc
from conftest import ROOT

FIELDS = ("bls12_377", "bls12_381")


def custom_offset(field):
    return 0xC0FFEE * 31 % nc.modulus(field)


def raw_input(field, n, seed):
    """n random 256-bit values (most of them above the modulus), the corners of the input range at both ends"""
    rng = random.Random(seed)
    vals = [rng.getrandbits(256) for _ in range(n)]
    edges = nc.edge_values(field)
    for i, e in enumerate(edges[:n]):
        vals[i] = e
    for i, e in enumerate(edges[:max(0, n - len(edges))]):
        vals[n - 1 - i] = e
    return b"".join(v.to_bytes(32, "little") for v in vals)


def check_against_model(oracle, field, k, kind, normal, reordered, in_len, offset):
    n = 1 << k
    raw = raw_input(field, n, 0x0C1E + 17 * k + kind)
    order = 0 if not reordered else (nc.FLAG_RN if kind & 1 else nc.FLAG_NR)
    vals = nc.decode(field, raw, normal)[:in_len]
    want = nc.encode(field, nc.transform(field, k, kind, vals, offset=offset, order_flags=order), normal)
    off = None if offset is None else nc.encode(field, [offset], normal)
    got = nc.oracle_ntt(oracle, field, k, kind, order | normal, raw, in_len=in_len, offset=off, threads=3)
    assert got.tobytes() == want, (field, k, kind, normal, order, in_len, offset)
    return got


def offsets_of(field, kind):
    return (None, custom_offset(field), 1) if kind & 2 else (None,)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", range(7))
def test_oracle_is_the_model_every_option(oracle, field, k):
    """k <= 6: the full product of kind, form, order, in_len and offset (the generator, a custom one, 1)"""
    n = 1 << k
    for kind in range(4):
        for normal in (0, 1):
            for reordered in (0, 1):
                for in_len in sorted({0, 1, min(n // 2 + 1, n), n}):
                    for offset in offsets_of(field, kind):
                        got = check_against_model(oracle, field, k, kind, normal, reordered, in_len, offset)
                        if offset == 1:   # offset 1 is the plain transform
                            plain = nc.oracle_ntt(oracle, field, k, kind & 1, (nc.FLAG_RN if kind & 1 else nc.FLAG_NR) * reordered | normal,
                                                  raw_input(field, n, 0x0C1E + 17 * k + kind), in_len=in_len)
                            assert np.array_equal(got, plain)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", range(7, 13))
def test_oracle_is_the_model(oracle, field, k):
    """k = 7 .. 12: every kind with every in_len; the form, the order and the offset go round so that each meets each kind"""
    n = 1 << k
    turn = k
    for kind in range(4):
        for in_len in (0, 1, n // 2 + 1, n):
            offs = offsets_of(field, kind)
            check_against_model(oracle, field, k, kind, turn & 1, (turn >> 1) & 1, in_len, offs[turn % len(offs)])
            turn += 1


def test_oracle_refuses_what_the_library_refuses(oracle):
    raw = bytes(64)
    out = ctypes.create_string_buffer(64)
    nc.oracle_ntt(oracle, "bls12_381", 1, 0, 0, raw)   # (binds the argument types)
    call = oracle.oracle_ntt
    assert call(2, 1, 0, 0, None, raw, 2, out, 1) == -1            # field
    assert call(1, 1, 4, 0, None, raw, 2, out, 1) == -1            # kind
    assert call(1, 1, 0, 8, None, raw, 2, out, 1) == -1            # flags
    assert call(1, 1, 1, nc.FLAG_NR, None, raw, 2, out, 1) == -1   # NR belongs to the forward kinds
    assert call(1, 1, 0, nc.FLAG_RN, None, raw, 2, out, 1) == -1   # RN to the inverse kinds
    assert call(1, 1, 0, 0, None, raw, 3, out, 1) == -1            # in_len above n
    assert call(1, 33, 0, 0, None, raw, 2, out, 1) == -1           # above the 2-adicity
    assert call(1, 1, 2, 0, bytes(32), raw, 2, out, 1) == -1       # a zero offset
    assert call(1, 1, 0, 0, raw[:32], raw, 2, out, 1) == -1        # an offset without a coset


# ---- at 2^18 -------------------------------------------------------------------------------------------------------------------------

K18 = 18


@pytest.fixture(scope="module")
def at_2_18(oracle):
    """per field: canonical random input bytes and the oracle's forward and coset forward transforms of them (normal form)"""
    made = {}

    def get(field):
        if field not in made:
            raw = np.random.default_rng(0x18 + nc.FIELD_IDS[field]).integers(0, 256, size=(1 << K18, 32), dtype=np.uint8)
            raw[:, 31] &= 0x0F   # below 2^252: canonical in both fields
            made[field] = (raw, {kind: nc.oracle_ntt(oracle, field, K18, kind, nc.FLAG_NORMAL, raw) for kind in (nc.FORWARD, nc.COSET_FORWARD)})
        return made[field]

    return get


@pytest.mark.parametrize("field", FIELDS)
def test_three_outputs_by_horner_at_2_18(at_2_18, field):
    """out[i] = sum_j x[j] (g omega^i)^j at i = 1, n/2 + 3 and n - 1, plain (g = 1) and over the coset of the generator"""
    n, r = 1 << K18, nc.modulus(field)
    raw, outs = at_2_18(field)
    coeffs = [int.from_bytes(bytes(row), "little") for row in raw]
    omega = nc.root_of_unity(field, K18)
    for kind, g in ((nc.FORWARD, 1), (nc.COSET_FORWARD, nc.generator(field))):
        for i in (1, n // 2 + 3, n - 1):
            e, acc = g * pow(omega, i, r) % r, 0
            for c in reversed(coeffs):
                acc = (acc * e + c) % r
            assert int.from_bytes(bytes(outs[kind][i]), "little") == acc, (kind, i)


@pytest.mark.parametrize("field", FIELDS)
def test_round_trips_at_2_18(oracle, at_2_18, field):
    raw, outs = at_2_18(field)
    assert np.array_equal(nc.oracle_ntt(oracle, field, K18, nc.INVERSE, nc.FLAG_NORMAL, outs[nc.FORWARD]), raw)
    assert np.array_equal(nc.oracle_ntt(oracle, field, K18, nc.COSET_INVERSE, nc.FLAG_NORMAL, outs[nc.COSET_FORWARD]), raw)
    assert not np.array_equal(outs[nc.FORWARD], outs[nc.COSET_FORWARD])


# ---- the host build where the HI table has more than one entry ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    cp, ci, cu = ctypes.c_char_p, ctypes.c_int, ctypes.c_uint
    lib.ht_ntt_transform.argtypes = [ci, cu, cu, cu, cu, cp, ctypes.c_void_p, cu, cu, ctypes.c_void_p]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


# (kind, flags, custom offset): the four kinds, one bit-reversed output, one bit-reversed input, one in normal form, a custom offset on
# one coset call of each direction and form
HOST_CALLS = (
    (nc.FORWARD, nc.FLAG_NR, False),
    (nc.INVERSE, nc.FLAG_RN, False),
    (nc.COSET_FORWARD, nc.FLAG_NORMAL, True),
    (nc.COSET_INVERSE, 0, True),
)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k,pass_log", ((15, 8), (16, 8), (17, 8), (16, 10), (16, 3)))
def test_host_build_against_the_oracle(oracle, ht, field, k, pass_log):
    """k = 15, 16, 17: 2, 4 and 8 HI entries, so the twiddle between passes (and every offset power past 2^14) is a product of two
    non-trivial table entries, under the limb-bound checker; in_len = n/2 + 1, random 256-bit inputs; every byte against the oracle"""
    n = 1 << k
    in_len = n // 2 + 1
    raw = np.random.default_rng(0xB0 + k).integers(0, 256, size=(n, 32), dtype=np.uint8)
    for kind, flags, custom in HOST_CALLS:
        off = nc.encode(field, [custom_offset(field)], bool(flags & nc.FLAG_NORMAL)) if custom else None
        want = nc.oracle_ntt(oracle, field, k, kind, flags, raw, in_len=in_len, offset=off)
        got = np.empty((n, 32), dtype=np.uint8)
        assert ht.ht_ntt_transform(nc.FIELD_IDS[field], k, pass_log, kind, flags, off, raw.ctypes.data, in_len, 1, got.ctypes.data) == 0
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, "%s k=%d pass_log=%d kind=%d flags=%d: %d elements differ, first %s" % (field, k, pass_log, kind, flags, bad.size, bad[:8].tolist())
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()
