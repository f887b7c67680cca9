"""CPU: the per-point classification of csrc/check_points.hpp, compiled for the host with the limb-bound checker armed
(libmsm_hosttest.so, ht_check_points), against the Python model on the whole corpus of tests/check_cases.py."""
import ctypes
import os

import pytest

import check_cases as cc
import pymodel as pm
from conftest import ROOT


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    lib.ht_check_points.argtypes = [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p]
    lib.ht_check_failures.restype = ctypes.c_long
    return lib


def classify(lib, curve, cases, serialized, method):
    buf = cc.encode_all(curve, cases, serialized)
    out = ctypes.create_string_buffer(max(len(cases), 1))
    stride = 2 * curve.coord_bytes if serialized else curve.affine_stride
    assert lib.ht_check_points(curve.curve_id, int(serialized), method, buf, stride, len(cases), out) == 0
    return list(out.raw[:len(cases)])


@pytest.mark.parametrize("method", [0, 1], ids=["exact", "endomorphism"])
@pytest.mark.parametrize("serialized", [False, True], ids=["in_memory", "serialized"])
@pytest.mark.parametrize("name", cc.CURVE_NAMES)
def test_host_build_classifies_the_corpus(ht, name, serialized, method):
    curve = pm.CURVES[name]
    cases, statuses, labels = cc.corpus(name)
    before = ht.ht_check_failures()
    got = classify(ht, curve, cases, serialized, method)
    wrong = [(i, labels[i], statuses[i], got[i]) for i in range(len(cases)) if got[i] != statuses[i]]
    assert not wrong, wrong[:8]
    assert ht.ht_check_failures() == before == 0      # every limb bound held through chains of bits(r) - 1 = 252 / 254 doublings


def test_corpus_holds_what_it_should():
    for name in cc.CURVE_NAMES:
        cases, statuses, labels = cc.corpus(name)
        assert statuses.count(0) >= 40 and statuses.count(3) >= 40
        assert statuses.count(1) >= 3 and statuses.count(2) >= 10
        assert statuses[labels.index("x + p and off the curve")] == 1           # the lowest status wins
        assert statuses[labels.index("(0, 0) without the flag")] == 2
        assert statuses[labels.index("inf junk non-canonical")] == 0            # the flag is authoritative
    labels = cc.corpus("bls12_377_g1")[2]
    assert "T of order 2" in labels and "T of order 3" in labels


@pytest.mark.parametrize("n", [0, 1, 255, 257, 1000])
def test_placement(ht, n):
    name = "bls12_377_g1"
    curve = pm.CURVES[name]
    cases, statuses = cc.placed(name, n)
    assert classify(ht, curve, cases, False, 1) == statuses
    if n:
        assert statuses[0] != 0 and statuses[n - 1] != 0


def test_bad_arguments(ht):
    out = ctypes.create_string_buffer(4)
    assert ht.ht_check_points(7, 0, 0, b"\0" * 104, 104, 1, out) == -1
    assert ht.ht_check_points(0, 0, 2, b"\0" * 104, 104, 1, out) == -1
    assert ht.ht_check_points(0, 0, 0, b"\0" * 104, 96, 1, out) == -1          # stride does not reach the flag byte
