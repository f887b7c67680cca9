"""CPU: the calls between a transform and an MSM (mi355_msm_domain_batch_inverse .. _divide_by_vanishing_on_coset) exist in every layer
with the same shape -- exported by libmi355msm.so, declared in the C header, in the Rust crate's extern block and in the Python
binding -- and judge their arguments before they look for a handle or a device.  (An offset inside the domain needs a domain to be
judged against: without a GPU no handle exists, so that refusal is pinned on the host build's copy of the same function in
tests/test_poly_host.py and on the call itself in tests/test_gpu_poly.py.)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ntt_cases as nc
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
ARITY = {
    "mi355_msm_domain_batch_inverse": 6,
    "mi355_msm_domain_batch_inverse_device": 7,
    "mi355_msm_domain_vec_op": 8,
    "mi355_msm_domain_vec_op_device": 9,
    "mi355_msm_domain_evaluate": 6,
    "mi355_msm_domain_evaluate_device": 7,
    "mi355_msm_domain_divide_by_linear": 7,
    "mi355_msm_domain_divide_by_linear_device": 8,
    "mi355_msm_domain_lagrange": 4,
    "mi355_msm_domain_lagrange_device": 5,
    "mi355_msm_domain_vanishing": 4,
    "mi355_msm_domain_divide_by_vanishing_on_coset": 6,
    "mi355_msm_domain_divide_by_vanishing_on_coset_device": 7,
}
HIP_ERROR_NO_DEVICE = 100
METHODS = ("batch_inversion", "batch_inversion_and_mul", "add", "sub", "mul_sub", "scale", "evaluate", "divide_by_linear",
           "evaluate_all_lagrange_coefficients", "evaluate_vanishing_polynomial", "divide_by_vanishing_poly_on_coset")


def _free(err):
    assert err.message
    msg = ctypes.string_at(err.message)
    ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
    return msg


def test_symbols_exported_and_declared_everywhere(ea):
    lib = ea.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libmi355msm.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355_msm.h")).read(), flags=re.S)
    c_decls = {name: len(params.split(",")) for name, params in re.findall(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", header)}
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    rust_items = {}
    for block in re.findall(r'extern\s+"C"\s*\{(.*?)\n\s*\}', rust, flags=re.S):
        for name, params in re.findall(r"fn\s+(\w+)\s*\((.*?)\)\s*(?:->\s*[\w:]+)?\s*;", block, flags=re.S):
            rust_items[name] = len([p for p in params.strip().rstrip(",").split(",") if p.strip()])
    for name, arity in ARITY.items():
        assert name in exported, name
        assert c_decls.get(name) == arity, (name, c_decls.get(name))
        assert rust_items.get(name) == arity, (name, rust_items.get(name))
        assert len(getattr(lib, name).argtypes) == arity, name
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for f in METHODS:
        assert hasattr(ea.Radix2EvaluationDomain, f), f
        assert f in hpp, f
    full = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    for word in ("poly_work_bytes", "poly_tile_log", "batch_inversion_and_mul", "divide_by_vanishing_poly_on_coset_in_place"):
        assert word in full, word


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: every argument is judged before the handle is, so a null
    handle is enough to reach each refusal"""
    lib = ea.load_library()
    buf = np.zeros(64 * 32, dtype=np.uint8)
    p = buf.ctypes.data
    one = ctypes.create_string_buffer(32)
    o32 = ctypes.create_string_buffer(32)
    big = (1 << 30) + 1
    L = lib
    calls = [
        # null pointers
        (L.mi355_msm_domain_batch_inverse(None, None, p, 4, None, 0), b"null input or output"),
        (L.mi355_msm_domain_batch_inverse_device(None, p, None, 4, None, 0, None), b"null input or output"),
        (L.mi355_msm_domain_vec_op(None, p, p, None, None, 4, 0, 0), b"null input or output"),
        (L.mi355_msm_domain_vec_op(None, p, p, p, None, 4, 2, 0), b"null input or output"),
        (L.mi355_msm_domain_vec_op_device(None, p, p, None, None, 4, 3, 0, None), b"null factor"),
        (L.mi355_msm_domain_evaluate(None, None, p, 4, one, 0), b"null input or output"),
        (L.mi355_msm_domain_evaluate_device(None, o32, p, 4, None, 0, None), b"null input or output"),
        (L.mi355_msm_domain_divide_by_linear(None, None, o32, p, 4, one, 0), b"null input or output"),
        (L.mi355_msm_domain_divide_by_linear_device(None, p + 1024, o32, None, 4, one, 0, None), b"null input or output"),
        (L.mi355_msm_domain_lagrange(None, None, one, 0), b"null input or output"),
        (L.mi355_msm_domain_lagrange_device(None, p, None, 0, None), b"null input or output"),
        (L.mi355_msm_domain_vanishing(None, o32, None, 0), b"null input or output"),
        (L.mi355_msm_domain_divide_by_vanishing_on_coset(None, None, p, 4, None, 0), b"null input or output"),
        # a partial overlap (out == in is allowed where the call says so; the division takes no overlap at all)
        (L.mi355_msm_domain_batch_inverse(None, p + 32, p, 8, None, 0), b"overlap"),
        (L.mi355_msm_domain_batch_inverse_device(None, p, p + 7 * 32, 8, None, 0, None), b"overlap"),
        (L.mi355_msm_domain_vec_op(None, p + 32, p + 512, p, None, 8, 0, 0), b"overlaps b"),
        (L.mi355_msm_domain_vec_op(None, p + 32, p, p + 512, None, 8, 1, 0), b"overlaps a"),
        (L.mi355_msm_domain_vec_op_device(None, p + 1024 + 32, p, p + 512, p + 1024, 8, 2, 0, None), b"overlaps c"),
        (L.mi355_msm_domain_divide_by_linear(None, p, o32, p, 8, one, 0), b"overlaps the coefficients"),
        (L.mi355_msm_domain_divide_by_linear_device(None, p + 7 * 32, o32, p, 8, one, 0, None), b"overlaps the coefficients"),
        (L.mi355_msm_domain_divide_by_vanishing_on_coset_device(None, p + 32, p, 8, None, 0, None), b"overlap"),
        # unknown flag bits, an unknown operation
        (L.mi355_msm_domain_batch_inverse(None, p, p, 4, None, 2), b"flag bits 0x2"),
        (L.mi355_msm_domain_vec_op(None, p, p, p, None, 4, 0, 4), b"flag bits 0x4"),
        (L.mi355_msm_domain_vec_op(None, p, p, p, None, 4, 4, 0), b"operation 4"),
        (L.mi355_msm_domain_evaluate(None, o32, p, 4, one, 3), b"flag bits 0x3"),
        (L.mi355_msm_domain_divide_by_linear(None, p + 1024, o32, p, 4, one, 8), b"flag bits 0x8"),
        (L.mi355_msm_domain_lagrange(None, p, one, 2), b"flag bits"),
        (L.mi355_msm_domain_vanishing(None, o32, one, 2), b"flag bits"),
        (L.mi355_msm_domain_divide_by_vanishing_on_coset(None, p, p, 4, None, 0x10), b"flag bits 0x10"),
        # n above 2^30
        (L.mi355_msm_domain_batch_inverse(None, p, p, big, None, 0), b"2^30"),
        (L.mi355_msm_domain_vec_op_device(None, p, p, p, None, big, 0, 0, None), b"2^30"),
        (L.mi355_msm_domain_evaluate(None, o32, p, big, one, 0), b"2^30"),
        (L.mi355_msm_domain_divide_by_linear(None, p, o32, p, big, one, 0), b"2^30"),
        (L.mi355_msm_domain_divide_by_vanishing_on_coset(None, p, p, big, None, 0), b"2^30"),
        # misaligned device pointers
        (L.mi355_msm_domain_batch_inverse_device(None, p + 1, p + 1, 4, None, 0, None), b"aligned"),
        # and, with everything else in order, the handle
        (L.mi355_msm_domain_batch_inverse(None, p, p, 4, None, 0), b"null domain handle"),
        (L.mi355_msm_domain_vec_op(None, p, p, p, p, 4, 2, 1), b"null domain handle"),
        (L.mi355_msm_domain_vec_op(None, p, p, one, None, 4, 3, 1), b"null domain handle"),
        (L.mi355_msm_domain_evaluate(None, o32, p, 4, one, 1), b"null domain handle"),
        (L.mi355_msm_domain_evaluate(None, o32, None, 0, one, 0), b"null domain handle"),
        (L.mi355_msm_domain_divide_by_linear(None, p + 1024, None, p, 4, one, 0), b"null domain handle"),
        (L.mi355_msm_domain_divide_by_linear(None, None, o32, p, 1, one, 0), b"null domain handle"),
        (L.mi355_msm_domain_lagrange(None, p, one, 1), b"null domain handle"),
        (L.mi355_msm_domain_vanishing(None, o32, one, 1), b"null domain handle"),
        (L.mi355_msm_domain_divide_by_vanishing_on_coset(None, p, p, 4, one, 0), b"null domain handle"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
    v = ctypes.c_uint64()
    for err in (lib.mi355_msm_domain_query(None, b"poly_work_bytes", ctypes.byref(v)), lib.mi355_msm_domain_set_option(None, b"poly_tile_log", 4)):
        assert err.code == -1 and _free(err)


def test_without_a_gpu_the_calls_say_so(ea):
    """there is no CPU fallback: without a device no handle can be made, and the wrapper passes the runtime's code on"""
    import torch

    if torch.cuda.is_available():
        with ea.Radix2EvaluationDomain(16, curve="bls12_381_g1") as d:
            assert d.query("poly_tile_log") == 10 and d.query("poly_work_bytes") == 0
            with pytest.raises(ea.MsmError) as e:
                d.set_option("poly_tile_log", 3)
            assert "poly_tile_log" in str(e.value)
            with pytest.raises(ea.MsmError):
                d.set_option("poly_tile_log", 11)
    else:
        with pytest.raises(ea.MsmError) as e:
            ea.Radix2EvaluationDomain(16, curve="bls12_381_g1").batch_inversion(bytes(64))
        assert e.value.code == HIP_ERROR_NO_DEVICE and "no HIP device" in str(e.value)


class _NoDevice:
    """the wrapper's own checks run before any call into the library: a stand-in handle is enough to reach them"""

    def __init__(self, ea):
        self.d = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
        self.d.curve, self.d.modulus, self.d.size, self.d.device = 1, nc.modulus("bls12_381"), 16, 0
        self.d.handle = ctypes.c_void_p(1)       # never dereferenced: every case below is refused in Python
        self.d._lib = None

    def __enter__(self):
        return self.d

    def __exit__(self, *exc):
        self.d.handle = ctypes.c_void_p()


def test_python_wrappers_check_shapes(ea):
    with _NoDevice(ea) as d:
        a, b = np.zeros((4, 32), dtype=np.uint8), np.zeros((5, 32), dtype=np.uint8)
        for call in (lambda: d.add(a, b), lambda: d.sub(b, a), lambda: d.mul_sub(a, a, b), lambda: d.batch_inversion(bytes(33)),
                     lambda: d.evaluate(bytes(31), 5), lambda: d.divide_by_linear(np.zeros(40, dtype=np.uint8), 5),
                     lambda: d.divide_by_vanishing_poly_on_coset(bytes(65)), lambda: d.scale(bytes(1), 3)):
            with pytest.raises(ValueError, match="32-byte elements"):
                call()
        for call in (lambda: d.batch_inversion(a, out=a), lambda: d.add(a, a, out=a), lambda: d.divide_by_linear(a, 3, out=a)):
            with pytest.raises(ValueError, match="out= goes with GPU tensors"):
                call()
        with pytest.raises(ValueError):
            d.evaluate_all_lagrange_coefficients(3, out=np.zeros((16, 32), dtype=np.uint8))
    closed = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
    closed.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        closed.batch_inversion(bytes(32))
    with pytest.raises(ea.MsmError, match="closed"):
        closed.evaluate_all_lagrange_coefficients(1)
