"""CPU: the scans and the permutation product (mi355_msm_domain_scan, mi355_msm_domain_permutation_product and their _device twins)
exist in every layer with the same shape -- exported by libmi355msm.so, declared in the C header, in the Rust crate's extern block and
in the Python binding -- and judge their arguments before they look for a handle or a device.  (A stride below the rows of the domain
and an output that overlaps the columns need a domain to be judged against: without a GPU no handle exists, so here only the stride
that is below every domain, 0, is refused, and the full checks are pinned on the call itself in tests/test_gpu_scan.py.)"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ntt_cases as nc
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
ARITY = {
    "mi355_msm_domain_scan": 7,
    "mi355_msm_domain_scan_device": 8,
    "mi355_msm_domain_permutation_product": 11,
    "mi355_msm_domain_permutation_product_device": 12,
}
METHODS = ("prefix_product", "prefix_sum", "permutation_product")


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
    for word in ("scan_work_bytes", "ZEROS ARE NOT SKIPPED", "A ZERO DENOMINATOR IS NOT AN ERROR"):
        assert word in full, word


def test_python_signatures(ea):
    d = ea.Radix2EvaluationDomain
    for f in ("prefix_product", "prefix_sum"):
        sig = inspect.signature(getattr(d, f))
        assert list(sig.parameters) == ["self", "v", "inclusive", "montgomery", "out"]
        assert (sig.parameters["inclusive"].default, sig.parameters["montgomery"].default, sig.parameters["out"].default) == (False, True, None)
    sig = inspect.signature(d.permutation_product)
    assert list(sig.parameters) == ["self", "wires", "sigmas", "beta", "gamma", "ks", "montgomery", "out"]
    assert sig.parameters["montgomery"].default is True and sig.parameters["out"].default is None


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: every argument is judged before the handle is, so a null
    handle is enough to reach each refusal; the order is that of the calls of tests/test_poly_api.py (flags, length, operation and
    column count, null pointers, overlap, alignment, handle)"""
    lib = ea.load_library()
    buf = np.zeros(64 * 32, dtype=np.uint8)
    p = buf.ctypes.data
    one = ctypes.create_string_buffer(32)
    ks = ctypes.create_string_buffer(8 * 32)
    t32 = ctypes.create_string_buffer(32)
    big = (1 << 30) + 1
    L = lib
    scan, scan_d = L.mi355_msm_domain_scan, L.mi355_msm_domain_scan_device
    perm, perm_d = L.mi355_msm_domain_permutation_product, L.mi355_msm_domain_permutation_product_device
    calls = [
        # an unknown operation
        (scan(None, p, t32, p, 4, 2, 0), b"operation 2"),
        (scan_d(None, p, None, p, 4, 7, 1, None), b"operation 7"),
        # unknown flag bits (the permutation product has no inclusive form)
        (scan(None, p, t32, p, 4, 0, 4), b"flag bits 0x4"),
        (scan_d(None, p, t32, p, 4, 1, 0x13, None), b"flag bits 0x13"),
        (perm(None, p, t32, p + 512, p + 1024, 3, 4, ks, one, one, 2), b"flag bits 0x2"),
        (perm_d(None, p, t32, p + 512, p + 1024, 3, 4, ks, one, one, 8, None), b"flag bits 0x8"),
        # a partial overlap (out == in is allowed)
        (scan(None, p + 32, t32, p, 8, 0, 0), b"overlap"),
        (scan_d(None, p, None, p + 7 * 32, 8, 1, 2, None), b"overlap"),
        # n above 2^30
        (scan(None, p, t32, p, big, 0, 0), b"2^30"),
        (scan_d(None, p, t32, p, big, 1, 3, None), b"2^30"),
        # the column count
        (perm(None, p, t32, p + 512, p + 1024, 0, 4, ks, one, one, 0), b"0 columns"),
        (perm_d(None, p, t32, p + 512, p + 1024, 9, 4, ks, one, one, 1, None), b"9 columns"),
        # a stride below the rows of every domain
        (perm(None, p, t32, p + 512, p + 1024, 3, 0, ks, one, one, 0), b"stride of 0"),
        # null pointers
        (scan(None, None, t32, p, 4, 0, 0), b"null input or output"),
        (scan_d(None, p, t32, None, 4, 1, 2, None), b"null input or output"),
        (perm(None, None, t32, p + 512, p + 1024, 3, 4, ks, one, one, 0), b"null input or output"),
        (perm(None, p, t32, None, p + 1024, 3, 4, ks, one, one, 0), b"null input or output"),
        (perm(None, p, t32, p + 512, None, 3, 4, ks, one, one, 0), b"null input or output"),
        (perm(None, p, t32, p + 512, p + 1024, 3, 4, None, one, one, 0), b"null input or output"),
        (perm(None, p, t32, p + 512, p + 1024, 3, 4, ks, None, one, 0), b"null input or output"),
        (perm_d(None, p, t32, p + 512, p + 1024, 3, 4, ks, one, None, 0, None), b"null input or output"),
        # the order: the operation before the pointers, the flags before the operation, the columns before the pointers
        (scan(None, None, None, None, 4, 2, 0), b"operation 2"),
        (scan(None, None, None, None, big, 2, 4), b"flag bits 0x4"),
        (scan(None, None, None, None, big, 2, 0), b"2^30"),
        (perm(None, None, None, None, None, 9, 0, None, None, None, 2), b"flag bits 0x2"),
        (perm(None, None, None, None, None, 9, 0, None, None, None, 0), b"9 columns"),
        (perm(None, None, None, None, None, 8, 0, None, None, None, 0), b"stride of 0"),
        # misaligned device pointers
        (scan_d(None, p + 1, t32, p + 1, 4, 0, 0, None), b"aligned"),
        (perm_d(None, p + 2, t32, p + 512, p + 1024, 3, 4, ks, one, one, 0, None), b"aligned"),
        # and, with everything else in order, the handle (total32 may be NULL; n = 0 needs no vectors)
        (scan(None, p, t32, p, 4, 0, 0), b"null domain handle"),
        (scan(None, p + 1024, None, p, 4, 1, 3), b"null domain handle"),
        (scan(None, None, t32, None, 0, 0, 0), b"null domain handle"),
        (scan_d(None, p, None, p, 4, 1, 2, None), b"null domain handle"),
        (perm(None, p, t32, p + 512, p + 1024, 1, 4, ks, one, one, 0), b"null domain handle"),
        (perm(None, p, None, p + 512, p + 1024, 8, 4, ks, one, one, 1), b"null domain handle"),
        (perm_d(None, p, t32, p + 512, p + 1024, 3, 4, ks, one, one, 0, None), b"null domain handle"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
    v = ctypes.c_uint64()
    err = lib.mi355_msm_domain_query(None, b"scan_work_bytes", ctypes.byref(v))
    assert err.code == -1 and _free(err)


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
        a = np.zeros((4, 32), dtype=np.uint8)
        cols = np.zeros((3, 16, 32), dtype=np.uint8)
        for call in (lambda: d.prefix_product(bytes(33)), lambda: d.prefix_sum(np.zeros(40, dtype=np.uint8))):
            with pytest.raises(ValueError, match="32-byte elements"):
                call()
        for call in (lambda: d.prefix_product(a, out=a), lambda: d.prefix_sum(a, inclusive=True, out=a),
                     lambda: d.permutation_product(cols, cols, 2, 3, [1, 2, 3], out=a)):
            with pytest.raises(ValueError, match="out= goes with GPU tensors"):
                call()
        for call in (lambda: d.permutation_product(cols[:, :8], cols, 2, 3, [1, 2, 3]),                 # rows that are not the domain's
                     lambda: d.permutation_product(np.zeros((9, 16, 32), np.uint8), np.zeros((9, 16, 32), np.uint8), 2, 3, list(range(9))),
                     lambda: d.permutation_product([], [], 2, 3, []),
                     lambda: d.permutation_product(cols, cols[:2], 2, 3, [1, 2, 3]),                    # fewer sigmas than wires
                     lambda: d.permutation_product(cols, cols, 2, 3, [1, 2]),                           # fewer ks than columns
                     lambda: d.permutation_product([bytes(16 * 32)] * 2, [bytes(16 * 32)] * 2, 2, 3, [1])):
            with pytest.raises(ValueError, match="columns"):
                call()
    closed = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
    closed.handle = ctypes.c_void_p()
    for call in (lambda: closed.prefix_product(bytes(32)), lambda: closed.prefix_sum(bytes(32)),
                 lambda: closed.permutation_product(np.zeros((1, 16, 32), np.uint8), np.zeros((1, 16, 32), np.uint8), 1, 1, [1])):
        with pytest.raises(ea.MsmError, match="closed"):
            call()
