"""CPU: the rows of the Plonk quotient and the linear combination (mi355_msm_domain_plonk_quotient, mi355_msm_domain_linear_combination
and their _device twins) exist in every layer with the same shape -- exported by libmi355msm.so, declared in the C header, in the Rust
crate's extern block and in the Python binding -- and judge their arguments before they look for a handle or a device.  (The ratio
M / n, a stride below the rows of the domain, the overlap of whole columns and an offset inside the domain need a domain to be judged
against: without a GPU no handle exists, so here only what holds for every domain is refused -- an n that is no power of two or leaves
no domain a ratio, a stride of 0, an output that IS an input, an offset of 32 zero bytes -- and the full checks are pinned on the call
itself in tests/test_gpu_quotient.py.)"""
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
    "mi355_msm_domain_plonk_quotient": 16,
    "mi355_msm_domain_plonk_quotient_device": 17,
    "mi355_msm_domain_linear_combination": 7,
    "mi355_msm_domain_linear_combination_device": 8,
}
METHODS = ("plonk_quotient", "linear_combination")


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
    for word in ("quotient_work_bytes", "x - 1 IS NEVER 0", "There is no CPU fallback"):
        assert word in full, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "x - 1 is never 0" in design


def test_python_signatures(ea):
    d = ea.Radix2EvaluationDomain
    sig = inspect.signature(d.plonk_quotient)
    assert list(sig.parameters) == ["self", "wires", "sigmas", "z", "alpha", "beta", "gamma", "ks", "n", "selectors", "pi", "offset", "montgomery", "out"]
    assert [sig.parameters[k].default for k in ("selectors", "pi", "offset", "montgomery", "out")] == [None, None, None, True, None]
    sig = inspect.signature(d.linear_combination)
    assert list(sig.parameters) == ["self", "cols", "coeffs", "montgomery", "out"]
    assert sig.parameters["montgomery"].default is True and sig.parameters["out"].default is None


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: every argument is judged before the handle is, so a null handle
    is enough to reach each refusal; the order is flags, column count, n, stride, null pointers, alignment, an output that is an input,
    a zero offset, handle"""
    lib = ea.load_library()
    buf = np.zeros(64 * 32, dtype=np.uint8)
    p = buf.ctypes.data
    w, s, q, z, pi = p + 4096, p + 8192, p + 12288, p + 16384, p + 20480     # never read: every call below is refused first
    one = ctypes.create_string_buffer(b"\x01" + bytes(31), 32)
    zero = ctypes.create_string_buffer(32)
    ks = ctypes.create_string_buffer(8 * 32)
    L = lib
    quot, quot_d = L.mi355_msm_domain_plonk_quotient, L.mi355_msm_domain_plonk_quotient_device
    lin, lin_d = L.mi355_msm_domain_linear_combination, L.mi355_msm_domain_linear_combination_device
    cols2 = (ctypes.c_void_p * 2)(p, p + 1024)
    part = (ctypes.c_void_p * 2)(p + 32, p + 1024)
    nullcol = (ctypes.c_void_p * 2)(p, None)
    odd = (ctypes.c_void_p * 2)(p, p + 1025)
    lens2 = (ctypes.c_size_t * 2)(8, 4)
    huge = (ctypes.c_size_t * 2)(8, (1 << 30) + 1)
    many = (ctypes.c_void_p * 33)(*([p] * 33))
    lens33 = (ctypes.c_size_t * 33)(*([1] * 33))
    calls = [
        # unknown flag bits
        (quot(None, p, w, s, q, z, pi, 5, 64, 8, ks, one, one, one, None, 2), b"flag bits 0x2"),
        (quot_d(None, p, w, s, None, z, None, 3, 64, 8, ks, one, one, one, None, 0x11, None), b"flag bits 0x11"),
        (lin(None, p, cols2, lens2, ks, 2, 4), b"flag bits 0x4"),
        (lin_d(None, p, cols2, lens2, ks, 2, 3, None), b"flag bits 0x3"),
        # the column count: 5 beside selectors, 1 .. 8 without, 1 .. 32 columns of a combination
        (quot(None, p, w, s, q, z, pi, 4, 64, 8, ks, one, one, one, None, 0), b"4 columns"),
        (quot_d(None, p, w, s, q, z, pi, 8, 64, 8, ks, one, one, one, None, 1, None), b"8 columns"),
        (quot(None, p, w, s, None, z, pi, 0, 64, 8, ks, one, one, one, None, 0), b"0 columns"),
        (quot(None, p, w, s, None, z, pi, 9, 64, 8, ks, one, one, one, None, 0), b"9 columns"),
        (lin(None, p, cols2, lens2, ks, 0, 0), b"0 columns"),
        (lin_d(None, p, many, lens33, ks, 33, 0, None), b"33 columns"),
        # n: a power of two, and small enough to leave some domain a ratio of 2
        (quot(None, p, w, s, q, z, pi, 5, 64, 0, ks, one, one, one, None, 0), b"not a power of two"),
        (quot(None, p, w, s, q, z, pi, 5, 64, 12, ks, one, one, one, None, 0), b"not a power of two"),
        (quot_d(None, p, w, s, None, z, pi, 2, 64, 1 << 28, ks, one, one, one, None, 0, None), b"ratio"),
        # the stride
        (quot(None, p, w, s, q, z, pi, 5, 0, 8, ks, one, one, one, None, 0), b"stride of 0"),
        (quot(None, p, w, s, q, z, pi, 5, (1 << 30) + 1, 8, ks, one, one, one, None, 0), b"2^30"),
        # a column above 2^30
        (lin(None, p, cols2, huge, ks, 2, 0), b"2^30"),
        # null pointers (selectors, pi and offset may be NULL)
        (quot(None, None, w, s, q, z, pi, 5, 64, 8, ks, one, one, one, None, 0), b"null input or output"),
        (quot(None, p, None, s, q, z, pi, 5, 64, 8, ks, one, one, one, None, 0), b"null input or output"),
        (quot(None, p, w, None, q, z, pi, 5, 64, 8, ks, one, one, one, None, 0), b"null input or output"),
        (quot(None, p, w, s, q, None, pi, 5, 64, 8, ks, one, one, one, None, 0), b"null input or output"),
        (quot(None, p, w, s, q, z, pi, 5, 64, 8, None, one, one, one, None, 0), b"null input or output"),
        (quot(None, p, w, s, q, z, pi, 5, 64, 8, ks, None, one, one, None, 0), b"null input or output"),
        (quot(None, p, w, s, q, z, pi, 5, 64, 8, ks, one, None, one, None, 0), b"null input or output"),
        (quot_d(None, p, w, s, q, z, pi, 5, 64, 8, ks, one, one, None, None, 0, None), b"null input or output"),
        (lin(None, p, None, lens2, ks, 2, 0), b"null input or output"),
        (lin(None, p, cols2, None, ks, 2, 0), b"null input or output"),
        (lin(None, p, cols2, lens2, None, 2, 0), b"null input or output"),
        (lin(None, None, cols2, lens2, ks, 2, 0), b"null input or output"),
        (lin_d(None, p, nullcol, lens2, ks, 2, 0, None), b"null input or output"),
        # misaligned device pointers
        (quot_d(None, p + 2, w, s, q, z, pi, 5, 64, 8, ks, one, one, one, None, 0, None), b"aligned"),
        (quot_d(None, p, w, s, q, z + 1, pi, 5, 64, 8, ks, one, one, one, None, 0, None), b"aligned"),
        (lin_d(None, p, odd, lens2, ks, 2, 0, None), b"aligned"),
        # overlap: the rows are never computed in place; a combination may write exactly one of its columns
        (quot(None, p, w, s, q, p, pi, 5, 64, 8, ks, one, one, one, None, 0), b"overlaps"),
        (quot(None, p, p, s, None, z, None, 1, 64, 8, ks, one, one, one, None, 0), b"overlaps"),
        (quot_d(None, p, w, s, q, z, p, 5, 64, 8, ks, one, one, one, None, 0, None), b"overlaps"),
        (lin(None, p, part, lens2, ks, 2, 0), b"overlaps column 0"),
        (lin_d(None, p + 1024 + 64, cols2, lens2, ks, 2, 0, None), b"overlaps column 1"),
        # an offset of zero
        (quot(None, p, w, s, q, z, pi, 5, 64, 8, ks, one, one, one, zero, 0), b"offset is zero"),
        (quot_d(None, p, w, s, None, z, None, 8, 64, 8, ks, one, one, one, zero, 1, None), b"offset is zero"),
        # the order: flags before the columns, the columns before n, n before the stride, the stride before the pointers
        (quot(None, None, None, None, q, None, None, 4, 0, 12, None, None, None, None, zero, 2), b"flag bits 0x2"),
        (quot(None, None, None, None, q, None, None, 4, 0, 12, None, None, None, None, zero, 0), b"4 columns"),
        (quot(None, None, None, None, q, None, None, 5, 0, 12, None, None, None, None, zero, 0), b"not a power of two"),
        (quot(None, None, None, None, q, None, None, 5, 0, 8, None, None, None, None, zero, 0), b"stride of 0"),
        (quot(None, None, None, None, q, None, None, 5, 64, 8, None, None, None, None, zero, 0), b"null input or output"),
        (lin(None, None, None, None, None, 33, 4), b"flag bits 0x4"),
        (lin(None, None, None, None, None, 33, 0), b"33 columns"),
        # and, with everything else in order, the handle (out == a column is allowed; all lengths 0 need no vectors)
        (quot(None, p, w, s, q, z, pi, 5, 64, 8, ks, one, one, one, None, 0), b"null domain handle"),
        (quot(None, p, w, s, None, z, None, 8, 64, 8, ks, one, one, one, one, 1), b"null domain handle"),
        (quot_d(None, p, w, s, q, z, None, 5, 64, 8, ks, one, one, one, None, 0, None), b"null domain handle"),
        (lin(None, p, cols2, lens2, ks, 2, 0), b"null domain handle"),
        (lin(None, None, nullcol, (ctypes.c_size_t * 2)(0, 0), ks, 2, 1), b"null domain handle"),
        (lin_d(None, p + 2048, cols2, lens2, ks, 2, 0, None), b"null domain handle"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
    v = ctypes.c_uint64()
    err = lib.mi355_msm_domain_query(None, b"quotient_work_bytes", ctypes.byref(v))
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
        v = np.zeros((16, 32), dtype=np.uint8)
        cols = np.zeros((5, 16, 32), dtype=np.uint8)
        wide = np.zeros((5, 20, 32), dtype=np.uint8)
        sel = np.zeros((13, 16, 32), dtype=np.uint8)
        ks = [1, 2, 3, 4, 5]
        for call in (lambda: d.plonk_quotient(cols[:, :8], cols, v, 1, 2, 3, ks, 4),                     # fewer rows than the domain has
                     lambda: d.plonk_quotient(np.zeros((9, 16, 32), np.uint8), np.zeros((9, 16, 32), np.uint8), v, 1, 2, 3, list(range(9)), 4),
                     lambda: d.plonk_quotient(cols, cols[:4], v, 1, 2, 3, ks, 4),                        # fewer sigmas than wires
                     lambda: d.plonk_quotient(cols, cols, v, 1, 2, 3, ks[:4], 4),                        # fewer ks than columns
                     lambda: d.plonk_quotient(wide, cols, v, 1, 2, 3, ks, 4),                            # two strides
                     lambda: d.plonk_quotient(cols, cols, v, 1, 2, 3, ks, 4, selectors=sel[:12]),        # 12 selectors
                     lambda: d.plonk_quotient(cols[:3], cols[:3], v, 1, 2, 3, ks[:3], 4, selectors=sel),  # selectors beside 3 wires
                     lambda: d.linear_combination([], []),
                     lambda: d.linear_combination([v] * 33, [1] * 33),
                     lambda: d.linear_combination([v, v], [1])):
            with pytest.raises(ValueError, match="columns"):
                call()
        for call in (lambda: d.plonk_quotient(cols, cols, v[:8], 1, 2, 3, ks, 4), lambda: d.plonk_quotient(cols, cols, v, 1, 2, 3, ks, 4, pi=v[:8]),
                     lambda: d.linear_combination([bytes(33)], [1])):
            with pytest.raises(ValueError, match="32-byte elements"):
                call()
        for call in (lambda: d.plonk_quotient(cols, cols, v, 1, 2, 3, ks, 4, out=v), lambda: d.linear_combination([v, v[:3]], [1, 2], out=v)):
            with pytest.raises(ValueError, match="out= goes with GPU tensors"):
                call()
    closed = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
    closed.handle = ctypes.c_void_p()
    one = np.zeros((1, 16, 32), np.uint8)
    for call in (lambda: closed.plonk_quotient(one, one, bytes(16 * 32), 1, 1, 1, [1], 4), lambda: closed.linear_combination([bytes(32)], [1])):
        with pytest.raises(ea.MsmError, match="closed"):
            call()
