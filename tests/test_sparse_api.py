"""CPU: resident sparse matrices over Fr (mi355_msm_sparse_create, _apply, _query, _destroy) exist in every layer with the same shape --
exported by libmi355msm.so, declared in the C header, in the Rust crate's extern block and in the Python binding -- and judge their
arguments before they look for a handle or a device: without a GPU no domain and so no matrix exists, and every refusal is still
reached with a null handle, in the stated order (unknown flag bits, sizes above their limits, null pointers, alignment, a stream
without flag bit 1, overlap, the structure of the matrix, and last the handle).  The extent of an overlap needs a matrix to be judged
against and is pinned on the handle in tests/test_gpu_sparse.py."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ntt_cases as nc
import stream_cases as st
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
ARITY = {
    "mi355_msm_sparse_create": 8,
    "mi355_msm_sparse_apply": 5,
    "mi355_msm_sparse_query": 3,
    "mi355_msm_sparse_destroy": 1,
}


def _free(err):
    assert err.message
    msg = ctypes.string_at(err.message)
    ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
    return msg


def test_symbols_exported_and_declared_everywhere(ea):
    lib = ea.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libmi355msm.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    full = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
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
    assert "pub struct SparseMatrix" in rust
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for word in ("struct SparseMatrix", "groth16_witness_map", "mi355_msm_sparse_apply"):
        assert word in hpp, word
    for word in ("entries_per_lane", "block_lanes", "work_bytes", "MUST OUTLIVE THE MATRIX", "There is no CPU fallback"):
        assert word in full, word
    assert hasattr(ea, "SparseMatrix") and hasattr(ea.SparseMatrix, "from_rows") and hasattr(ea.SparseMatrix, "apply")
    for f in ("sparse_matrix", "groth16_witness_map"):
        assert hasattr(ea.Radix2EvaluationDomain, f), f


def test_no_new_device_twin_in_the_header():
    """one apply with a flag bit: the names that end in _device( are exactly those of stream_cases.COVERED, which this change leaves alone"""
    text = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    names = set(re.findall(r"\b(mi355_msm_\w+_device)\s*\(", text))
    assert names == {n for n in st.COVERED if n.endswith("_device")}
    assert not [n for n in names if "sparse" in n]
    assert "tests/test_stream_coverage.py" in text and "tests/test_gpu_sparse.py" in text     # the header says why


def test_python_signatures(ea):
    d = ea.Radix2EvaluationDomain
    sig = inspect.signature(d.sparse_matrix)
    assert list(sig.parameters) == ["self", "rows", "cols", "row_ptr", "col_idx", "values", "montgomery"]
    assert sig.parameters["montgomery"].default is True
    sig = inspect.signature(d.groth16_witness_map)
    assert list(sig.parameters) == ["self", "A", "B", "z", "num_inputs", "montgomery"]
    assert sig.parameters["montgomery"].default is True
    sig = inspect.signature(ea.SparseMatrix.apply)
    assert list(sig.parameters) == ["self", "z", "montgomery", "out"]
    assert sig.parameters["montgomery"].default is True and sig.parameters["out"].default is None
    sig = inspect.signature(ea.SparseMatrix.from_rows)
    assert list(sig.parameters) == ["dom", "rows_list", "cols"]
    for f in ("close", "__enter__", "__exit__"):
        assert hasattr(ea.SparseMatrix, f)


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: a null handle is enough to reach each refusal"""
    lib = ea.load_library()
    create, apply_ = lib.mi355_msm_sparse_create, lib.mi355_msm_sparse_apply
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    buf = np.zeros(64 * 32, dtype=np.uint8)
    p = buf.ctypes.data
    vals = p + 1024
    good = np.array([0, 2, 2, 3], dtype=np.uint64)                # 3 rows, 3 entries
    cols3 = np.array([0, 4, 1], dtype=np.uint32)
    first = np.array([1, 2, 2, 3], dtype=np.uint64)               # row_ptr[0] != 0
    down = np.array([0, 2, 1, 3], dtype=np.uint64)                # decreasing at row 1
    wide = np.array([0, 5, 1], dtype=np.uint32)                   # a column >= cols in row 0 ...
    wide2 = np.array([0, 4, 7], dtype=np.uint32)                  # ... and in row 2
    huge = np.array([0, (1 << 31) + 1], dtype=np.uint64)          # nnz above 2^31
    zeros = np.zeros(4, dtype=np.uint64)
    rp, ci = good.ctypes.data, cols3.ctypes.data
    fake = ctypes.c_void_p(64)                                    # a stream that is never used: the call is refused first
    calls = [
        # unknown flag bits
        (create(out, None, 3, 5, rp, ci, vals, 2), b"flag bits 0x2"),
        (create(out, None, 3, 5, rp, ci, vals, 0x10), b"flag bits 0x10"),
        (apply_(None, p, p + 1024, 4, None), b"flag bits 0x4"),
        (apply_(None, p, p + 1024, 0x13, None), b"flag bits 0x13"),
        # sizes above their limits
        (create(out, None, (1 << 30) + 1, 5, rp, ci, vals, 0), b"rows exceed 2^30"),
        (create(out, None, 3, (1 << 30) + 1, rp, ci, vals, 1), b"columns exceed 2^30"),
        (create(out, None, 1, 5, huge.ctypes.data, ci, vals, 0), b"exceed 2^31"),
        # null pointers
        (create(None, None, 3, 5, rp, ci, vals, 0), b"null"),
        (create(out, None, 3, 5, None, ci, vals, 0), b"null"),
        (create(out, None, 3, 5, rp, None, vals, 0), b"null col_idx or values"),
        (create(out, None, 3, 5, rp, ci, None, 0), b"null col_idx or values"),
        (apply_(None, None, p, 0, None), b"null input or output"),
        (apply_(None, p, None, 2, None), b"null input or output"),
        # alignment
        (create(out, None, 3, 5, rp + 4, ci, vals, 0), b"aligned"),
        (create(out, None, 3, 5, rp, ci + 2, vals, 0), b"aligned"),
        (apply_(None, p + 2, p + 1024, 2, None), b"aligned"),
        (apply_(None, p, p + 1025, 3, None), b"aligned"),
        # a stream without flag bit 1
        (apply_(None, p, p + 1024, 0, fake), b"stream goes with device pointers"),
        (apply_(None, p, p + 1024, 1, fake), b"stream goes with device pointers"),
        # overlap: without a matrix only out == z can be judged
        (apply_(None, p, p, 0, None), b"overlaps z"),
        (apply_(None, p, p, 2, fake), b"overlaps z"),
        # the structure, naming the first offending row
        (create(out, None, 3, 5, first.ctypes.data, ci, vals, 0), b"row 0: row_ptr[0] is 1"),
        (create(out, None, 3, 5, down.ctypes.data, ci, vals, 0), b"row 1: row_ptr decreases"),
        (create(out, None, 3, 5, rp, wide.ctypes.data, vals, 0), b"row 0: column index 5"),
        (create(out, None, 3, 5, rp, wide2.ctypes.data, vals, 1), b"row 2: column index 7"),
        (create(out, None, 3, 4, rp, ci, vals, 0), b"row 0: column index 4"),
        # the order: flags before sizes, sizes before pointers, pointers before alignment, alignment before the stream, the stream
        # before the overlap, the structure before the handle
        (create(None, None, (1 << 30) + 1, 5, None, None, None, 2), b"flag bits 0x2"),
        (create(None, None, (1 << 30) + 1, 5, None, None, None, 0), b"rows exceed 2^30"),
        (create(None, None, 3, 5, rp + 4, None, None, 0), b"null"),
        (create(out, None, 3, 5, first.ctypes.data + 4, ci, vals, 0), b"aligned"),
        (apply_(None, None, None, 4, fake), b"flag bits 0x4"),
        (apply_(None, None, p + 1, 2, fake), b"null input or output"),
        (apply_(None, p + 1, p + 1, 2, None), b"aligned"),
        (apply_(None, p, p, 0, fake), b"stream goes with device pointers"),
        # and, with everything else in order, the handle (an empty matrix needs neither indices nor values)
        (create(out, None, 3, 5, rp, ci, vals, 0), b"null domain handle"),
        (create(out, None, 3, 5, rp, ci, vals, 1), b"null domain handle"),
        (create(out, None, 3, 0, zeros.ctypes.data, None, None, 0), b"null domain handle"),
        (create(out, None, 0, 0, zeros.ctypes.data, None, None, 0), b"null domain handle"),
        (apply_(None, p, p + 1024, 0, None), b"null matrix handle"),
        (apply_(None, p, p + 1024, 3, fake), b"null matrix handle"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
        assert not h.value, i
    v = ctypes.c_uint64()
    for key in (b"rows", b"cols", b"nnz", b"work_bytes"):
        err = lib.mi355_msm_sparse_query(None, key, ctypes.byref(v))
        assert err.code == -1 and b"null matrix handle" in _free(err)
    # the constants of the kernels are answered without a matrix; a lane boundary lies at every multiple of the first
    for key in (b"entries_per_lane", b"block_lanes"):
        assert lib.mi355_msm_sparse_query(None, key, ctypes.byref(v)).code == 0 and v.value >= 2
    assert lib.mi355_msm_sparse_destroy(None).code == 0


class _NoDevice:
    """the wrapper's own checks run before any call into the library: a stand-in handle is enough to reach them"""

    def __init__(self, ea, rows=6, cols=5):
        self.d = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
        self.d.curve, self.d.modulus, self.d.size, self.d.device = 1, nc.modulus("bls12_381"), 16, 0
        self.d.handle = ctypes.c_void_p(1)       # never dereferenced: every case below is refused in Python
        self.d._lib = None
        self.m = ea.SparseMatrix.__new__(ea.SparseMatrix)
        self.m.dom, self.m._lib, self.m.handle = self.d, None, ctypes.c_void_p(1)
        self.m.rows, self.m.cols, self.m.nnz = rows, cols, 0

    def __enter__(self):
        return self.d, self.m

    def __exit__(self, *exc):
        self.d.handle = ctypes.c_void_p()
        self.m.handle = ctypes.c_void_p()


def test_python_wrappers_check_shapes(ea):
    with _NoDevice(ea) as (d, m):
        for z in (np.zeros((4, 32), np.uint8), np.zeros((5, 31), np.uint8), np.zeros(5 * 32, np.uint8), bytes(5 * 32 + 1), bytes(4 * 32)):
            with pytest.raises(ValueError, match=r"z: 5 32-byte elements"):
                m.apply(z)
        with pytest.raises(ValueError, match="out= goes with GPU tensors"):
            m.apply(np.zeros((5, 32), np.uint8), out=np.zeros((6, 32), np.uint8))
        zero = np.zeros(0, dtype=np.uint32)
        for call in (lambda: d.sparse_matrix(3, 5, np.zeros(3, np.uint64), zero, b""),               # rows + 1 offsets
                     lambda: d.sparse_matrix(3, 5, bytes(8 * 4 + 1), zero, b"")):
            with pytest.raises(ValueError, match="row_ptr"):
                call()
        with pytest.raises(ValueError, match="values"):
            d.sparse_matrix(1, 5, np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), bytes(32))
        with pytest.raises(ValueError, match="negative"):
            d.sparse_matrix(-1, 5, np.zeros(1, np.uint64), zero, b"")
        # the witness map: two matrices of one shape, and constraints plus inputs within the domain
        other = _NoDevice(ea, rows=7).m
        with pytest.raises(ValueError, match="agree in shape"):
            d.groth16_witness_map(m, other, bytes(5 * 32), 1)
        big = _NoDevice(ea, rows=15).m
        with pytest.raises(ValueError, match="do not fit a domain of 16"):
            d.groth16_witness_map(big, big, bytes(5 * 32), 2)
        for o in (other, big):
            o.handle = ctypes.c_void_p()
    closed = ea.SparseMatrix.__new__(ea.SparseMatrix)
    closed.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        closed.apply(bytes(32))
    dom = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
    dom.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        dom.sparse_matrix(0, 0, np.zeros(1, np.uint64), np.zeros(0, np.uint32), b"")
    with pytest.raises(ea.MsmError, match="closed"):
        dom.groth16_witness_map(closed, closed, b"", 0)
