"""CPU: the multilinear-extension and sumcheck calls of the domain handle (mi355_msm_domain_mle_fix, _mle_eq, _sumcheck_round) exist in
every layer with the same shape -- exported by libmi355msm.so, declared in the C header, in the Rust crate's extern block and in the
Python binding -- and judge their arguments before they look for a handle or a device: every refusal is reached with a null handle, in
the stated order (unknown flag bits, sizes outside their limits, null pointers, alignment, a stream without flag bit 1, overlap, the
term list, and last the handle), every limit at its edge and one past it."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

import stream_cases as st
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
ARITY = {"mi355_msm_domain_mle_fix": 8, "mi355_msm_domain_mle_eq": 6, "mi355_msm_domain_sumcheck_round": 11}
HANDLE = b"null domain handle"


class Term(ctypes.Structure):
    _fields_ = [("coeff", ctypes.c_uint8 * 32), ("n_factors", ctypes.c_uint32), ("factors", ctypes.c_uint32 * 5)]


def terms_of(lists):
    arr = (Term * max(len(lists), 1))()
    for j, fs in enumerate(lists):
        arr[j].coeff[0] = 1
        arr[j].n_factors = len(fs)
        for q, f in enumerate(fs[:5]):
            arr[j].factors[q] = f
    return arr


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
    assert ctypes.sizeof(Term) == 56 and "mi355_msm_sumcheck_term" in header and "pub struct SumcheckTerm" in rust and "pub mod mle" in rust
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for word in ("mle_fix_variables", "mle_evaluate", "eq_table", "sumcheck_round", "mi355_msm_domain_sumcheck_round"):
        assert word in hpp, word
    for word in ("mle_work_bytes", "sumcheck_max_tables", "sumcheck_max_terms", "sumcheck_max_factors", "There is no CPU fallback",
                 "a lane's pair is another block's output"):
        assert word in full, word
    for f in ("mle_fix_variables", "mle_evaluate", "eq_table", "sumcheck_round", "sumcheck_prove"):
        assert hasattr(ea.Radix2EvaluationDomain, f), f


def test_no_new_device_twin_in_the_header():
    """one call each with a flag bit: the names that end in _device( are exactly those of stream_cases.COVERED, which this change
    leaves alone, and the header says in one sentence that this is the route the sparse handle took"""
    text = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    names = set(re.findall(r"\b(mi355_msm_\w+_device)\s*\(", text))
    assert names == {n for n in st.COVERED if n.endswith("_device")}
    assert not [n for n in names if "mle" in n or "sumcheck" in n]
    assert "this is the route mi355_msm_sparse_apply took" in text and "tests/test_gpu_mle.py" in text


def test_python_signatures(ea):
    d = ea.Radix2EvaluationDomain
    assert list(inspect.signature(d.mle_fix_variables).parameters) == ["self", "evals", "point", "montgomery", "out"]
    assert list(inspect.signature(d.mle_evaluate).parameters) == ["self", "evals", "point", "montgomery"]
    assert list(inspect.signature(d.eq_table).parameters)[:4] == ["self", "point", "montgomery", "out"]
    assert list(inspect.signature(d.sumcheck_round).parameters) == ["self", "tables", "terms", "r_prev", "montgomery", "out"]
    assert list(inspect.signature(d.sumcheck_prove).parameters) == ["self", "tables", "terms", "challenge", "montgomery"]
    assert inspect.signature(d.sumcheck_round).parameters["r_prev"].default is None


def test_the_limit_queries_need_no_handle(ea):
    lib = ea.load_library()
    v = ctypes.c_uint64()
    for key, want in ((b"sumcheck_max_tables", 12), (b"sumcheck_max_terms", 8), (b"sumcheck_max_factors", 5)):
        assert lib.mi355_msm_domain_query(None, key, ctypes.byref(v)).code == 0 and v.value == want
    for key in (b"mle_work_bytes", b"poly_work_bytes", b"size"):
        err = lib.mi355_msm_domain_query(None, key, ctypes.byref(v))
        assert err.code == -1 and b"null argument" in _free(err)


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: a null handle is enough to reach each refusal.  No pointer below
    is ever dereferenced as a vector: with a null handle every call ends at the handle check at the latest."""
    lib = ea.load_library()
    fix, eq, rnd = lib.mi355_msm_domain_mle_fix, lib.mi355_msm_domain_mle_eq, lib.mi355_msm_domain_sumcheck_round
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    q = p + (1 << 15)
    pt = bytes(32 * 31)
    ev = ctypes.create_string_buffer(32 * 6)
    fake = ctypes.c_void_p(64)                                    # a stream that is never used: the call is refused first
    far = 1 << 40                                                 # addresses that only the overlap check ever looks at

    def ptrs(*a):
        return (ctypes.c_void_p * len(a))(*a)

    t1 = terms_of([[0]])
    spartan = terms_of([[0, 1, 2], [0, 3]])
    t8, t9 = terms_of([[0]] * 8), terms_of([[0]] * 9)
    f5, f6, f0 = terms_of([[0, 0, 0, 0, 0]]), terms_of([[0]]), terms_of([[0]])
    f6[0].n_factors = 6
    f0[0].n_factors = 0
    tabs12, tabs13 = ptrs(*[far + (i << 36) for i in range(12)]), ptrs(*[far + (i << 36) for i in range(13)])
    tabs4 = ptrs(*[far + (i << 36) for i in range(4)])
    fold4 = ptrs(*[(far << 1) + (i << 36) for i in range(4)])
    r32 = bytes(32)
    calls = [
        # unknown flag bits
        (fix(None, p, q, 3, pt, 1, 4, None), b"flag bits 0x4"),
        (eq(None, p, pt, 3, 0x10, None), b"flag bits 0x10"),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, None, None, 8, None), b"flag bits 0x8"),
        # sizes: num_vars 30 / 31, k > num_vars, m 12 / 13 and 0, 8 / 9 terms and 0, nv == 1 with r_prev, nv == 0
        (fix(None, far, far << 2, 30, pt, 30, 0, None), HANDLE),
        (fix(None, far, far << 2, 31, pt, 30, 0, None), b"31 variables exceed 30"),
        (fix(None, p, q, 3, pt, 4, 0, None), b"4 variables to fix exceed the 3"),
        (fix(None, p, q, 3, pt, 3, 0, None), HANDLE),
        (eq(None, far, pt, 30, 0, None), HANDLE),
        (eq(None, far, pt, 31, 0, None), b"31 variables exceed 30"),
        (rnd(None, ev, tabs12, 12, 30, t1, 1, None, None, 0, None), HANDLE),
        (rnd(None, ev, tabs13, 13, 3, t1, 1, None, None, 0, None), b"13 tables"),
        (rnd(None, ev, tabs4, 0, 3, t1, 1, None, None, 0, None), b"0 tables"),
        (rnd(None, ev, tabs4, 4, 31, t1, 1, None, None, 0, None), b"31 variables"),
        (rnd(None, ev, tabs4, 4, 0, t1, 1, None, None, 0, None), b"0 variables"),
        (rnd(None, ev, tabs4, 4, 3, t8, 8, None, None, 0, None), HANDLE),
        (rnd(None, ev, tabs4, 4, 3, t9, 9, None, None, 0, None), b"9 terms"),
        (rnd(None, ev, tabs4, 4, 3, t1, 0, None, None, 0, None), b"0 terms"),
        (rnd(None, ev, tabs4, 4, 1, t1, 1, r32, fold4, 0, None), b"one variable cannot be folded"),
        (rnd(None, ev, tabs4, 4, 2, t1, 1, r32, fold4, 0, None), HANDLE),
        (rnd(None, ev, tabs4, 4, 1, t1, 1, None, None, 0, None), HANDLE),
        # null pointers
        (fix(None, None, q, 3, pt, 1, 0, None), b"null"),
        (fix(None, p, None, 3, pt, 1, 0, None), b"null"),
        (fix(None, p, q, 3, None, 1, 0, None), b"null"),
        (fix(None, p, q, 3, None, 0, 0, None), HANDLE),               # k == 0 reads no point
        (eq(None, None, pt, 3, 0, None), b"null"),
        (eq(None, p, None, 3, 0, None), b"null"),
        (eq(None, p, None, 0, 0, None), HANDLE),
        (rnd(None, None, tabs4, 4, 3, spartan, 2, None, None, 0, None), b"null"),
        (rnd(None, ev, None, 4, 3, spartan, 2, None, None, 0, None), b"null"),
        (rnd(None, ev, tabs4, 4, 3, None, 2, None, None, 0, None), b"null"),
        (rnd(None, ev, ptrs(far, 0, far, far), 4, 3, spartan, 2, None, None, 0, None), b"null table"),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, r32, None, 0, None), b"null"),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, r32, ptrs(far << 1, 0, far << 2, far << 3), 0, None), b"null table"),
        # alignment (device pointers only)
        (fix(None, p + 2, q, 3, pt, 1, 2, None), b"aligned"),
        (fix(None, p, q + 1, 3, pt, 1, 3, None), b"aligned"),
        (fix(None, p + 2, q + 1, 3, pt, 1, 0, None), HANDLE),
        (eq(None, p + 1, pt, 3, 2, None), b"aligned"),
        (rnd(None, ev, ptrs(far, far + 2, far, far), 4, 3, spartan, 2, None, None, 2, None), b"aligned"),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, r32, ptrs(far << 1, (far << 2) + 1, far << 3, far << 4), 2, None), b"aligned"),
        # a stream without flag bit 1
        (fix(None, p, q, 3, pt, 1, 0, fake), b"stream goes with device pointers"),
        (eq(None, p, pt, 3, 1, fake), b"stream goes with device pointers"),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, None, None, 1, fake), b"stream goes with device pointers"),
        # overlap: out against in (out ends where in begins is allowed), folded against a table and against another folded table
        (fix(None, p, p, 3, pt, 1, 0, None), b"overlaps the input"),
        (fix(None, p + 32 * 7, p, 3, pt, 1, 2, fake), b"overlaps the input"),
        (fix(None, p + 32 * 8, p, 3, pt, 1, 0, None), HANDLE),
        (fix(None, p - 32 * 4 + 4, p, 3, pt, 1, 2, None), b"overlaps the input"),
        (fix(None, p - 32 * 4, p, 3, pt, 1, 0, None), HANDLE),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, r32, ptrs(far << 1, far << 2, far + (3 << 36) + 32 * 7, far << 3), 0, None), b"folded table 2 overlaps table 3"),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, r32, ptrs(far << 1, far << 2, far + (3 << 36) + 32 * 8, far << 3), 0, None), HANDLE),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, r32, ptrs(far << 1, far << 2, (far << 1) + 32 * 3, far << 3), 2, fake), b"folded table 0 overlaps folded table 2"),
        (rnd(None, ev, ptrs(far, far, far, far), 4, 3, spartan, 2, r32, fold4, 0, None), HANDLE),       # tables may repeat
        # the term list: 5 / 6 factors, none, a factor index == m
        (rnd(None, ev, tabs4, 4, 3, f5, 1, None, None, 0, None), HANDLE),
        (rnd(None, ev, tabs4, 4, 3, f6, 1, None, None, 0, None), b"term 0 has 6 factors"),
        (rnd(None, ev, tabs4, 4, 3, f0, 1, None, None, 0, None), b"term 0 has 0 factors"),
        (rnd(None, ev, tabs4, 3, 3, spartan, 2, None, None, 0, None), b"term 1: factor index 3 is not below the 3 tables"),
        (rnd(None, ev, tabs4, 4, 3, spartan, 2, None, None, 0, None), HANDLE),
        # the order: flags before sizes, sizes before pointers, pointers before alignment, alignment before the stream, the stream
        # before the overlap, the overlap before the term list, the term list before the handle
        (fix(None, None, None, 31, None, 32, 4, fake), b"flag bits 0x4"),
        (fix(None, None, None, 31, None, 32, 0, fake), b"31 variables exceed 30"),
        (fix(None, None, p + 1, 3, pt, 1, 2, None), b"null"),
        (fix(None, p + 1, p + 1, 3, pt, 1, 2, None), b"aligned"),
        (fix(None, p, p, 3, pt, 1, 0, fake), b"stream goes with device pointers"),
        (rnd(None, None, None, 13, 3, None, 9, None, None, 4, fake), b"flag bits 0x4"),
        (rnd(None, None, None, 13, 3, None, 9, None, None, 0, fake), b"13 tables"),
        (rnd(None, None, None, 4, 3, None, 9, None, None, 0, fake), b"9 terms"),
        (rnd(None, None, ptrs(far + 1, far, far, far), 4, 3, f6, 1, None, None, 2, None), b"null"),
        (rnd(None, ev, ptrs(far + 1, far, far, far), 4, 3, f6, 1, None, None, 0, fake), b"stream goes with device pointers"),
        (rnd(None, ev, ptrs(far + 1, far, far, far), 4, 3, f6, 1, None, None, 2, fake), b"aligned"),
        (rnd(None, ev, tabs4, 4, 3, f6, 1, r32, tabs4, 0, None), b"folded table 0 overlaps table 0"),
        (rnd(None, ev, tabs4, 4, 3, f6, 1, r32, fold4, 0, None), b"term 0 has 6 factors"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
