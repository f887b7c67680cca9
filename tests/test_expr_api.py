"""CPU: the expression calls (mi355_msm_expr_create, _run, _query, _destroy) exist in every layer with the same shape -- exported by
libmi355msm.so, declared in the C header, in the Rust crate's extern block, in the C++ mirror and in the Python binding -- and judge
their arguments before they look for a handle or a device: without a GPU no domain and so no program exists (hipErrorNoDevice), and
every refusal that does not need the program is still reached with a null handle.  Also here: the Python builder (hash-consing, the
products of a power, the flat nodes)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import expr_cases as xc
import stream_cases as st
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
ARITY = {"mi355_msm_expr_create": 9, "mi355_msm_expr_run": 11, "mi355_msm_expr_query": 3, "mi355_msm_expr_destroy": 1}
DOMAIN = b"null domain handle"
HANDLE = b"null expression handle"
HIP_ERROR_NO_DEVICE = 100


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
    assert "pub mod expr" in rust and "pub struct GateProgram" in rust
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for word in ("struct GateProgram", "mi355_msm_expr_create", "mi355_msm_expr_run", "mi355_msm_expr_query", "mi355_msm_expr_destroy"):
        assert word in hpp, word
    for word in ("evaluate_h", "rot * rot_step", "lds_bytes", "rotation 0 only", "There is no CPU fallback", "names S and the limit"):
        assert word in full, word
    assert hasattr(ea, "Expr") and hasattr(ea, "GateProgram") and hasattr(ea.Radix2EvaluationDomain, "compile_expression")


def test_no_new_device_twin_in_the_header():
    text = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    names = set(re.findall(r"\b(mi355_msm_\w+_device)\s*\(", text))
    assert names == {n for n in st.COVERED if n.endswith("_device")}
    assert not [n for n in names if "expr" in n]
    assert "tests/test_gpu_expr.py" in text


def test_python_signatures(ea):
    g = ea.GateProgram
    assert list(inspect.signature(ea.Radix2EvaluationDomain.compile_expression).parameters) == ["self", "expr", "ncols"]
    assert list(inspect.signature(g.run).parameters) == ["self", "cols", "challenges", "rot_step", "montgomery", "out"]
    p = inspect.signature(g.run).parameters
    assert p["challenges"].default == () and p["rot_step"].default == 1 and p["montgomery"].default is True and p["out"].default is None
    assert list(inspect.signature(ea.Expr.col).parameters) == ["j", "rot"] and inspect.signature(ea.Expr.col).parameters["rot"].default == 0
    for f in ("query", "close"):
        assert hasattr(g, f)


def test_builder_hash_consing_and_powers(ea):
    E = ea.Expr
    a, b = E.col(0), E.col(1, -1)
    assert E.col(0) is a and E.col(1, -1) is b and E.col(1, 1) is not b
    assert E.const(5) is E.const(5) and E.challenge(2) is E.challenge(2) and E.const(5) is not E.challenge(5)
    assert a + b is a + b and a + b is b + a and a * b is b * a and a - b is not b - a
    assert (a + b) * (a + b) is (b + a) ** 2 and -a is -a
    assert a + 3 is 3 + a and a + 3 is a + E.const(3)
    assert a ** 1 is a and a ** 0 is E.const(1)
    with pytest.raises(TypeError):
        E(0, 0, 0)
    with pytest.raises(TypeError):
        a + 1.5
    with pytest.raises(ValueError):
        a ** -1

    def count(e, ops):
        return sum(1 for op, _, _ in e.nodes()[0] if op in ops)

    nodes, consts, n_chal, n_cols = (a ** 5).nodes()
    assert nodes == [(xc.COL, 0, 0), (xc.SQR, 0, 0), (xc.SQR, 1, 0), (xc.MUL, 0, 2)] or nodes == [(xc.COL, 0, 0), (xc.SQR, 0, 0), (xc.SQR, 1, 0), (xc.MUL, 2, 0)]
    assert count(a ** 5, (xc.MUL, xc.SQR)) == 3 and count(a ** 16, (xc.MUL, xc.SQR)) == 4 and count(a ** 7, (xc.MUL, xc.SQR)) == 4
    # equal sub-expressions become ONE node, however often they are written
    s = (a + b) * (a + b) + (b + a) * E.challenge(1) - (a + b)
    nodes, consts, n_chal, n_cols = s.nodes(101)
    assert [op for op, _, _ in nodes].count(xc.ADD) == 2 and len(nodes) == 8 and n_chal == 2 and n_cols == 2
    assert nodes[-1][0] == xc.SUB and all(x < i and (op not in (xc.ADD, xc.SUB, xc.MUL) or y < i) for i, (op, x, y) in enumerate(nodes) if op > xc.CHAL)
    assert (xc.COL, 1, 0xFFFFFFFF) in nodes
    # constants are reduced modulo the field and shared
    nodes, consts, _, _ = (a * 102 + 1 + b * E.const(-100)).nodes(101)
    assert consts == [1] and [op for op, _, _ in nodes].count(xc.CONST) == 1
    # the nodes evaluate to what the expression says
    cols = [[3, 4, 5], [7, 8, 9]]
    e = (a + b) ** 3 - a * b + 11
    nodes, consts, n_chal, n_cols = e.nodes()
    r = xc.nc.modulus("bls12_381")
    want = [((cols[0][i] + cols[1][(i - 1) % 3]) ** 3 - cols[0][i] * cols[1][(i - 1) % 3] + 11) % r for i in range(3)]
    assert xc.evaluate("bls12_381", nodes, consts, [], cols, 3) == want


def test_without_a_gpu_no_program_can_exist(ea):
    import torch

    lib = ea.load_library()
    h = ctypes.c_void_p()
    err = lib.mi355_msm_domain_create(ctypes.byref(h), 1, -1, 16)
    if torch.cuda.is_available():
        assert err.code == 0 and h.value
        assert lib.mi355_msm_domain_destroy(h).code == 0
    else:
        assert err.code == HIP_ERROR_NO_DEVICE and not h.value
        _free(err)
    v = ctypes.c_uint64()
    for key in (b"nodes", b"instructions", b"slots", b"products", b"reduces", b"columns", b"lds_bytes", b"last_us", b"last_device_us", b"nonsense"):
        err = lib.mi355_msm_expr_query(None, key, ctypes.byref(v))
        assert err.code == -1 and HANDLE in _free(err)
    assert b"null argument" in _free(lib.mi355_msm_expr_query(None, None, ctypes.byref(v)))
    assert lib.mi355_msm_expr_destroy(None).code == 0


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: a null handle is enough to reach each refusal.  No column is ever
    dereferenced: with a null handle every call ends at the handle check at the latest."""
    lib = ea.load_library()
    create, run = lib.mi355_msm_expr_create, lib.mi355_msm_expr_run
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    q = p + (1 << 15)
    h = ctypes.c_void_p()
    hp = ctypes.byref(h)
    fake = ctypes.c_void_p(64)                                    # a stream that is never used: the call is refused first
    far = 1 << 40                                                 # addresses that only the overlap check ever looks at
    b32 = bytes(32)

    def nodes(*triples):
        return (ctypes.c_uint32 * (3 * len(triples)))(*[w for t in triples for w in t])

    def ptrs(*a):
        return (ctypes.c_void_p * len(a))(*a)

    def lens(*a):
        return (ctypes.c_size_t * len(a))(*a)

    one = nodes((xc.COL, 0, 0))
    many = (ctypes.c_uint32 * (3 * 65536))()
    calls = [
        # create: flag bits, null pointers, the limits of the DAG, and last the domain
        (create(hp, None, one, 1, None, 0, 0, 1, 2), b"flag bits 0x2"),
        (create(None, None, one, 1, None, 0, 0, 1, 0), b"null handle out-pointer"),
        (create(hp, None, None, 1, None, 0, 0, 1, 0), b"node pointer"),
        (create(hp, None, one, 1, None, 1, 0, 1, 0), b"constant pointer"),
        (create(hp, None, one, 0, None, 0, 0, 1, 0), b"at least one node"),
        (create(hp, None, many, 65536, None, 0, 0, 1, 0), b"65536 nodes exceed 65535"),
        (create(hp, None, one, 1, b32, 4097, 0, 1, 0), b"4097 constants exceed 4096"),
        (create(hp, None, one, 1, None, 0, 65, 1, 0), b"65 challenges exceed 64"),
        (create(hp, None, one, 1, None, 0, 0, 65, 0), b"65 columns exceed 64"),
        (create(hp, None, nodes((xc.COL, 0, (1 << 15) + 1)), 1, None, 0, 0, 1, 0), b"outside +-2^15"),
        (create(hp, None, nodes((xc.COL, 0, xc.u32(-(1 << 15) - 1))), 1, None, 0, 0, 1, 0), b"outside +-2^15"),
        (create(hp, None, nodes((xc.COL, 1, 0)), 1, None, 0, 0, 1, 0), b"column 1 of 1"),
        (create(hp, None, nodes((xc.CONST, 0, 0)), 1, None, 0, 0, 1, 0), b"constant 0 of 0"),
        (create(hp, None, nodes((xc.CHAL, 1, 0)), 1, None, 0, 1, 1, 0), b"challenge 1 of 1"),
        (create(hp, None, nodes((8, 0, 0)), 1, None, 0, 0, 1, 0), b"unknown op 8"),
        (create(hp, None, nodes((xc.COL, 0, 0), (xc.ADD, 0, 1)), 2, None, 0, 0, 1, 0), b"topological order"),
        (create(hp, None, nodes((xc.COL, 0, xc.u32(-(1 << 15))), (xc.SQR, 0, 0)), 2, None, 0, 0, 64, 0), DOMAIN),
        # run: flag bits; len above 2^30; too many columns or challenges; null pointers
        (run(None, p, ptrs(q), lens(4), 1, 4, 1, None, 0, 4, None), b"flag bits 0x4"),
        (run(None, p, ptrs(q), lens(4), 1, 4, 1, None, 0, 0x11, None), b"flag bits 0x11"),
        (run(None, far, ptrs(far << 2), lens(1 << 30), 1, 1 << 30, 1, None, 0, 0, None), HANDLE),
        (run(None, p, ptrs(q), lens(1), 1, (1 << 30) + 1, 1, None, 0, 0, None), b"exceed 2^30"),
        (run(None, p, ptrs(q), lens(4), 65, 4, 1, None, 0, 0, None), b"65 columns exceed 64"),
        (run(None, p, ptrs(q), lens(4), 1, 4, 1, b32, 65, 0, None), b"65 challenges exceed 64"),
        (run(None, None, ptrs(q), lens(4), 1, 4, 1, None, 0, 0, None), b"null output"),
        (run(None, p, None, lens(4), 1, 4, 1, None, 0, 0, None), b"null output, column"),
        (run(None, p, ptrs(q), None, 1, 4, 1, None, 0, 0, None), b"null output, column, length"),
        (run(None, p, ptrs(q), lens(4), 1, 4, 1, None, 1, 0, None), b"challenge pointer"),
        # a length of 0; one that does not divide len; a null column
        (run(None, p, ptrs(q, q), lens(4, 0), 2, 4, 1, None, 0, 0, None), b"column 1 has length 0"),
        (run(None, p, ptrs(q, q), lens(4, 3), 2, 4, 1, None, 0, 0, None), b"length 3 of column 1 does not divide the 4 rows"),
        (run(None, p, ptrs(q, q), lens(8, 4), 2, 4, 1, None, 0, 0, None), b"length 8 of column 0 does not divide"),
        (run(None, p, ptrs(q, None), lens(4, 1), 2, 4, 1, None, 0, 0, None), b"column 1 is a null pointer"),
        # alignment of device pointers; a stream without flag bit 1
        (run(None, p + 2, ptrs(q), lens(4), 1, 4, 1, None, 0, 2, None), b"4-byte aligned"),
        (run(None, p, ptrs(q + 1), lens(4), 1, 4, 1, None, 0, 2, None), b"4-byte aligned"),
        (run(None, p, ptrs(q), lens(4), 1, 4, 1, None, 0, 0, fake), b"flag bit 1"),
        # an overlap in part (the whole of a full-length column is judged against the program)
        (run(None, p, ptrs(q, p + 32), lens(4, 4), 2, 4, 1, None, 0, 0, None), b"the output overlaps column 1"),
        (run(None, p, ptrs(q, p), lens(4, 2), 2, 4, 1, None, 0, 0, None), b"the output overlaps column 1"),
        (run(None, p, ptrs(p, q), lens(4, 2), 2, 4, 1, None, 0, 0, None), HANDLE),
        # len = 0 judges the same and ends at the handle
        (run(None, None, ptrs(q), lens(4), 1, 0, 1, None, 0, 0, None), HANDLE),
        (run(None, p, ptrs(q), lens(4), 1, 4, 1, b32, 1, 0, None), HANDLE),
    ]
    for err, word in calls:
        assert err.code == -1, word
        msg = _free(err)
        assert word in msg, (word, msg)
    assert not h.value
