"""CPU: the Poseidon handle (mi355_msm_poseidon_create, _hash, _merkle, _set_option, _query, _destroy) exists in every layer with the
same shape -- exported by libmi355msm.so, declared in the C header, in the C++ mirror, in the Rust crate's extern block and in the
Python binding -- and judges its arguments before it looks for a handle or a device: without a GPU no domain and so no handle exists,
and every refusal is still reached with a null handle, in the stated order (unknown flag bits, sizes outside their limits, null
pointers, alignment, a stream without flag bit 1, overlap, and last the handle)."""
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
    "mi355_msm_poseidon_create": 9,
    "mi355_msm_poseidon_hash": 9,
    "mi355_msm_poseidon_merkle": 8,
    "mi355_msm_poseidon_set_option": 3,
    "mi355_msm_poseidon_query": 3,
    "mi355_msm_poseidon_destroy": 1,
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
    assert "pub struct Poseidon" in rust and "pub mod poseidon" in rust
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for word in ("struct Poseidon", "mi355_msm_poseidon_hash", "mi355_msm_poseidon_merkle", "merkle_tree"):
        assert word in hpp, word
    for word in ("products_per_permutation", "work_bytes", "MUST OUTLIVE THE", "There is\n * no CPU fallback", "hash_many", "\"sparse\""):
        assert word in full, word
    for f in ("sponge", "hash_many", "hash", "merkle_tree", "set_option", "query", "close"):
        assert hasattr(ea.Poseidon, f), f
    for f in ("root", "path", "empty_hash"):
        assert hasattr(ea.PoseidonMerkleTree, f), f
    assert callable(ea.poseidon_parameters)


def test_no_new_device_twin_in_the_header():
    """one call each with a flag bit: the names that end in _device( are exactly those of stream_cases.COVERED, which this change leaves alone"""
    text = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    names = set(re.findall(r"\b(mi355_msm_\w+_device)\s*\(", text))
    assert names == {n for n in st.COVERED if n.endswith("_device")}
    assert not [n for n in names if "poseidon" in n]
    assert "tests/test_gpu_poseidon.py" in text                              # the header says where the promise of flag bit 1 is pinned


def test_python_signatures(ea):
    sig = inspect.signature(ea.poseidon_parameters)
    assert list(sig.parameters) == ["curve", "rate", "alpha", "full_rounds", "partial_rounds", "skip_matrices"]
    assert sig.parameters["skip_matrices"].default == 0
    sig = inspect.signature(ea.Poseidon.__init__)
    assert list(sig.parameters) == ["self", "dom", "rate", "parameters", "domain"]
    assert sig.parameters["parameters"].default is None and sig.parameters["domain"].default is None
    for f, lead in (("sponge", ["self", "inputs", "n_out"]), ("hash_many", ["self", "inputs", "n_out"]), ("hash", ["self", "inputs"]),
                    ("merkle_tree", ["self", "leaves"])):
        sig = inspect.signature(getattr(ea.Poseidon, f))
        assert list(sig.parameters)[:len(lead)] == lead, f
        assert sig.parameters["montgomery"].default is True and sig.parameters["out"].default is None, f


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: a null handle is enough to reach each refusal"""
    lib = ea.load_library()
    create, hash_, merkle = lib.mi355_msm_poseidon_create, lib.mi355_msm_poseidon_hash, lib.mi355_msm_poseidon_merkle
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    buf = np.zeros(256 * 32, dtype=np.uint8)
    p = buf.ctypes.data
    q = p + 4096
    fake = ctypes.c_void_p(64)                                    # a stream that is never used: the call is refused first
    big = (1 << 30) + 1
    calls = [
        # unknown flag bits
        (create(out, None, 2, 17, 8, 31, p, q, 2), b"flag bits 0x2"),
        (hash_(None, p, q, 4, 2, 1, None, 4, None), b"flag bits 0x4"),
        (merkle(None, p, q, 4, 2, p + 64, 0x13, None), b"flag bits 0x13"),
        # sizes outside their limits
        (create(out, None, 0, 17, 8, 31, p, q, 0), b"rate must be 1 .. 8"),
        (create(out, None, 9, 17, 8, 31, p, q, 1), b"rate must be 1 .. 8"),
        (create(out, None, 2, 16, 8, 31, p, q, 0), b"alpha must be odd"),
        (create(out, None, 2, 1, 8, 31, p, q, 0), b"alpha must be odd"),
        (create(out, None, 2, 1 << 16 | 1, 8, 31, p, q, 0), b"alpha must be odd"),
        (create(out, None, 2, 17, 7, 31, p, q, 0), b"full_rounds must be even"),
        (create(out, None, 2, 17, 0, 31, p, q, 0), b"full_rounds must be even"),
        (create(out, None, 2, 17, 8, 5000, p, q, 0), b"partial_rounds exceed"),
        (hash_(None, p, q, big, 2, 1, None, 0, None), b"sponges exceed 2^30"),
        (hash_(None, p, q, 4, (1 << 16) + 1, 1, None, 0, None), b"input elements per sponge exceed 2^16"),
        (hash_(None, p, q, 4, 2, (1 << 16) + 1, None, 2, None), b"output elements per sponge exceed 2^16"),
        (merkle(None, p, q, 0, 2, p + 64, 0, None), b"a tree has 1 .. 2^30"),
        (merkle(None, p, q, big, 2, p + 64, 0, None), b"a tree has 1 .. 2^30"),
        (merkle(None, p, q, 4, 1 << 16, p + 64, 0, None), b"per leaf exceed"),
        # null pointers
        (create(None, None, 2, 17, 8, 31, p, q, 0), b"null"),
        (create(out, None, 2, 17, 8, 31, None, q, 0), b"null"),
        (create(out, None, 2, 17, 8, 31, p, None, 0), b"null"),
        (hash_(None, None, q, 4, 2, 1, None, 0, None), b"null input or output"),
        (hash_(None, p, None, 4, 2, 1, None, 2, None), b"null input or output"),
        (merkle(None, None, q, 4, 2, p + 64, 0, None), b"null tree"),
        (merkle(None, p, None, 4, 2, p + 64, 0, None), b"null tree"),
        (merkle(None, p, q, 4, 2, None, 0, None), b"null tree"),
        # alignment (device pointers)
        (hash_(None, p + 2, q, 4, 2, 1, None, 2, None), b"aligned"),
        (hash_(None, p, q + 1, 4, 2, 1, None, 3, None), b"aligned"),
        (merkle(None, p + 1, q, 4, 2, p + 64, 2, None), b"aligned"),
        # a stream without flag bit 1
        (hash_(None, p, q, 4, 2, 1, None, 0, fake), b"stream goes with device pointers"),
        (merkle(None, p, q, 4, 2, p + 64, 1, fake), b"stream goes with device pointers"),
        # overlap, with its whole extent: the sizes are arguments of the call
        (hash_(None, p, p, 4, 2, 1, None, 0, None), b"overlaps the input"),
        (hash_(None, p + 32 * 7, p, 4, 2, 1, None, 2, fake), b"overlaps the input"),          # the last input element
        (hash_(None, p, p + 32 * 3, 4, 2, 1, None, 0, None), b"overlaps the input"),          # the last output element
        (merkle(None, p, p + 32 * 6, 4, 2, p + 4096, 0, None), b"overlaps the leaves"),       # the root level is 7 nodes
        # the order
        (create(None, None, 0, 17, 8, 31, None, None, 2), b"flag bits 0x2"),
        (create(None, None, 0, 17, 8, 31, None, None, 0), b"rate must be"),
        (hash_(None, None, None, big, 2, 1, None, 4, fake), b"flag bits 0x4"),
        (hash_(None, None, None, big, 2, 1, None, 0, fake), b"exceed 2^30"),
        (hash_(None, None, q + 1, 4, 2, 1, None, 2, None), b"null input or output"),
        (hash_(None, p + 1, p + 1, 4, 2, 1, None, 2, None), b"aligned"),
        (hash_(None, p, p, 4, 2, 1, None, 0, fake), b"stream goes with device pointers"),
        (merkle(None, p + 1, p + 1, 4, 2, p + 64, 0, fake), b"stream goes with device pointers"),
        # and, with everything else in order, the handle; nothing to do is no excuse
        (create(out, None, 2, 17, 8, 31, p, q, 0), b"null domain handle"),
        (create(out, None, 8, 3, 2, 0, p, q, 1), b"null domain handle"),
        (hash_(None, p, q, 4, 2, 1, None, 0, None), b"null parameter handle"),
        (hash_(None, p, p + 32 * 4, 4, 2, 1, None, 2, fake), b"null parameter handle"),       # adjacent, not overlapping
        (hash_(None, None, None, 0, 0, 0, None, 0, None), b"null parameter handle"),
        (hash_(None, None, q, 4, 2, 0, None, 0, None), b"null parameter handle"),
        (merkle(None, p, q, 4, 2, p + 4096 + 256, 3, fake), b"null parameter handle"),
        (merkle(None, p, None, 4, 0, p + 64, 0, None), b"null parameter handle"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
        assert not h.value, i
    v = ctypes.c_uint64()
    for key in (b"rate", b"state", b"rounds", b"products_per_permutation", b"work_bytes"):
        err = lib.mi355_msm_poseidon_query(None, key, ctypes.byref(v))
        assert err.code == -1 and b"null parameter handle" in _free(err)
    assert lib.mi355_msm_poseidon_query(None, b"block_lanes", ctypes.byref(v)).code == 0 and v.value >= 32
    err = lib.mi355_msm_poseidon_set_option(None, b"sparse", 0)
    assert err.code == -1 and b"null parameter handle" in _free(err)
    assert lib.mi355_msm_poseidon_destroy(None).code == 0


def test_python_wrappers_check_before_the_library(ea):
    dom = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
    dom.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        ea.Poseidon(dom, 2)
    dom.handle, dom._lib, dom.curve, dom.modulus, dom.device = ctypes.c_void_p(1), None, 1, nc.modulus("bls12_381"), 0
    try:
        with pytest.raises(ValueError, match="fixes none for BLS12-381"):
            ea.Poseidon(dom, 2)
        with pytest.raises(ValueError, match="ark: 39 rows of 3"):
            ea.Poseidon(dom, 2, parameters=dict(alpha=17, full_rounds=8, partial_rounds=31, ark=[[1, 2, 3]], mds=[[1]]))
    finally:
        dom.handle = ctypes.c_void_p()
    closed = ea.Poseidon.__new__(ea.Poseidon)
    closed.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        closed.sponge(bytes(64), 1, in_len=2)
    with pytest.raises(ea.MsmError, match="closed"):
        closed.merkle_tree(bytes(64), leaf_len=1)
