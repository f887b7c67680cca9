"""CPU: the hash-to-curve handle (mi355_msm_h2c_create, _field, _map, _hash, _query, _destroy) exists in every layer with the same
shape -- exported by libmi355msm.so, declared in the C header, in the C++ mirror, in the Rust crate's extern block and in the Python
binding -- and judges its arguments before it looks for a handle or a device: every refusal is reached with a null handle, in the
stated order (unknown flag bits; count, or an odd n with pairs; the stride; null pointers; alignment; a stream without flag bit 1;
bad offsets of a host-pointer call; and last the handle -- for create, the out-pointer, the curve, the tag, BLS12-377, the device)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import stream_cases as st
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
ARITY = {
    "mi355_msm_h2c_create": 5,
    "mi355_msm_h2c_field": 9,
    "mi355_msm_h2c_map": 7,
    "mi355_msm_h2c_hash": 9,
    "mi355_msm_h2c_query": 3,
    "mi355_msm_h2c_destroy": 1,
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
    assert "pub struct HashToCurve" in rust and "pub mod h2c" in rust
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for word in ("struct HashToCurve", "mi355_msm_h2c_hash", "mi355_msm_h2c_field", "mi355_msm_h2c_map", "hash_to_field"):
        assert word in hpp, word
    for word in ("work_bytes", "lanes_in_flight", "last_launches", "H2C-OVERSIZE-DST-", "no CPU fallback", "no standard", "kilobyte messages"):
        assert word in full, word
    for f in ("hash", "encode", "hash_to_field", "map_to_curve", "query", "close"):
        assert hasattr(ea.HashToCurve, f), f
    build = open(os.path.join(PKG, "build.py")).read()
    assert '"kernels_h2c.hip"' in build
    for name in ("h2c.hpp", "kernels_h2c.hip", "launch_h2c.hpp", "msm_h2c.hpp", "h2c_consts.inc"):
        assert os.path.exists(os.path.join(PKG, "csrc", name)), name


def test_no_new_device_twin_in_the_header():
    """one call each with a flag bit: the names that end in _device( are exactly those of stream_cases.COVERED, which this change leaves alone"""
    text = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    names = set(re.findall(r"\b(mi355_msm_\w+_device)\s*\(", text))
    assert names == {n for n in st.COVERED if n.endswith("_device")}
    assert not [n for n in names if "h2c" in n]
    assert "tests/test_gpu_h2c.py" in text                                   # the header says where the promise of flag bit 1 is pinned


def test_python_signatures(ea):
    sig = inspect.signature(ea.HashToCurve.__init__)
    assert list(sig.parameters) == ["self", "curve", "dst", "device"]
    assert sig.parameters["curve"].default == "bls12_381_g2" and sig.parameters["device"].default is None
    for name in ("hash", "encode"):
        sig = inspect.signature(getattr(ea.HashToCurve, name))
        assert list(sig.parameters) == ["self", "msgs", "projective", "out"]
        assert sig.parameters["projective"].default is False and sig.parameters["out"].default is None
    sig = inspect.signature(ea.HashToCurve.hash_to_field)
    assert list(sig.parameters)[:3] == ["self", "msgs", "count"] and sig.parameters["count"].default == 2
    sig = inspect.signature(ea.HashToCurve.map_to_curve)
    assert list(sig.parameters)[:3] == ["self", "u", "pairs"] and sig.parameters["pairs"].default is False


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: a null handle is enough to reach each refusal"""
    lib = ea.load_library()
    create, field, mapc, hashc = lib.mi355_msm_h2c_create, lib.mi355_msm_h2c_field, lib.mi355_msm_h2c_map, lib.mi355_msm_h2c_hash
    h = ctypes.c_void_p()
    buf = np.zeros(1 << 16, dtype=np.uint8)
    o = buf.ctypes.data                  # output
    d = o + 8192                         # 100 bytes of messages
    u = o + 16384                        # field images
    offs = np.array([0, 10, 10, 100], dtype=np.uint64)
    bad1 = np.array([0, 20, 10, 100], dtype=np.uint64)
    bad2 = np.array([0, 10, 10, 101], dtype=np.uint64)
    of, b1, b2 = offs.ctypes.data, bad1.ctypes.data, bad2.ctypes.data
    tag = ctypes.create_string_buffer(b"tag")
    fake = ctypes.c_void_p(64)           # a stream that is never used: the call is refused first
    calls = [
        # 1: unknown flag bits (field knows bit 1 alone; map has no bit 0; hash has no bit 2)
        (field(None, o, d, 100, of, 3, 2, 1, None), b"flag bits 0x1"),
        (field(None, o, d, 100, of, 3, 2, 8, None), b"flag bits 0x8"),
        (mapc(None, o, 104, u, 4, 1, None), b"flag bits 0x1"),
        (hashc(None, o, 104, d, 100, of, 3, 4, None), b"flag bits 0x4"),
        (hashc(None, o, 104, d, 100, of, 3, 16, None), b"flag bits 0x10"),
        # 2: count; an odd n with pairs
        (field(None, o, d, 100, of, 3, 0, 0, None), b"count 0"),
        (field(None, o, d, 100, of, 3, 3, 0, None), b"count 3"),
        (mapc(None, o, 104, u, 3, 4, None), b"not whole pairs"),
        # 3: the stride
        (mapc(None, o, 100, u, 4, 0, None), b"out_stride 100"),
        (hashc(None, o, 106, d, 100, of, 3, 0, None), b"out_stride 106"),
        (hashc(None, o, 104, d, 100, of, 3, 8, None), b"out_stride 104"),
        # 4: null pointers
        (field(None, None, d, 100, of, 3, 2, 0, None), b"null output"),
        (mapc(None, o, 104, None, 4, 0, None), b"null output or input"),
        (hashc(None, o, 104, d, 100, None, 3, 0, None), b"null offsets"),
        (hashc(None, o, 104, None, 100, of, 3, 0, None), b"null message buffer"),
        # 5: alignment (device pointers)
        (hashc(None, o + 2, 104, d, 100, of, 3, 2, None), b"aligned"),
        (mapc(None, o, 104, u + 1, 4, 2, None), b"aligned"),
        (field(None, o, d, 100, of + 4, 3, 2, 2, None), b"aligned"),
        # 6: a stream without flag bit 1
        (hashc(None, o, 104, d, 100, of, 3, 0, fake), b"stream goes with device pointers"),
        (mapc(None, o, 104, u, 4, 0, fake), b"stream goes with device pointers"),
        # 7: the offsets of a host-pointer call (with device pointers they are not read)
        (hashc(None, o, 104, d, 100, b1, 3, 0, None), b"offsets decrease"),
        (field(None, o, d, 100, b2, 3, 2, 0, None), b"outside the message buffer"),
        (hashc(None, o, 104, d, 100, b1, 3, 2, None), b"null hash-to-curve handle"),
        # the order
        (hashc(None, None, 100, None, 100, None, 3, 4, fake), b"flag bits 0x4"),
        (mapc(None, None, 100, None, 3, 4, fake), b"not whole pairs"),
        (mapc(None, None, 100, None, 4, 4, fake), b"out_stride 100"),
        (hashc(None, None, 104, d, 100, b1, 3, 0, fake), b"null output"),
        (hashc(None, o + 2, 104, d, 100, b1, 3, 2, None), b"aligned"),
        (hashc(None, o, 104, d, 100, b1, 3, 0, fake), b"stream goes with device pointers"),
        (hashc(None, o, 104, d, 100, b1, 3, 0, None), b"offsets decrease"),
        # 8: and, with everything else in order, the handle; nothing to do is no excuse
        (hashc(None, o, 104, d, 100, of, 3, 0, None), b"null hash-to-curve handle"),
        (hashc(None, o, 200, d, 100, of, 3, 11, fake), b"null hash-to-curve handle"),
        (field(None, o, d, 100, of, 3, 1, 0, None), b"null hash-to-curve handle"),
        (mapc(None, o, 104, u, 4, 4, None), b"null hash-to-curve handle"),
        (hashc(None, None, 104, None, 0, of, 0, 0, None), b"null hash-to-curve handle"),
        # create: the out-pointer, the curve, the tag, then BLS12-377 -- before any device is looked for
        (create(None, 1, tag, 3, -1), b"null handle out-pointer"),
        (create(ctypes.byref(h), 4, tag, 3, -1), b"unknown curve id 4"),
        (create(ctypes.byref(h), 0, None, 3, -1), b"domain separation tag"),
        (create(ctypes.byref(h), 3, tag, 0, -1), b"domain separation tag"),
        (create(ctypes.byref(h), 0, tag, 3, -1), b"no standard hash-to-curve suite"),
        (create(ctypes.byref(h), 2, tag, 3, 99), b"no standard hash-to-curve suite"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
        assert not h.value, i
    v = ctypes.c_uint64()
    for key in (b"work_bytes", b"lanes_in_flight", b"last_launches", b"device", b"dst_bytes"):
        err = lib.mi355_msm_h2c_query(None, key, ctypes.byref(v))
        assert err.code == -1 and b"null hash-to-curve handle" in _free(err)
    assert lib.mi355_msm_h2c_query(None, b"block_lanes", ctypes.byref(v)).code == 0 and v.value == 256
    assert lib.mi355_msm_h2c_query(None, b"max_lanes", ctypes.byref(v)).code == 0 and v.value == 131072
    err = lib.mi355_msm_h2c_query(None, b"slots", ctypes.byref(v))
    assert err.code == -1 and b"null hash-to-curve handle" in _free(err)     # no such constant: the slot counts differ by field
    assert lib.mi355_msm_h2c_destroy(None).code == 0


def test_python_wrapper_checks_before_the_library(ea):
    closed = ea.HashToCurve.__new__(ea.HashToCurve)
    closed.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        closed.hash([b"abc"])
    with pytest.raises(ea.MsmError, match="closed"):
        closed.map_to_curve(bytes(48))
    fake = ea.HashToCurve.__new__(ea.HashToCurve)
    fake.handle, fake._lib, fake.device, fake.m, fake.curve = ctypes.c_void_p(1), None, 0, 2, 3
    try:
        with pytest.raises(ValueError, match="n images of 96 bytes"):
            fake.map_to_curve(bytes(100))
        with pytest.raises(ValueError, match="not whole pairs"):
            fake.map_to_curve(bytes(96 * 3), pairs=True)
        with pytest.raises(ValueError, match="count is 1 or 2"):
            fake.hash_to_field([b"a"], count=3)
        with pytest.raises(ValueError, match="shape"):
            fake.hash(np.zeros(7, dtype=np.uint8))
    finally:
        fake.handle = ctypes.c_void_p()
