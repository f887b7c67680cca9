"""CPU: the lookup-table calls (mi355_msm_lookup_create, _count, _sorted, _query, _destroy) and mi355_msm_domain_logup_sum exist in every
layer with the same shape -- exported by libmi355msm.so, declared in the C header, in the Rust crate's extern block and in the Python
binding -- and judge their arguments before they look for a handle or a device: without a GPU no domain and so no table exists
(hipErrorNoDevice), and every refusal is still reached with a null handle, in the stated order (unknown flag bits, sizes outside their
limits, null pointers, alignment, a stream without flag bit 1, overlap, and last the handle)."""
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
ARITY = {"mi355_msm_lookup_create": 6, "mi355_msm_lookup_count": 8, "mi355_msm_lookup_sorted": 7, "mi355_msm_lookup_query": 3,
         "mi355_msm_lookup_destroy": 1, "mi355_msm_domain_logup_sum": 13}
DOMAIN = b"null domain handle"
HANDLE = b"null lookup handle"
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
    assert "pub mod lookup" in rust and "pub struct LookupTable" in rust and "pub unsafe fn logup_sum" in rust
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for word in ("struct LookupTable", "multiplicities", "sorted", "logup_sum", "mi355_msm_lookup_count", "mi355_msm_domain_logup_sum"):
        assert word in hpp, word
    for word in ("logup_work_bytes", "lookup_work_bytes", "max_probe", "A MISSING VALUE IS NOT AN ERROR", "A ZERO DENOMINATOR IS NOT AN ERROR",
                 "There is no CPU fallback", "h1 = s[:n], h2 = s[n-1:]", "No lane waits on another lane's progress"):
        assert word in full, word
    assert hasattr(ea, "LookupTable") and hasattr(ea.Radix2EvaluationDomain, "logup_sum")


def test_no_new_device_twin_in_the_header():
    text = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    names = set(re.findall(r"\b(mi355_msm_\w+_device)\s*\(", text))
    assert names == {n for n in st.COVERED if n.endswith("_device")}
    assert not [n for n in names if "lookup" in n or "logup" in n]
    assert "tests/test_gpu_lookup.py" in text


def test_python_signatures(ea):
    t = ea.LookupTable
    assert list(inspect.signature(t.__init__).parameters) == ["self", "dom", "table", "montgomery"]
    assert list(inspect.signature(t.multiplicities).parameters) == ["self", "values", "index"]
    assert list(inspect.signature(t.sorted).parameters) == ["self", "values", "out"]
    assert inspect.signature(t.multiplicities).parameters["index"].default is False
    assert list(inspect.signature(ea.Radix2EvaluationDomain.logup_sum).parameters) == ["self", "table", "mult", "values", "beta", "helpers", "montgomery", "out"]
    assert inspect.signature(ea.Radix2EvaluationDomain.logup_sum).parameters["helpers"].default is False
    assert "linear_combination([a, b, c], [1, zeta" in ea.Radix2EvaluationDomain.logup_sum.__doc__
    for f in ("query", "close"):
        assert hasattr(t, f)


def test_without_a_gpu_no_table_can_exist(ea):
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
    for key in (b"n", b"slots", b"distinct", b"max_probe", b"table_bytes", b"lookup_work_bytes", b"nonsense"):
        err = lib.mi355_msm_lookup_query(None, key, ctypes.byref(v))
        assert err.code == -1 and HANDLE in _free(err)
    err = lib.mi355_msm_domain_query(None, b"logup_work_bytes", ctypes.byref(v))
    assert err.code == -1 and b"null argument" in _free(err)
    assert lib.mi355_msm_lookup_destroy(None).code == 0


def test_argument_errors_come_before_the_handle_and_the_device(ea):
    """-1 and a message that names the fault, with or without a GPU: a null handle is enough to reach each refusal.  No pointer below
    is ever dereferenced: with a null handle every call ends at the handle check at the latest."""
    lib = ea.load_library()
    create, count, srt, logup = lib.mi355_msm_lookup_create, lib.mi355_msm_lookup_count, lib.mi355_msm_lookup_sorted, lib.mi355_msm_domain_logup_sum
    buf = np.zeros(1 << 16, dtype=np.uint8)
    p = buf.ctypes.data
    q = p + (1 << 15)
    h = ctypes.c_void_p()
    hp = ctypes.byref(h)
    stats = (ctypes.c_uint64 * 2)()
    fake = ctypes.c_void_p(64)                                    # a stream that is never used: the call is refused first
    far = 1 << 40                                                 # addresses that only the overlap check ever looks at
    b32 = bytes(32)
    calls = [
        # unknown flag bits
        (create(hp, None, p, 4, 4, None), b"flag bits 0x4"),
        (count(None, p, None, stats, q, 4, 8, None), b"flag bits 0x8"),
        (srt(None, p, stats, q, 4, 0x10, None), b"flag bits 0x10"),
        (logup(None, p, None, None, far, far << 1, far << 2, 1, 4, 4, b32, 4, None), b"flag bits 0x4"),
        # sizes: n_t 0, 2^28 / 2^28 + 1; n_f 2^30 / 2^30 + 1; m 0, 8 / 9; stride below n, above 2^30; n 2^30 + 1
        (create(hp, None, p, 0, 0, None), b"at least one entry"),
        (create(hp, None, p, 1 << 28, 0, None), DOMAIN),
        (create(hp, None, p, (1 << 28) + 1, 0, None), b"exceed 2^28"),
        (count(None, far, None, stats, far << 2, 1 << 30, 0, None), HANDLE),
        (count(None, p, None, stats, q, (1 << 30) + 1, 0, None), b"exceed 2^30"),
        (srt(None, far, stats, far << 2, 1 << 30, 0, None), HANDLE),
        (srt(None, p, stats, q, (1 << 30) + 1, 0, None), b"exceed 2^30"),
        (logup(None, p, None, None, far, far << 1, far << 2, 0, 4, 4, b32, 0, None), b"0 columns"),
        (logup(None, p, None, None, far, far << 1, far << 2, 9, 4, 4, b32, 0, None), b"9 columns"),
        (logup(None, p, None, None, far, far << 1, far << 2, 8, 4, 4, b32, 0, None), DOMAIN),
        (logup(None, p, None, None, far, far << 1, far << 2, 2, 3, 4, b32, 0, None), b"stride of 3 elements is below the 4 rows"),
        (logup(None, p, None, None, far, far << 1, far << 2, 2, (1 << 30) + 1, 4, b32, 0, None), b"exceeds 2^30"),
        (logup(None, p, None, None, far, far << 1, far << 2, 1, 1 << 31, (1 << 30) + 1, b32, 0, None), b"rows exceed 2^30"),
        # null pointers
        (create(None, None, p, 4, 0, None), b"null"),
        (create(hp, None, None, 4, 0, None), b"null"),
        (count(None, p, None, None, q, 4, 0, None), b"null"),
        (count(None, p, None, stats, None, 4, 0, None), b"null"),
        (count(None, None, None, stats, None, 0, 0, None), HANDLE),                 # no values, no outputs: nothing to point at
        (srt(None, None, stats, q, 4, 0, None), b"null"),
        (srt(None, p, None, q, 4, 0, None), b"null"),
        (srt(None, p, stats, None, 4, 0, None), b"null"),
        (logup(None, None, None, None, far, far << 1, far << 2, 1, 4, 4, b32, 0, None), b"null"),
        (logup(None, p, None, None, None, far << 1, far << 2, 1, 4, 4, b32, 0, None), b"null"),
        (logup(None, p, None, None, far, None, far << 2, 1, 4, 4, b32, 0, None), b"null"),
        (logup(None, p, None, None, far, far << 1, None, 1, 4, 4, b32, 0, None), b"null"),
        (logup(None, p, None, None, far, far << 1, far << 2, 1, 4, 4, None, 0, None), b"null"),
        (logup(None, None, None, None, None, None, None, 1, 0, 0, b32, 0, None), DOMAIN),   # n == 0 reads no vector
        # alignment (device pointers only)
        (create(hp, None, p + 2, 4, 2, None), b"aligned"),
        (create(hp, None, p + 2, 4, 0, None), DOMAIN),
        (count(None, p + 1, None, stats, q, 4, 2, None), b"aligned"),
        (count(None, p, p + 4098, stats, q, 4, 3, None), b"aligned"),
        (count(None, p, None, stats, q + 3, 4, 2, None), b"aligned"),
        (count(None, p + 1, None, stats, q + 3, 4, 0, None), HANDLE),
        (srt(None, p + 2, stats, q, 4, 2, None), b"aligned"),
        (logup(None, p, None, p + 4097, far, far << 1, far << 2, 1, 4, 4, b32, 2, None), b"aligned"),
        (logup(None, p, None, None, far, (far << 1) + 2, far << 2, 1, 4, 4, b32, 2, None), b"aligned"),
        # a stream without flag bit 1
        (create(hp, None, p, 4, 0, fake), b"stream goes with device pointers"),
        (count(None, p, None, stats, q, 4, 1, fake), b"stream goes with device pointers"),
        (srt(None, p, stats, q, 4, 0, fake), b"stream goes with device pointers"),
        (logup(None, p, None, None, far, far << 1, far << 2, 1, 4, 4, b32, 1, fake), b"stream goes with device pointers"),
        # overlap: what can be judged without the table's size
        (count(None, q, None, stats, q, 4, 0, None), b"overlaps the values"),
        (count(None, p, q + 32, stats, q, 4, 2, fake), b"overlaps the values"),
        (count(None, p, q + 32 * 4, stats, q, 4, 0, None), HANDLE),
        (srt(None, q - 32 * 3, stats, q, 4, 0, None), b"overlaps the values"),
        (srt(None, q - 32 * 4, stats, q, 4, 0, None), HANDLE),                       # (the rest of s_out is judged against the handle)
        (logup(None, p, None, None, p + 32 * 3, far << 1, far << 2, 1, 4, 4, b32, 0, None), b"output overlaps an input"),
        (logup(None, p, None, None, far, p, far << 2, 1, 4, 4, b32, 2, fake), b"output overlaps an input"),
        (logup(None, p, None, None, far, far << 1, p - 32 * 7, 2, 4, 4, b32, 0, None), b"output overlaps an input"),
        (logup(None, p, None, None, far, far << 1, p - 32 * 8, 2, 4, 4, b32, 0, None), DOMAIN),
        (logup(None, p, None, q, far, q + 32 * 11, far << 2, 2, 4, 4, b32, 0, None), b"output overlaps an input"),   # helpers: (m + 1) n = 12
        (logup(None, p, None, q, far, q + 32 * 12, far << 2, 2, 4, 4, b32, 0, None), DOMAIN),
        (logup(None, q + 32 * 11, None, q, far, far << 1, far << 2, 2, 4, 4, b32, 0, None), b"overlaps the helper columns"),
        # the order: flags before sizes, sizes before pointers, pointers before alignment, alignment before the stream, the stream
        # before the overlap, the overlap before the handle
        (create(None, None, None, 0, 4, fake), b"flag bits 0x4"),
        (create(None, None, None, 0, 0, fake), b"at least one entry"),
        (create(None, None, p + 1, 4, 2, None), b"null"),
        (create(hp, None, p + 1, 4, 2, fake), b"aligned"),
        (create(hp, None, p, 4, 0, fake), b"stream goes with device pointers"),
        (count(None, None, None, None, None, (1 << 30) + 1, 4, fake), b"flag bits 0x4"),
        (count(None, None, None, None, None, (1 << 30) + 1, 0, fake), b"exceed 2^30"),
        (count(None, q + 1, None, None, q, 4, 2, None), b"null"),
        (count(None, q + 1, None, stats, q, 4, 0, fake), b"stream goes with device pointers"),
        (count(None, q + 1, None, stats, q, 4, 2, fake), b"aligned"),
        (count(None, q, None, stats, q, 4, 2, fake), b"overlaps the values"),
        (logup(None, None, None, None, None, None, None, 9, 1, 4, None, 4, fake), b"flag bits 0x4"),
        (logup(None, None, None, None, None, None, None, 9, 1, 4, None, 0, fake), b"9 columns"),
        (logup(None, None, None, None, None, None, None, 1, 1, 4, None, 0, fake), b"stride of 1"),
        (logup(None, p + 1, None, None, p, None, None, 1, 4, 4, b32, 2, None), b"null"),
        (logup(None, p + 1, None, None, p, far, far << 1, 1, 4, 4, b32, 0, fake), b"stream goes with device pointers"),
        (logup(None, p + 1, None, None, p, far, far << 1, 1, 4, 4, b32, 2, fake), b"aligned"),
        (logup(None, p, None, None, p, far, far << 1, 1, 4, 4, b32, 2, fake), b"output overlaps an input"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)
    assert not h.value


class _NoDevice:
    """the wrapper's own checks run before any call into the library: a stand-in handle is enough to reach them"""

    def __init__(self, ea):
        self.d = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
        self.d.curve, self.d.modulus, self.d.size, self.d.device = 1, nc.modulus("bls12_381"), 16, 0
        self.d.handle = ctypes.c_void_p(1)       # never dereferenced: every case below is refused in Python
        self.d._lib = None
        self.t = ea.LookupTable.__new__(ea.LookupTable)
        self.t.dom, self.t._lib, self.t.handle, self.t.n, self.t._flags = self.d, None, ctypes.c_void_p(1), 5, 0

    def __enter__(self):
        return self.d, self.t

    def __exit__(self, *exc):
        self.d.handle = ctypes.c_void_p()
        self.t.handle = ctypes.c_void_p()


def test_python_wrappers_check_shapes(ea):
    with _NoDevice(ea) as (d, t):
        for bad in (b"", bytes(33), np.zeros(31, np.uint8)):
            with pytest.raises(ValueError, match="table: a whole number"):
                ea.LookupTable(d, bad)
        for call in (t.multiplicities, t.sorted):
            with pytest.raises(ValueError, match="values: a whole number"):
                call(bytes(65))
        with pytest.raises(ValueError, match="out= goes with GPU tensors"):
            t.sorted(bytes(64), out=np.zeros((7, 32), np.uint8))
        with pytest.raises(ValueError, match="same number of 32-byte elements"):
            d.logup_sum(bytes(64), bytes(96), bytes(64), 1)
        with pytest.raises(ValueError, match="values: 2 32-byte elements"):
            d.logup_sum(bytes(64), bytes(64), bytes(96), 1)
        with pytest.raises(ValueError, match=r"values: m columns"):
            d.logup_sum(bytes(64), bytes(64), np.zeros((9, 2, 32), np.uint8), 1)
        with pytest.raises(ValueError, match=r"values: m columns"):
            d.logup_sum(bytes(64), bytes(64), np.zeros((2, 1, 32), np.uint8), 1)
    closed = ea.LookupTable.__new__(ea.LookupTable)
    closed.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        closed.multiplicities(bytes(32))
    dom = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
    dom.handle = ctypes.c_void_p()
    with pytest.raises(ea.MsmError, match="closed"):
        dom.logup_sum(bytes(32), bytes(32), bytes(32), 1)
    with pytest.raises(ea.MsmError, match="closed"):
        ea.LookupTable(dom, bytes(32))
