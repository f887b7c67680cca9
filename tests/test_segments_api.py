"""CPU: the segmented MSM (mi355_msm_segments) exists in every layer with the same shape -- exported by libmi355msm.so, declared in
the C header, in the Rust crate's extern block and in the Python binding; its C++ wrapper is a header of its own that compiles without
a warning, and include/mi355_msm.hpp does not know the call; the Python argument checks fire before any GPU work; without a GPU the
call itself fails with the no-device error."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
NAME = "mi355_msm_segments"
ARITY = 12
HIP_ERROR_NO_DEVICE = 100


def test_symbol_exported_and_declared_everywhere(ea):
    lib = ea.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "libmi355msm.so")], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert NAME in exported
    assert not any(s.startswith(NAME) and s.endswith("_device") for s in exported)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355_msm.h")).read(), flags=re.S)
    c_decls = {name: len(params.split(",")) for name, params in re.findall(r"\b(\w+)\s*\(([^;{}()]*)\)\s*;", header)}
    assert c_decls.get(NAME) == ARITY, c_decls.get(NAME)
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    rust_items = {}
    for block in re.findall(r'extern\s+"C"\s*\{(.*?)\n\s*\}', rust, flags=re.S):
        for name, params in re.findall(r"fn\s+(\w+)\s*\((.*?)\)\s*(?:->\s*[\w:]+)?\s*;", block, flags=re.S):
            rust_items[name] = len([p for p in params.strip().rstrip(",").split(",") if p.strip()])
    assert rust_items.get(NAME) == ARITY, rust_items.get(NAME)
    assert "pub unsafe fn msm_segments(" in rust and "pub unsafe fn msm_segments_shared(" in rust
    assert len(getattr(lib, NAME).argtypes) == ARITY
    assert hasattr(ea, "msm_segments") and hasattr(ea.MultiScalarMultContext, "msm_segments")
    full = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    for word in ("seg_window", "seg_tile", "seg_chunk", "seg_work_bytes", "last_segments_us"):
        assert word in full, word


def test_cpp_wrapper_is_its_own_header_and_compiles_clean(tmp_path):
    assert NAME not in open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    src = tmp_path / "use.cpp"
    src.write_text('#include "mi355_msm_segments.hpp"\n'
                   "int use(mi355::MultiScalarMultContext& c, const std::vector<mi355::G1Affine>& p, const std::vector<mi355::BigInteger256>& s) {\n"
                   "  std::vector<uint64_t> o = {0, p.size()};\n"
                   "  return (int)(mi355::msm_segments(c, p, s, o).size() + mi355::msm_segments_shared(c, p, s, 1).size());\n}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr


def test_python_argument_checks_fire_before_any_gpu_work(ea):
    pts = np.zeros((10, 104), dtype=np.uint8)
    s = np.zeros((10, 32), dtype=np.uint8)
    call = lambda *a, **k: ea.msm_segments(*a, curve="bls12_381_g1", **k)
    bad = [
        (dict(offsets=[0, 4, 3, 10]), r"offsets\[2\] = 3 is smaller"),
        (dict(offsets=[1, 10]), r"offsets\[0\] = 1"),
        (dict(offsets=[0, 9]), r"offsets\[1\] = 9"),
        (dict(offsets=[0, 10], lengths=[10]), "one of them"),
        (dict(), "one of them"),
        (dict(offsets=[0.0, 10.0]), "integer"),
        (dict(lengths=[-1, 11]), "negative"),
        (dict(offsets=[0, 10], stride=102), "stride 102"),
        (dict(offsets=[0, 10], out_stride=100), "out_stride 100"),
        (dict(offsets=[0, 10], projective=True, out_stride=104), "out_stride 104"),
        (dict(offsets=[0, 10], shared=True), "neither offsets nor lengths"),
        (dict(offsets=[0, 10], out=np.zeros(104, dtype=np.uint8)), None),
    ]
    for kw, phrase in bad:
        with pytest.raises((ValueError, TypeError), match=phrase):
            call(pts, s, **kw)
    with pytest.raises(ValueError, match="not a multiple of the 10 points"):
        call(pts, np.zeros((25, 32), dtype=np.uint8), shared=True)
    with pytest.raises(ValueError, match=r"shape \(S, 10, 32\)"):
        call(pts, np.zeros((2, 5, 32), dtype=np.uint8), shared=True)
    with pytest.raises(ValueError, match="need 10 scalars"):
        call(pts, s[:9], offsets=[0, 10])
    with pytest.raises(ValueError):
        ea.msm_segments(pts, s, [0, 10], curve="no_such_curve")


def test_refusals_need_no_device_and_the_call_itself_reports_none(ea):
    lib = ea.load_library()
    free = ctypes.CDLL(None).free
    buf = np.zeros(4 * 104 + 4 * 32 + 4 * 104, dtype=np.uint8)
    P = buf.ctypes.data
    S, O = P + 4 * 104, P + 4 * 104 + 4 * 32
    offs = (ctypes.c_uint64 * 3)(0, 1, 4)
    err = lib.mi355_msm_segments(None, P, 4, 104, S, 4, offs, 2, 0, O, 104, None)
    assert err.code == -1 and b"null context" in ctypes.string_at(err.message)
    free(ctypes.c_void_p(err.message))
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    try:
        ctx = ea.MultiScalarMultContext("bls12_381_g1")
    except ea.MsmError as e:
        assert e.code == HIP_ERROR_NO_DEVICE
        return
    try:
        bad = (ctypes.c_uint64 * 3)(0, 5, 4)
        err = lib.mi355_msm_segments(ctx.context, P, 4, 104, S, 4, bad, 2, 0, O, 104, None)
        assert err.code == -1 and b"offsets[2] = 4 is smaller" in ctypes.string_at(err.message)
        free(ctypes.c_void_p(err.message))
        with pytest.raises(ea.MsmError) as ei:
            ctx.msm_segments(buf[:4 * 104], buf[4 * 104:4 * 104 + 128], [0, 1, 4])
        assert ei.value.code == HIP_ERROR_NO_DEVICE
    finally:
        ctx.close()
