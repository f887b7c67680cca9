"""CPU: the transform over curve points (mi355_msm_fft_points[_device]) exists in every layer with the same shape -- exported by
libmi355msm.so, declared in the C header, in the Rust crate's extern block and in the Python binding -- and refuses what it must
before any device call.  Without a GPU no context and no domain exist, so the refusals that are judged against a handle are pinned on
the function the engine calls for them (gf_check_call of csrc/group_fft.hpp, through the host build: ht_gf_check) and, with live
handles, in tests/test_gpu_gfft.py; the ones that need no handle are reached through the C ABI itself with null handles."""
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
ARITY = {"mi355_msm_fft_points": 10, "mi355_msm_fft_points_device": 11}
HIP_ERROR_NO_DEVICE = 100
LIMIT = 64 << 30


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
    assert "mi355_msm_fft_points" in hpp and "ifft_points" in hpp
    full = open(os.path.join(ROOT, "include", "mi355_msm.h")).read()
    for word in ("fft_points_work_bytes", "fft_points_chunk", "last_fft_points_us", "last_fft_points_device_us"):
        assert word in full, word


def test_python_signature(ea):
    sig = inspect.signature(ea.MultiScalarMultContext.fft_points)
    assert list(sig.parameters)[:3] == ["self", "dom", "points"]
    for name in ("kind", "inverse", "coset", "offset", "in_len", "projective", "out", "stride", "out_stride"):
        assert name in sig.parameters, name
    assert hasattr(ea.MultiScalarMultContext, "ifft_points")


def test_refusals_that_need_no_handle(ea):
    """an unknown kind, unknown flag bits and an offset on kinds 0 and 1 are judged first; then the handles"""
    lib = ea.load_library()
    buf = np.zeros(8 * 104, dtype=np.uint8)
    p = buf.ctypes.data
    off = ctypes.create_string_buffer(32)
    calls = [
        (lib.mi355_msm_fft_points(None, None, p, 104, p, 4, 104, 4, 0, None), b"unknown transform kind 4"),
        (lib.mi355_msm_fft_points_device(None, None, p, 104, p, 4, 104, 7, 0, None, None), b"unknown transform kind 7"),
        (lib.mi355_msm_fft_points(None, None, p, 104, p, 4, 104, 0, 1, None), b"flag bits 0x1"),
        (lib.mi355_msm_fft_points_device(None, None, p, 104, p, 4, 104, 3, 6, None, None), b"flag bits 0x6"),
        (lib.mi355_msm_fft_points(None, None, p, 104, p, 4, 104, 0, 0, off), b"not over a coset"),
        (lib.mi355_msm_fft_points_device(None, None, p, 104, p, 4, 104, 1, 2, off, None), b"not over a coset"),
        (lib.mi355_msm_fft_points(None, None, p, 104, p, 4, 104, 2, 2, off), b"null context"),
        (lib.mi355_msm_fft_points_device(None, None, p, 104, p, 4, 104, 0, 0, None, None), b"null context"),
    ]
    for i, (err, word) in enumerate(calls):
        assert err.code == -1, i
        msg = _free(err)
        assert word in msg, (i, word, msg)


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(PKG, "libmsm_hosttest.so"))
    sz, ci, cu, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p
    lib.ht_gf_check.argtypes = [ci, ci, ci, ci, ci, cu, vp, sz, vp, sz, sz, cu, cu, ci, ci, sz, ctypes.c_char_p, sz]
    return lib


def _check(ht, ctx_curve=1, sharded=0, ctx_device=0, dom_curve=1, dom_device=0, k=4, out=0x10000, out_stride=104, inp=0x20000, in_len=16, stride=104,
           kind=0, flags=0, has_offset=0, offset_is_zero=0, limit=LIMIT):
    msg = ctypes.create_string_buffer(256)
    rc = ht.ht_gf_check(ctx_curve, sharded, ctx_device, dom_curve, dom_device, k, out, out_stride, inp, in_len, stride, kind, flags, has_offset,
                        offset_is_zero, limit, msg, 256)
    assert (rc == 0) == (msg.value == b"")
    return rc, msg.value


def test_every_refusal_is_decided_from_plain_values(ht):
    """gf_check_call is the whole judgement of a call (the engine adds the null handles, the alignment of device pointers and the zero
    test of the offset's value): no device, no handle"""
    ok = [
        dict(),
        dict(ctx_curve=3, dom_curve=1, stride=200, out_stride=200),             # G2 points over the family's domain
        dict(ctx_curve=0, dom_curve=2),                                         # any curve id names the family
        dict(kind=2, has_offset=1), dict(kind=3, has_offset=1), dict(kind=1),
        dict(flags=2, out_stride=144),                                          # Projective images
        dict(in_len=0, inp=0),                                                  # nothing to read
        dict(inp=0x10000, out=0x10000),                                         # in place, equal strides
        dict(inp=0x10000, out=0x10000, stride=112, out_stride=112),
        dict(inp=0x10000 + 16 * 104, out=0x10000),                              # back to back
        dict(inp=0x10000, out=0x10000 + 5 * 104, in_len=5),                     # the output begins where the bytes read end
        dict(k=0, in_len=1), dict(k=0, in_len=0, inp=0),
        dict(k=28, in_len=1, inp=0x1000),                                               # 2^28 G1 points: 2 * 2^28 * 104 bytes of work vectors
        dict(ctx_device=3, dom_device=3),
    ]
    for kw in ok:
        assert _check(ht, **kw) == (0, b""), kw
    bad = [
        (dict(kind=4), b"unknown transform kind 4"),
        (dict(flags=1), b"flag bits 0x1"),
        (dict(flags=4), b"flag bits 0x4"),
        (dict(kind=0, has_offset=1), b"not over a coset"),
        (dict(kind=1, has_offset=1), b"not over a coset"),
        (dict(kind=2, has_offset=1, offset_is_zero=1), b"offset is zero"),
        (dict(sharded=1), b"sharded context"),
        (dict(ctx_curve=0, dom_curve=1), b"different curve families"),
        (dict(ctx_curve=3, dom_curve=0, stride=200, out_stride=200), b"different curve families"),
        (dict(ctx_device=0, dom_device=1), b"device 1"),
        (dict(in_len=17), b"in_len 17 exceeds the domain size 16"),
        (dict(k=0, in_len=2), b"exceeds the domain size 1"),
        (dict(stride=96), b"stride 96"),
        (dict(stride=106), b"stride 106"),
        (dict(ctx_curve=2, dom_curve=0, stride=104, out_stride=200), b"stride 104"),
        (dict(out_stride=100), b"out_stride 100"),
        (dict(out_stride=106), b"out_stride 106"),
        (dict(flags=2, out_stride=104), b"out_stride 104"),
        (dict(out=0), b"null input or output"),
        (dict(inp=0), b"null input or output"),
        (dict(inp=0x10000, out=0x10000 + 104), b"overlap in part"),
        (dict(inp=0x10000 + 104, out=0x10000), b"overlap in part"),
        (dict(inp=0x10000, out=0x10000, stride=104, out_stride=112), b"overlap in part"),     # the same start, other strides
        (dict(inp=0x10000, out=0x10000 + 5 * 104 - 8, in_len=5), b"overlap in part"),
        (dict(inp=0x10000 + 16 * 104 - 8, out=0x10000), b"overlap in part"),
        (dict(k=28, in_len=1, inp=0x1000, ctx_curve=3, stride=200, out_stride=200), b"work vectors"),        # 2 * 2^28 * 200 bytes > 64 GiB
        (dict(k=20, in_len=1, inp=0x1000, limit=1 << 27), b"work vectors"),
    ]
    for kw, word in bad:
        rc, msg = _check(ht, **kw)
        assert rc == -1 and word in msg, (kw, msg)


def test_without_a_gpu_the_call_says_so(ea):
    """there is no CPU fallback: the entry points judge a call without handles the same with and without a device and compute nothing;
    without a device neither handle can be made, and the wrapper passes the runtime's code on"""
    import torch

    lib = ea.load_library()
    buf = np.zeros(104, dtype=np.uint8)
    for err in (lib.mi355_msm_fft_points(None, None, buf.ctypes.data, 104, None, 0, 104, 0, 0, None),
                lib.mi355_msm_fft_points_device(None, None, buf.ctypes.data, 104, None, 0, 104, 1, 0, None, None)):
        assert err.code == -1 and b"null context" in _free(err)
    assert not buf.any()
    if torch.cuda.is_available():
        ctx = ea.MultiScalarMultContext("bls12_381_g1")
        try:
            assert ctx.query("fft_points_work_bytes") == 0 and ctx.query("fft_points_chunk") == 1 << 19
            assert ctx.query("last_fft_points_us") == 0 and ctx.query("last_fft_points_device_us") == 0
        finally:
            ctx.close()
    else:
        with pytest.raises(ea.MsmError) as e:
            ea.Radix2EvaluationDomain(16, curve="bls12_381_g1")
        assert e.value.code == HIP_ERROR_NO_DEVICE
        with pytest.raises(ea.MsmError) as e:
            ea.MultiScalarMultContext("bls12_381_g1")
        assert e.value.code == HIP_ERROR_NO_DEVICE


class _Stand:
    """the wrapper's own checks run before any call into the library: stand-in handles are enough to reach them"""

    def __init__(self, ea):
        self.ctx = ea.MultiScalarMultContext.__new__(ea.MultiScalarMultContext)
        self.ctx.curve, self.ctx.context, self.ctx._lib = 1, ctypes.c_void_p(1), None
        self.dom = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
        self.dom.curve, self.dom.size, self.dom.device, self.dom.handle, self.dom._lib = 1, 16, 0, ctypes.c_void_p(1), None
        self.dom.modulus = nc.modulus("bls12_381")

    def __enter__(self):
        return self.ctx, self.dom

    def __exit__(self, *exc):
        self.ctx.context = ctypes.c_void_p()
        self.dom.handle = ctypes.c_void_p()


def test_python_wrapper_checks_shapes(ea):
    with _Stand(ea) as (ctx, dom):
        pts = bytes(104 * 4)
        with pytest.raises(ValueError, match="not both"):
            ctx.fft_points(dom, pts, kind=1, inverse=True)
        with pytest.raises(ValueError, match="kind 4"):
            ctx.fft_points(dom, pts, kind=4)
        with pytest.raises(ValueError, match="coset kinds"):
            ctx.fft_points(dom, pts, offset=5)
        with pytest.raises(ValueError, match="stride 96"):
            ctx.fft_points(dom, pts, stride=96)
        with pytest.raises(ValueError, match="out_stride 104"):
            ctx.fft_points(dom, pts, projective=True, out_stride=104)
        with pytest.raises(ValueError, match="not a multiple"):
            ctx.fft_points(dom, bytes(105))
        with pytest.raises(ValueError, match="in_len 5"):
            ctx.fft_points(dom, pts, in_len=5)
        with pytest.raises(ValueError, match="exceed the domain size"):
            ctx.fft_points(dom, bytes(104 * 17))
        with pytest.raises(ValueError, match="out= goes with GPU tensors"):
            ctx.fft_points(dom, pts, out=np.zeros(16 * 104, dtype=np.uint8))
        closed = ea.Radix2EvaluationDomain.__new__(ea.Radix2EvaluationDomain)
        closed.handle = ctypes.c_void_p()
        with pytest.raises(ea.MsmError, match="closed"):
            ctx.fft_points(closed, pts)
