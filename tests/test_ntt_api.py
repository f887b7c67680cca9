"""CPU: the domain entry points exist in every layer with the same shape -- exported by libmi355msm.so, declared in the C header, in the
Rust crate's extern block and in the Python binding -- and refuse bad arguments before they look for a device."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
ARITY = {
    "mi355_msm_domain_create": 4,
    "mi355_msm_domain_transform": 8,
    "mi355_msm_domain_transform_device": 9,
    "mi355_msm_domain_mul": 6,
    "mi355_msm_domain_mul_device": 7,
    "mi355_msm_domain_set_option": 3,
    "mi355_msm_domain_query": 3,
    "mi355_msm_domain_element": 3,
    "mi355_msm_domain_destroy": 1,
}
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
    assert "typedef struct mi355_msm_domain mi355_msm_domain;" in header
    hpp = open(os.path.join(ROOT, "include", "mi355_msm.hpp")).read()
    for item in ("struct Radix2EvaluationDomain", "coset_ifft", "element"):
        assert item in hpp, item
    for f in ("fft", "ifft", "coset_fft", "coset_ifft", "mul", "element", "group_gen", "size_inv", "query", "set_option", "close"):
        assert hasattr(ea.Radix2EvaluationDomain, f), f


def test_argument_errors_come_before_the_device(ea):
    """-1 and a message, with or without a GPU: the arguments are judged first"""
    lib = ea.load_library()
    h = ctypes.c_void_p()
    for args, word in (((None, 0, -1, 16), b"null"), ((ctypes.byref(h), 7, -1, 16), b"curve"), ((ctypes.byref(h), -1, -1, 16), b"curve"),
                       ((ctypes.byref(h), 1, -1, (1 << 28) + 1), b"2^28"), ((ctypes.byref(h), 3, -1, (1 << 32) + 1), b"2-adicity"),
                       ((ctypes.byref(h), 0, -1, (1 << 32) + 1), b"2^28"), ((ctypes.byref(h), 2, -1, 1 << 63), b"2-adicity")):
        err = lib.mi355_msm_domain_create(*args)
        assert err.code == -1, args
        assert word in _free(err), args
        assert not h.value
    out = ctypes.create_string_buffer(32)
    v = ctypes.c_uint64()
    for err in (lib.mi355_msm_domain_transform(None, out, out, 1, 1, 0, 0, None), lib.mi355_msm_domain_transform_device(None, out, out, 1, 1, 0, 0, None, None),
                lib.mi355_msm_domain_mul(None, out, out, out, 1, 0), lib.mi355_msm_domain_mul_device(None, out, out, out, 1, 0, None),
                lib.mi355_msm_domain_query(None, b"size", ctypes.byref(v)), lib.mi355_msm_domain_set_option(None, b"pass_log", 1),
                lib.mi355_msm_domain_element(None, 0, out)):
        assert err.code == -1
        assert _free(err)
    err = lib.mi355_msm_domain_destroy(None)                     # like free(NULL)
    assert err.code == 0 and not err.message
    with pytest.raises(ValueError):
        ea.Radix2EvaluationDomain(16, curve="no_such_curve")


def test_create_without_a_gpu_says_so(ea):
    import torch

    lib = ea.load_library()
    h = ctypes.c_void_p()
    err = lib.mi355_msm_domain_create(ctypes.byref(h), 1, -1, 1000)
    if torch.cuda.is_available():
        assert err.code == 0 and h.value
        v = ctypes.c_uint64()
        assert lib.mi355_msm_domain_query(h, b"size", ctypes.byref(v)).code == 0 and v.value == 1024
        assert lib.mi355_msm_domain_destroy(h).code == 0
    else:
        assert err.code == HIP_ERROR_NO_DEVICE and not h.value
        assert b"no HIP device" in _free(err)
        with pytest.raises(ea.MsmError) as e:
            ea.Radix2EvaluationDomain(1000, curve="bls12_381_g1")
        assert e.value.code == HIP_ERROR_NO_DEVICE
