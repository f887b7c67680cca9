"""GPU: the prefix scans and the permutation product on the domain handle (csrc/scan.hpp, csrc/msm_scan.hpp) through the Python layer,
byte for byte against Python big integers (tests/scan_cases.py), at the sizes where the plan gains a level, and the computation they
exist for -- a Plonk prover's second round, z -> ifft -> MSM -- end to end in device memory."""
import ctypes
import os
import random
import re
import statistics
import time

import numpy as np
import pytest

import ntt_cases as nc
import poly_cases as pc
import scan_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def domains(ea):
    """one domain per (field, k) for the whole module"""
    made = {}

    def get(field, k):
        if (field, k) not in made:
            made[(field, k)] = ea.Radix2EvaluationDomain(1 << k, CURVE_OF[field])
        d = made[(field, k)]
        d.set_option("poly_tile_log", 0)
        return d

    yield get
    for d in made.values():
        d.close()


def dev(torch, raw):
    return torch.frombuffer(bytearray(raw) if len(raw) else bytearray(32), dtype=torch.uint8).cuda()[:len(raw)].reshape(-1, 32)


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else (t.tobytes() if hasattr(t, "tobytes") else bytes(t))


def _check(ea, err):
    """a RustError of a direct call into the library -> MsmError, as the binding does"""
    if err.code != 0:
        msg = ctypes.string_at(err.message).decode() if err.message else ""
        if err.message:
            ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
        raise ea.MsmError(err.code, msg)


def ints(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


# ---- the host build's case list ------------------------------------------------------------------------------------------------------

def case_list(field, tile_log, op):
    """(raw patterns, position of the single zero or None) for every length of tests/test_scan_host.py"""
    lengths = pc.lengths(4) if tile_log == 4 else [0, 1, 1023, 1024, 1025, 3 * 1024 + 5]
    out = []
    for n in lengths:
        out.append((sc.vector(field, n, tile_log, 0xC0 + n), None))
        if op == sc.PRODUCT:
            out.append((sc.vector(field, n, tile_log, 0xD0 + n, zeros=False), None))
            out.append(sc.single_zero(field, n, tile_log, 0xE0 + n, which=n))
    return out


@pytest.mark.parametrize("tile_log", [4, 0])
@pytest.mark.parametrize("op", [sc.PRODUCT, sc.SUM])
@pytest.mark.parametrize("field", FIELDS)
def test_case_list_host_and_device_pointers(domains, torch_, field, op, tile_log):
    """every length and every planted pattern of tests/test_scan_host.py, from host memory, from GPU tensors with out= and in place:
    identical bytes, equal to Python's, and the same total"""
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 6)
    dom.set_option("poly_tile_log", tile_log)
    assert dom.query("poly_tile_log") == (tile_log or 10)
    call = dom.prefix_product if op == sc.PRODUCT else dom.prefix_sum
    for pattern, zero_at in case_list(field, tile_log or 10, op):
        n = len(pattern)
        raw = pc.to_raw(pattern)
        for montgomery in (True, False):
            vals = pc.values(field, pattern, not montgomery)
            for inclusive in (False, True):
                want, want_total = sc.ref_scan(vals, op, inclusive, r)
                want_raw = nc.encode(field, want, not montgomery)
                if zero_at is not None:
                    assert all(v == 0 for v in want[zero_at + 1:]) and all(v != 0 for v in want[:zero_at])
                got, total = call(raw, inclusive=inclusive, montgomery=montgomery)
                assert got == want_raw and total == want_total, (n, inclusive, "host pointers")
                x = dev(torch, raw)
                out = torch.full((n, 32), 0x55, dtype=torch.uint8, device="cuda")
                got, total = call(x, inclusive=inclusive, montgomery=montgomery, out=out)
                assert got.is_cuda and got.data_ptr() == out.data_ptr() and raw_of(got) == want_raw and total == want_total, (n, inclusive, "out=")
                assert raw_of(x) == raw                                  # the input is left alone
                got, total = call(x, inclusive=inclusive, montgomery=montgomery, out=x)
                assert raw_of(x) == want_raw and total == want_total, (n, inclusive, "in place")
    dom.set_option("poly_tile_log", 0)


# ---- at size -------------------------------------------------------------------------------------------------------------------------

def report_mismatches(got, want, tile):
    """got, want: (n, 32) uint8 arrays; fails with the count, the first indices and their tiles"""
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        first = bad[:8].tolist()
        pytest.fail("%d of %d outputs differ; first at %s (tiles %s, positions in the tile %s)"
                    % (bad.size, got.shape[0], first, [i // tile for i in first], [i % tile for i in first]))


@pytest.mark.parametrize("field,n,op,inclusive", [("bls12_377", (1 << 20) + 1025, sc.PRODUCT, False), ("bls12_381", (1 << 20) + 1025, sc.SUM, True),
                                                  ("bls12_381", 1 << 22, sc.PRODUCT, True), ("bls12_377", 1 << 22, sc.SUM, False)])
def test_at_size_every_output(domains, torch_, field, n, op, inclusive):
    """2^20 + 1025: the first three-level plan at the default tile, with a ragged last tile at two levels; 2^22.  Random 256-bit
    patterns (plain integers: the value is the pattern modulo r), every output against a Python loop"""
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 6)
    raw = np.random.default_rng(n + op).integers(0, 256, size=(n, 32), dtype=np.uint8)
    x = torch.from_numpy(raw).cuda()
    call = dom.prefix_product if op == sc.PRODUCT else dom.prefix_sum
    got, total = call(x, inclusive=inclusive, montgomery=False)
    got = got.cpu().numpy()
    buf = raw.tobytes()
    want = bytearray(n * 32)
    acc = 1 if op == sc.PRODUCT else 0
    for i in range(n):
        v = int.from_bytes(buf[32 * i:32 * i + 32], "little")
        if not inclusive:
            want[32 * i:32 * i + 32] = acc.to_bytes(32, "little")
        acc = acc * v % r if op == sc.PRODUCT else (acc + v) % r
        if inclusive:
            want[32 * i:32 * i + 32] = acc.to_bytes(32, "little")
    report_mismatches(got, np.frombuffer(bytes(want), dtype=np.uint8).reshape(n, 32), 1024)
    assert total == acc


# ---- the permutation product ---------------------------------------------------------------------------------------------------------

def perm_inputs(torch, p, montgomery, device=True):
    w = np.frombuffer(p.columns(p.wires, not montgomery, p.n), dtype=np.uint8).reshape(p.m, p.n, 32)
    s = np.frombuffer(p.columns(p.sigmas, not montgomery, p.n), dtype=np.uint8).reshape(p.m, p.n, 32)
    return (torch.from_numpy(w.copy()).cuda(), torch.from_numpy(s.copy()).cuda()) if device else (w, s)


@pytest.mark.parametrize("field", FIELDS)
def test_permutation_product_every_output(domains, torch_, field):
    """m = 5 at 2^16 rows: z and the total against the model for the valid, the broken and the zero-denominator instance, from GPU
    tensors and (the valid one) from host memory and from a list of column vectors"""
    torch = torch_
    k, m = 16, 5
    dom = domains(field, k)
    good = sc.permutation(field, k, m, 0x9E16)
    zden, zrow = sc.zero_denominator(good)
    for p, montgomery in ((good, True), (sc.broken(good, 3), False), (zden, True)):
        z, total = p.model()
        assert (total == 1) == (p is good) and (total == 0) == (p is zden)
        w, s = perm_inputs(torch, p, montgomery)
        got, got_total = dom.permutation_product(w, s, p.beta, p.gamma, p.ks, montgomery=montgomery)
        assert got.is_cuda and got_total == total
        report_mismatches(got.cpu().numpy(), np.frombuffer(nc.encode(field, z, not montgomery), dtype=np.uint8).reshape(-1, 32), 1024)
        if p is zden:
            assert z[zrow] != 0 and not any(z[zrow + 1:])
        if p is good:
            wh, sh = perm_inputs(torch, p, montgomery, device=False)
            host, host_total = dom.permutation_product(wh, sh, p.beta, p.gamma, p.ks, montgomery=montgomery)
            assert host_total == 1 and host.tobytes() == raw_of(got)
            lst, lst_total = dom.permutation_product([w[i] for i in range(m)], list(s), p.beta, p.gamma, p.ks, montgomery=montgomery)
            assert lst_total == 1 and raw_of(lst) == raw_of(got)


@pytest.mark.parametrize("field", FIELDS)
def test_permutation_product_stride_tile_and_refusals(domains, torch_, ea, field):
    """2^9 rows, m = 3: the columns n + 3 elements apart and a tile of 16 elements (three levels) give the bytes of the default; a
    stride below n and an output inside the columns are refused by the call itself"""
    torch = torch_
    k, m = 9, 3
    dom = domains(field, k)
    p = sc.permutation(field, k, m, 0x5709)
    z, total = p.model()
    want = nc.encode(field, z, False)
    w, s = perm_inputs(torch, p, True)
    got, t = dom.permutation_product(w, s, p.beta, p.gamma, p.ks)
    assert raw_of(got) == want and t == 1
    dom.set_option("poly_tile_log", 4)
    got4, t4 = dom.permutation_product(w, s, p.beta, p.gamma, p.ks)
    dom.set_option("poly_tile_log", 0)
    assert raw_of(got4) == want and t4 == 1
    stride = p.n + 3
    ws = dev(torch, p.columns(p.wires, False, stride))
    ss = dev(torch, p.columns(p.sigmas, False, stride))
    out = torch.empty((p.n, 32), dtype=torch.uint8, device="cuda")
    tot = ctypes.create_string_buffer(32)
    ks, beta, gamma = (nc.encode(field, v, False) for v in (p.ks, [p.beta], [p.gamma]))
    lib = dom._lib
    _check(ea, lib.mi355_msm_domain_permutation_product_device(dom.handle, out.data_ptr(), tot, ws.data_ptr(), ss.data_ptr(), m, stride, ks, beta, gamma, 0, None))
    torch.cuda.synchronize()
    assert raw_of(out) == want and nc.decode(field, tot.raw, False) == [1]
    _check(ea, lib.mi355_msm_domain_permutation_product_device(dom.handle, out.data_ptr(), None, ws.data_ptr(), ss.data_ptr(), m, stride, ks, beta, gamma, 0, None))
    for args, word in (((out.data_ptr(), tot, ws.data_ptr(), ss.data_ptr(), m, p.n - 1, ks, beta, gamma, 0, None), "stride"),
                       ((ws.data_ptr() + 32 * stride, tot, ws.data_ptr(), ss.data_ptr(), m, stride, ks, beta, gamma, 0, None), "overlaps"),
                       ((ss.data_ptr() + 32 * (p.n - 1), tot, ws.data_ptr(), ss.data_ptr(), m, stride, ks, beta, gamma, 0, None), "overlaps")):
        with pytest.raises(ea.MsmError, match=word) as e:
            _check(ea, lib.mi355_msm_domain_permutation_product_device(dom.handle, *args))
        assert e.value.code == -1


def big_permutation(field, k, m, seed):
    """a valid instance of 2^k rows built with NumPy: cells shuffled, cut into cycles of 1 .. 6, one random 256-bit pattern per cycle as
    the wire value (plain integers: any pattern is a value), sigma of a cell the id of the next cell of its cycle.  Returns
    (wires, sigmas: (m, n, 32) uint8; ks; the domain's elements; cell order; cycle starts)"""
    r = nc.modulus(field)
    n = 1 << k
    rng = np.random.default_rng(seed)
    ks = sc.coset_representatives(field, m)
    om = sc.domain_elements(field, k)
    ids = np.frombuffer(b"".join((ki * w % r).to_bytes(32, "little") for ki in ks for w in om), dtype=np.uint8).reshape(m * n, 32)
    cells = rng.permutation(m * n)
    lens = rng.integers(1, 7, size=m * n)
    starts = np.concatenate(([0], np.cumsum(lens)))
    starts = starts[starts < m * n]
    cyc = np.zeros(m * n, dtype=np.int64)
    cyc[starts[1:]] = 1
    cyc = np.cumsum(cyc)                                  # the cycle every position of `cells` belongs to
    nxt = np.arange(1, m * n + 1)
    ends = np.concatenate((starts[1:], [m * n])) - 1
    nxt[ends] = starts                                    # the last cell of a cycle points back to its first
    values = rng.integers(0, 256, size=(starts.size, 32), dtype=np.uint8)
    wires = np.empty((m * n, 32), dtype=np.uint8)
    sigmas = np.empty((m * n, 32), dtype=np.uint8)
    wires[cells] = values[cyc]
    sigmas[cells] = ids[cells[nxt]]
    return wires.reshape(m, n, 32), sigmas.reshape(m, n, 32), ks, om, cells, nxt


def test_permutation_product_at_2_20(domains, torch_):
    """m = 3 at 2^20 rows of BLS12-381: out[0] = 1, total = 1, 4096 sampled rows hold z[j+1] den[j] == z[j] num[j] in Python integers,
    and one changed wire gives total != 1"""
    torch = torch_
    field, k, m = "bls12_381", 20, 3
    r = nc.modulus(field)
    n = 1 << k
    dom = domains(field, k)
    wires, sigmas, ks, om, cells, nxt = big_permutation(field, k, m, 0x20F)
    rng = random.Random(0x210)
    beta, gamma = rng.randrange(1, r), rng.randrange(1, r)
    w_d, s_d = torch.from_numpy(wires).cuda(), torch.from_numpy(sigmas).cuda()
    z, total = dom.permutation_product(w_d, s_d, beta, gamma, ks, montgomery=False)
    zh = z.cpu().numpy()
    val = lambda a: int.from_bytes(a.tobytes(), "little")
    assert val(zh[0]) == 1 and total == 1
    rows = [0, 1, 1022, 1023, 1024, n - 2] + [rng.randrange(n - 1) for _ in range(4090)]
    for j in rows:
        num = den = 1
        for i in range(m):
            wv = val(wires[i, j])
            num = num * (wv + beta * ks[i] * om[j] + gamma) % r
            den = den * (wv + beta * val(sigmas[i, j]) + gamma) % r
        assert val(zh[j + 1]) * den % r == val(zh[j]) * num % r, j
    # the broken instance: a wire value changed in a cell that sigma does not map to itself
    at = next(int(cells[t]) for t in range(m * n) if nxt[t] != t)
    w_d.reshape(-1, 32)[at, 0] ^= 1
    zb, total_b = dom.permutation_product(w_d, s_d, beta, gamma, ks, montgomery=False)
    assert total_b != 1 and val(zb[0].cpu().numpy()) == 1


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_round_two_feeds_the_msm(ea, oracle, domains, torch_):
    """2^12 rows of BLS12-381: z = permutation_product(wires, sigmas), its coefficients by ifft, their commitment by ctx.run under
    scalars_montgomery -- three calls on device memory with nothing downloaded in between -- equal to the CPU oracle's MSM of the
    model's coefficients; scan_work_bytes is reported and the other work memory is what it was"""
    torch = torch_
    field, k, m = "bls12_381", 12, 3
    n = 1 << k
    curve = CURVE_OF[field]
    cid = ea.CURVE_IDS[curve]
    dom = domains(field, k)
    p = sc.permutation(field, k, m, 0xE2E)
    z, total = p.model()
    coeffs = nc.transform(field, k, nc.INVERSE, z)
    bases = ea.generate_points(n, distinct=n, seed=0xBA5F, curve=curve)
    scal = np.frombuffer(nc.encode(field, coeffs, True), dtype=np.uint8).reshape(n, 32)
    exp = ctypes.create_string_buffer(ea.projective_bytes(curve))
    assert oracle.oracle_msm(cid, bases.ctypes.data, ea.affine_stride(curve), scal.ctypes.data, n, exp, 0) == 0
    w, s = perm_inputs(torch, p, True)
    dom.ifft(w[0])                                         # (the transform's work memory exists before the new calls)
    before = (dom.query("work_bytes"), dom.query("poly_work_bytes"))
    ctx = ea.multi_scalar_mult_init(torch.from_numpy(bases).cuda(), curve)
    try:
        ctx.set_option("scalars_montgomery", 1)
        z_d, got_total = dom.permutation_product(w, s, p.beta, p.gamma, p.ks)
        commit = ctx.run(dom.ifft(z_d))
        assert z_d.is_cuda and got_total == 1 and commit[0] == exp.raw
    finally:
        ctx.close()
    dom.prefix_sum(z_d)
    dom.prefix_product(raw_of(z_d))
    assert dom.query("scan_work_bytes") >= 2 * n * 32
    assert (dom.query("work_bytes"), dom.query("poly_work_bytes")) == before


# ---- speed ---------------------------------------------------------------------------------------------------------------------------

# Modelled without a run, from the product count, against the forward transform of 2^22 elements of BLS12-381 Fr that
# tests/test_gpu_ntt.py models at 17 products per element:
#   product scan   the way up: conversion 1 + run 3/4 + tree 3/4 (12 wave-products a block of 1024) = 2.5; the way down: conversion 1 +
#                  prefixes 3/4 + scan 8/4 + offset and outputs 1 + conversion 1 = 5.75: 8.25 products, the count of divide_by_linear,
#                  which tests/test_gpu_poly.py models at 0.5 and profiles/poly.txt measured at 0.48.
# The sum scan and permutation_product are recorded in profiles/scan.txt by tools/scan_bench.py and not guarded.
MODEL_RATIO = 0.5


def speed_bound():
    """(bound on the product scan / forward transform, source): 1.5 x the ratio profiles/scan.txt recorded, or 2 x the modelled ratio"""
    path = os.path.join(ROOT, "profiles", "scan.txt")
    if os.path.exists(path):
        m = re.search(r"^bls12_381 ratio prefix_product 2\^22 / forward NN 2\^22: ([0-9.]+)", open(path).read(), flags=re.M)
        if m:
            return 1.5 * float(m.group(1)), "profiles/scan.txt"
    return 2 * MODEL_RATIO, "the model"


def test_speed_guard_against_the_transform(domains, torch_):
    """BLS12-381, 2^22 device-resident elements, warmed up, median of 5: the product scan against the forward NN transform of the same
    length, which this change does not touch, run in the same test on the same box.  Bound: 1.5 x the ratio profiles/scan.txt
    recorded (tools/scan_bench.py; the margin covers box-to-box spread and clock differences under the power limit), or
    2 x the modelled ratio above without that file."""
    torch = torch_
    n = 1 << 22
    dom = domains("bls12_381", 22)
    rng = np.random.default_rng(0x5EED)
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x3F
    x = torch.from_numpy(raw).cuda()
    out = torch.empty_like(x)

    def median5(fn):
        fn()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    t_ntt = median5(lambda: dom.fft(x, out=out))
    t = median5(lambda: dom.prefix_product(x, out=out))
    bound, source = speed_bound()
    print("2^22: prefix_product %.3f ms, forward NN %.3f ms, ratio %.4f, bound %.4f from %s" % (1e3 * t, 1e3 * t_ntt, t / t_ntt, bound, source))
    assert t / t_ntt <= bound
