"""GPU: the calls between a transform and an MSM on the domain handle (csrc/poly.hpp, csrc/msm_poly.hpp) through the Python layer,
byte for byte against Python big integers (pow(x, -1, r), Horner, synthetic division: tests/poly_cases.py), and the two computations
they exist for -- the Groth16 / Marlin quotient and a KZG opening -- end to end in device memory."""
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


def ints(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


# ---- the host build's case list ------------------------------------------------------------------------------------------------------

def case_list(field, tile_log):
    if tile_log == 4:
        out = [(n, pc.vector(field, n, 4, 0xA0 + n)) for n in pc.lengths(4)]
    else:
        out = [(n, pc.vector(field, n, 10, 0xB0 + n)) for n in (0, 1, 2, 1023, 1024, 1025, 3 * 1024 + 5)]
    mult = pc.multiples_of_r(field)
    out.append(((1 << tile_log) + 5, [mult[i % len(mult)] for i in range((1 << tile_log) + 5)]))
    return out


@pytest.mark.parametrize("tile_log", [4, 0])
@pytest.mark.parametrize("field", FIELDS)
def test_case_list_host_and_device_pointers(domains, torch_, field, tile_log):
    """every length and every planted zero of tests/test_poly_host.py, from host memory and from GPU tensors: identical bytes, equal
    to Python's"""
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 6)
    dom.set_option("poly_tile_log", tile_log)
    assert dom.query("poly_tile_log") == (tile_log or 10)
    for n, pattern in case_list(field, tile_log or 10):
        raw = pc.to_raw(pattern)
        d_raw = dev(torch, raw)
        for montgomery in (True, False):
            vals = pc.values(field, pattern, not montgomery)
            for coeff in (None, 0x1234567):
                want = nc.encode(field, pc.ref_inverse(vals, 1 if coeff is None else coeff, r), not montgomery)
                assert dom.batch_inversion_and_mul(raw, coeff, montgomery=montgomery) == want, (n, coeff)
                got = dom.batch_inversion_and_mul(d_raw, coeff, montgomery=montgomery)
                assert got.is_cuda and raw_of(got) == want, (n, coeff)
            for z in pc.scalars(field, n):
                want_q, want_rem = pc.ref_divide(vals, z, r)
                assert dom.evaluate(raw, z, montgomery=montgomery) == want_rem, (n, z)
                assert dom.evaluate(d_raw, z, montgomery=montgomery) == want_rem, (n, z)
                for src in (raw, d_raw):
                    q, rem = dom.divide_by_linear(src, z, montgomery=montgomery)
                    assert rem == want_rem and raw_of(q) == nc.encode(field, want_q, not montgomery), (n, z)
    dom.set_option("poly_tile_log", 0)


@pytest.mark.parametrize("field", FIELDS)
def test_vec_ops_and_in_place(domains, torch_, field):
    """a + b, a - b, a*b - c, s*a and the division on the coset on inputs above the modulus; out aliasing each input exactly; the
    inversion in place"""
    torch = torch_
    r, g = nc.modulus(field), nc.generator(field)
    dom = domains(field, 6)
    n = 1024 + 77
    pa, pb, pc_ = (pc.vector(field, n, 10, s, zeros=(s == 1)) for s in (1, 2, 3))
    for montgomery in (True, False):
        va, vb, vc = (pc.values(field, p, not montgomery) for p in (pa, pb, pc_))
        enc = lambda v: nc.encode(field, v, not montgomery)
        want = {"add": enc([x + y for x, y in zip(va, vb)]), "sub": enc([x - y for x, y in zip(va, vb)]),
                "mul_sub": enc([x * y - z for x, y, z in zip(va, vb, vc)]), "scale": enc([(r - 3) * x for x in va]),
                "coset": enc([x * pow(pow(g, 64, r) - 1, -1, r) for x in va]), "coset5": enc([x * pow(pow(5, 64, r) - 1, -1, r) for x in va]),
                "inv": enc(pc.ref_inverse(va, 7, r))}
        fresh = lambda: [dev(torch, pc.to_raw(p)) for p in (pa, pb, pc_)]
        a, b, c = fresh()
        assert raw_of(dom.add(a, b, montgomery=montgomery)) == want["add"]
        assert dom.add(pc.to_raw(pa), pc.to_raw(pb), montgomery=montgomery) == want["add"]
        assert raw_of(dom.sub(a, b, montgomery=montgomery)) == want["sub"]
        assert dom.sub(pc.to_raw(pa), pc.to_raw(pb), montgomery=montgomery) == want["sub"]
        assert raw_of(dom.mul_sub(a, b, c, montgomery=montgomery)) == want["mul_sub"]
        assert dom.mul_sub(pc.to_raw(pa), pc.to_raw(pb), pc.to_raw(pc_), montgomery=montgomery) == want["mul_sub"]
        assert raw_of(dom.scale(a, r - 3, montgomery=montgomery)) == want["scale"]
        assert dom.scale(pc.to_raw(pa), r - 3, montgomery=montgomery) == want["scale"]
        assert raw_of(dom.divide_by_vanishing_poly_on_coset(a, montgomery=montgomery)) == want["coset"]
        assert dom.divide_by_vanishing_poly_on_coset(pc.to_raw(pa), offset=5, montgomery=montgomery) == want["coset5"]
        assert raw_of(a) == pc.to_raw(pa)                                     # nothing above wrote to an input
        for name, which in (("add", 0), ("add", 1), ("sub", 0), ("sub", 1), ("mul_sub", 0), ("mul_sub", 1), ("mul_sub", 2)):
            t = fresh()
            args = t[:3] if name == "mul_sub" else t[:2]
            res = getattr(dom, name)(*args, montgomery=montgomery, out=t[which])
            assert res is t[which] and raw_of(res) == want[name], (name, which)
        a, b, c = fresh()
        assert raw_of(dom.scale(a, r - 3, montgomery=montgomery, out=a)) == want["scale"]
        a, b, c = fresh()
        assert raw_of(dom.divide_by_vanishing_poly_on_coset(a, montgomery=montgomery, out=a)) == want["coset"]
        a, b, c = fresh()
        assert raw_of(dom.batch_inversion_and_mul(a, 7, montgomery=montgomery, out=a)) == want["inv"]
        assert raw_of(dom.add(a, a, montgomery=montgomery, out=a)) == enc([2 * x for x in ints_mod(want["inv"], field, not montgomery)])


def ints_mod(raw, field, normal):
    return nc.decode(field, raw, normal)


def test_refusals_with_a_handle(ea, domains, torch_):
    """what needs a domain to be judged: an offset inside it; and the refusals reach Python as MsmError(-1)"""
    torch = torch_
    for field in FIELDS:
        r = nc.modulus(field)
        dom = domains(field, 6)
        w = dom.group_gen
        x = dev(torch, nc.encode(field, list(range(1, 9)), False))
        for bad in (1, w, pow(w, 63, r), 0):
            for src in (x, raw_of(x)):
                with pytest.raises(ea.MsmError) as e:
                    dom.divide_by_vanishing_poly_on_coset(src, offset=bad, montgomery=False)
                assert e.value.code == -1 and ("lies in the domain" in str(e.value) or "offset is zero" in str(e.value))
        with pytest.raises(ea.MsmError, match="overlap"):
            buf = torch.zeros((16, 32), dtype=torch.uint8, device="cuda")
            dom.batch_inversion(buf[1:9], out=buf[0:8])
        with pytest.raises(ea.MsmError, match="overlaps the coefficients"):
            dom.divide_by_linear(buf[0:8], 3, out=buf[1:8])
        assert dom.evaluate_vanishing_polynomial(w) == 0 and dom.evaluate_vanishing_polynomial(3) == (pow(3, 64, r) - 1) % r


def test_work_memory_is_reported_apart(domains, torch_):
    torch = torch_
    with __import__("entries_amd").Radix2EvaluationDomain(1 << 6, "bls12_381_g1") as dom:
        assert dom.query("poly_work_bytes") == 0 and dom.query("work_bytes") == 0
        x = dev(torch, nc.encode("bls12_381", list(range(1, 5000)), False))
        dom.batch_inversion(x)
        first = dom.query("poly_work_bytes")
        assert 0 < first <= 36 * (2 * 5 + 8) + 4096 and dom.query("work_bytes") == 0
        dom.evaluate(x, 3)
        dom.divide_by_linear(x, 3)
        assert dom.query("poly_work_bytes") == first                        # kept by the handle, not allocated again


# ---- at size ---------------------------------------------------------------------------------------------------------------------------

_AT_SIZE = {}


def at_size(field, n, montgomery):
    """(raw bytes as a NumPy array, the integers they stand for): random 256-bit patterns, computed once"""
    key = (field, n, montgomery)
    if key not in _AT_SIZE:
        rng = np.random.default_rng(n + len(field) + (1 if montgomery else 0) + (0 if field == "bls12_377" else 99))
        raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        r = nc.modulus(field)
        f = pow(nc.MONT, -1, r) if montgomery else 1
        _AT_SIZE[key] = (raw, [x * f % r for x in ints(raw.tobytes())])
    return _AT_SIZE[key]


AT_SIZE = [((1 << 20) + 1025, False), ((1 << 20) - 1, True)]     # three levels, ragged at each; one element short of full tiles


@pytest.mark.parametrize("n,montgomery", AT_SIZE)
@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_and_divide_at_size(domains, torch_, field, n, montgomery):
    """default tile: every quotient coefficient and the remainder against Python's synthetic division"""
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 6)
    raw, vals = at_size(field, n, montgomery)
    x = torch.from_numpy(raw).cuda()
    z = random.Random(n).randrange(r)
    want_q, want_rem = pc.ref_divide(vals, z, r)
    assert dom.evaluate(x, z, montgomery=montgomery) == want_rem
    q, rem = dom.divide_by_linear(x, z, montgomery=montgomery)
    assert rem == want_rem
    assert q.shape == (n - 1, 32) and raw_of(q) == nc.encode(field, want_q, not montgomery)
    assert dom.query("poly_work_bytes") >= 36 * 2 * (1025 + 2)


@pytest.mark.parametrize("n,montgomery", AT_SIZE)
@pytest.mark.parametrize("field", FIELDS)
def test_batch_inverse_at_size(domains, torch_, field, n, montgomery):
    """default tile, zeros planted at the first and last position of lane runs and of tiles, over a lane run and over a whole tile
    (1054 of them): pow() on the first, the last and 4096 random positions; every other position by in * out == coeff, out < r,
    zeros staying zero"""
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 6)
    raw, vals = at_size(field, n, montgomery)
    raw, vals = raw.copy(), list(vals)
    mult = pc.multiples_of_r(field)
    spots = [0, 3, 4, 7, 1023, 1024, 2047, n - 1, n - 4, 5 * 1024 + 511, (1 << 20) - 1, 1 << 19] + list(range(40, 44)) + list(range(9 * 1024, 10 * 1024)) \
        + [1024 * t + 17 * t % 1024 for t in range(20, 34)]
    for j, pos in enumerate(p for p in spots if 0 <= p < n):
        raw[pos] = np.frombuffer(mult[j % len(mult)].to_bytes(32, "little"), dtype=np.uint8)
        vals[pos] = 0
    assert sum(1 for v in vals if v == 0) >= 1000
    coeff = 0xC0FFEE
    f = nc.MONT if montgomery else 1
    got = ints(raw_of(dom.batch_inversion_and_mul(torch.from_numpy(raw).cuda(), coeff, montgomery=montgomery)))
    assert len(got) == n and max(got) < r
    rng = random.Random(n)
    for i in [0, n - 1, 1, n - 2] + [rng.randrange(n) for _ in range(4096)]:
        assert got[i] == (coeff * pow(vals[i], -1, r) * f % r if vals[i] else 0), i
    minv = pow(f, -1, r)
    bad = [i for i in range(n) if (got[i] != 0 if vals[i] == 0 else vals[i] * got[i] * minv % r != coeff)]
    assert not bad, bad[:8]


# ---- Lagrange coefficients ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_lagrange_small(domains, torch_, field):
    r = nc.modulus(field)
    dom = domains(field, 10)
    w = nc.root_of_unity(field, 10)
    assert dom.group_gen == w
    for tau in (0, 1, r - 1, pow(w, 5, r), pow(w, 1023, r), 0xDEADBEEF):
        want = pc.ref_lagrange(field, 10, tau)
        for montgomery in (True, False):
            assert raw_of(dom.evaluate_all_lagrange_coefficients(tau, montgomery=montgomery)) == nc.encode(field, want, not montgomery), tau
            got = dom.evaluate_all_lagrange_coefficients(tau, montgomery=montgomery, device=True)
            assert got.is_cuda and raw_of(got) == nc.encode(field, want, not montgomery), tau
    for tile_log in (4, 7):
        dom.set_option("poly_tile_log", tile_log)
        assert raw_of(dom.evaluate_all_lagrange_coefficients(0xDEADBEEF)) == nc.encode(field, want, False)
    dom.set_option("poly_tile_log", 0)


@pytest.mark.parametrize("field", FIELDS)
def test_lagrange_at_2_20(domains, torch_, field):
    """sum L_i = 1; sum L_i w^i = tau; 64 entries against the closed form; sum L_i(tau) f(w^i) = f(tau) with f(w^i) from the
    existing fft and f(tau) from the new evaluate (and from Python)"""
    torch = torch_
    k, n = 20, 1 << 20
    r = nc.modulus(field)
    dom = domains(field, k)
    w = nc.root_of_unity(field, k)
    tau = random.Random(0x7A0).randrange(r)
    L_dev = dom.evaluate_all_lagrange_coefficients(tau, montgomery=False, device=True)
    L = ints(raw_of(L_dev))
    assert max(L) < r and sum(L) % r == 1
    acc, x = 0, 1
    for v in L:
        acc += v * x
        x = x * w % r
    assert acc % r == tau
    c = (pow(tau, n, r) - 1) * pow(n, -1, r) % r
    rng = random.Random(0x7A1)
    for i in [0, 1, n - 1, n // 2] + [rng.randrange(n) for _ in range(60)]:
        wi = pow(w, i, r)
        assert L[i] == c * wi * pow(tau - wi, -1, r) % r, i
    f_raw, f = at_size(field, n, False)
    f_dev = torch.from_numpy(f_raw).cuda()
    evals = dom.fft(f_dev, montgomery=False)
    f_tau = dom.evaluate(f_dev, tau, montgomery=False)
    assert f_tau == pc.ref_evaluate(f, tau, r)
    assert sum(ints(raw_of(dom.mul(L_dev, evals, montgomery=False)))) % r == f_tau


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

def poly_long_division_by_vanishing(num, n, r):
    """schoolbook: the quotient of num by X^n - 1 (exact division expected)"""
    num = list(num)
    q = [0] * (len(num) - n)
    for i in range(len(num) - 1, n - 1, -1):
        q[i - n] = num[i]
        num[i - n] = (num[i - n] + num[i]) % r
        num[i] = 0
    assert not any(num)
    return q


@pytest.mark.parametrize("k", [12, 8])
@pytest.mark.parametrize("field", FIELDS)
def test_quotient_polynomial_on_the_device(domains, torch_, field, k):
    """h = coset_ifft((coset_fft(a) coset_fft(b) - coset_fft(c)) / Z(g)) with c = a * b on the domain: h(x) (x^n - 1) = a(x) b(x) - c(x)
    at three random x (k = 12), and h equal to Python's long division coefficient for coefficient (k = 8)"""
    torch = torch_
    n = 1 << k
    r = nc.modulus(field)
    dom = domains(field, k)
    a_ev, b_ev = nc.random_values(field, n, 0xE2E + k), nc.random_values(field, n, 0xE2F + k)
    a_d, b_d = dev(torch, nc.encode(field, a_ev, False)), dev(torch, nc.encode(field, b_ev, False))
    c_d = dom.mul(a_d, b_d)
    a_c, b_c, c_c = dom.ifft(a_d), dom.ifft(b_d), dom.ifft(c_d)
    num = dom.mul_sub(dom.coset_fft(a_c), dom.coset_fft(b_c), dom.coset_fft(c_c))
    h = dom.coset_ifft(dom.divide_by_vanishing_poly_on_coset(num, out=num))
    assert h.is_cuda
    a, b, c, hh = (nc.decode(field, raw_of(t), False) for t in (a_c, b_c, c_c, h))
    assert a == nc.transform(field, k, nc.INVERSE, a_ev) and c == nc.transform(field, k, nc.INVERSE, [x * y % r for x, y in zip(a_ev, b_ev)])
    rng = random.Random(k)
    for _ in range(3):
        x = rng.randrange(r)
        ev = lambda p: pc.ref_evaluate(p, x, r)
        assert ev(hh) * (pow(x, n, r) - 1) % r == (ev(a) * ev(b) - ev(c)) % r
    if k == 8:
        prod = [0] * (2 * n - 1)
        for i, u in enumerate(a):
            for j, v in enumerate(b):
                prod[i + j] = (prod[i + j] + u * v) % r
        for i, v in enumerate(c):
            prod[i] = (prod[i] - v) % r
        want = poly_long_division_by_vanishing(prod, n, r)
        assert hh == want + [0] * (n - len(want))


@pytest.mark.parametrize("field", FIELDS)
def test_kzg_opening_feeds_the_msm(ea, oracle, domains, torch_, field):
    """p(z) and (p - p(z)) / (X - z) at 2^12 coefficients; the quotient, still in device memory, goes into ctx.run under
    scalars_montgomery and equals the CPU oracle's MSM of Python's quotient"""
    torch = torch_
    n = 4096
    r = nc.modulus(field)
    curve = CURVE_OF[field]
    cid = ea.CURVE_IDS[curve]
    dom = domains(field, 12)
    p = nc.random_values(field, n, 0x4B5A)
    z = random.Random(0x4B5B).randrange(r)
    want_q, want_rem = pc.ref_divide(p, z, r)
    bases = ea.generate_points(n, distinct=n, seed=0xBA5E, curve=curve)
    scal = np.frombuffer(nc.encode(field, want_q + [0], True), dtype=np.uint8).reshape(n, 32)
    exp = ctypes.create_string_buffer(ea.projective_bytes(curve))
    assert oracle.oracle_msm(cid, bases.ctypes.data, ea.affine_stride(curve), scal.ctypes.data, n, exp, 0) == 0
    p_d = dev(torch, nc.encode(field, p, False))
    assert dom.evaluate(p_d, z) == want_rem
    qbuf = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    q, rem = dom.divide_by_linear(p_d, z, out=qbuf[:n - 1])
    assert rem == want_rem and q.is_cuda and q.data_ptr() == qbuf.data_ptr()
    ctx = ea.multi_scalar_mult_init(torch.from_numpy(bases).cuda(), curve)
    try:
        ctx.set_option("scalars_montgomery", 1)
        assert ctx.run(qbuf)[0] == exp.raw
    finally:
        ctx.close()


# ---- speed ------------------------------------------------------------------------------------------------------------------------------

# Modelled without a run, from product counts and bytes, against the forward transform of 2^22 elements of BLS12-381 Fr
# that tests/test_gpu_ntt.py models at 2601 multiply-adds per element (17 products of 153):
#   batch_inverse      launch 1: conversion 1 + run 3/4 + tree 3/4 (12 wave-products a block of 1024) = 2.5; launch 2: 380 / 1024 = 0.4;
#                      launch 3: conversion 1 + run and outputs 13/4 + two scans 2 x 8 / 4 + conversion 1 = 9.25: 12.15 products, ratio 0.71.
#                      96 bytes an element, 0.1 ms at 4 TB/s: under the arithmetic (0.43 ms).
#   evaluate           conversion 1 + Horner 3/4 + tree 3/4 = 2.5 products, ratio 0.15; two launches, one download of 36 bytes and the
#                      host's 80 squarings add what 0.05 of the transform takes: 0.2.
#   divide_by_linear   the way up 2.5; the way down: conversion 1 + Horner 3/4 + scan 8/4 + finish 1 + conversion 1 = 5.75: 8.25 products,
#                      ratio 0.49; 0.5.
MODEL_RATIO = {"batch_inverse": 0.75, "evaluate": 0.2, "divide_by_linear": 0.5}


def speed_bound(call):
    """(bound on call / forward transform, source): 1.5 x the ratio profiles/poly.txt recorded, or 2 x the modelled ratio"""
    path = os.path.join(ROOT, "profiles", "poly.txt")
    if os.path.exists(path):
        m = re.search(r"^bls12_381 ratio %s 2\^22 / forward NN 2\^22: ([0-9.]+)" % call, open(path).read(), flags=re.M)
        if m:
            return 1.5 * float(m.group(1)), "profiles/poly.txt"
    return 2 * MODEL_RATIO[call], "the model"


def test_speed_guard_against_the_transform(domains, torch_):
    """BLS12-381, 2^22 device-resident elements, warmed up, median of 5: batch_inverse, evaluate and divide_by_linear each against
    the forward NN transform of the same length, which this change does not touch, run in the same test on the same box.  Bound:
    1.5 x the ratio profiles/poly.txt recorded (tools/poly_bench.py; the margin covers box-to-box spread and clock differences under
    the power limit), or 2 x the modelled ratio above without that file."""
    torch = torch_
    n = 1 << 22
    dom = domains("bls12_381", 22)
    rng = np.random.default_rng(0x5EED)
    raw = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 31] &= 0x3F
    x = torch.from_numpy(raw).cuda()
    out = torch.empty_like(x)
    q = torch.empty((n - 1, 32), dtype=torch.uint8, device="cuda")

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
    times = {"batch_inverse": median5(lambda: dom.batch_inversion(x, out=out)), "evaluate": median5(lambda: dom.evaluate(x, 0x1234567)),
             "divide_by_linear": median5(lambda: dom.divide_by_linear(x, 0x1234567, out=q))}
    verdicts = []
    for call, t in times.items():
        bound, source = speed_bound(call)
        print("2^22: %s %.3f ms, forward NN %.3f ms, ratio %.4f, bound %.4f from %s" % (call, 1e3 * t, 1e3 * t_ntt, t / t_ntt, bound, source))
        verdicts.append((call, t / t_ntt, bound))
    for call, ratio, bound in verdicts:
        assert ratio <= bound, call
