"""GPU: the rows of the Plonk quotient and the linear combination on the domain handle (csrc/quotient.hpp, csrc/msm_quot.hpp) through the
Python layer, byte for byte against Python big integers (tests/quotient_cases.py), and the computations they exist for -- a TurboPlonk
prover's third round, wires -> z -> 25 coset_ffts -> rows -> coset_ifft, and the opening polynomial of its fourth and fifth -- end to
end in device memory."""
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
import quotient_cases as qc
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


def report_mismatches(got_raw, want_raw, what):
    got = np.frombuffer(got_raw, dtype=np.uint8).reshape(-1, 32)
    want = np.frombuffer(want_raw, dtype=np.uint8).reshape(-1, 32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        pytest.fail("%s: %d of %d rows differ; first at %s" % (what, bad.size, got.shape[0], bad[:8].tolist()))


# ---- rows against the model --------------------------------------------------------------------------------------------------------

def host_columns(c, which, stride):
    return np.frombuffer(c.columns(which, stride) + b"\xee" * (32 * (stride - c.M)), dtype=np.uint8).reshape(len(which), stride, 32).copy()


@pytest.mark.parametrize("montgomery", [True, False])
@pytest.mark.parametrize("field", FIELDS)
def test_case_list_three_ways(domains, torch_, field, montgomery):
    """every case of tests/test_quotient_host.py from host memory, from GPU tensors with out=, and with the columns M + 3 elements
    apart against lists of separate vectors: identical bytes, equal to the model's, under both inversion tiles"""
    torch = torch_
    normal = not montgomery
    for name, c, tile_logs in qc.row_cases(field):
        dom = domains(field, c.K)
        want = nc.encode(field, c.model(normal), normal)
        z = np.frombuffer(pc.to_raw(c.raw_z(normal)), dtype=np.uint8).reshape(c.M, 32)
        pi = None if c.pi is None else np.frombuffer(pc.to_raw(c.pi), dtype=np.uint8).reshape(c.M, 32)
        kw = dict(montgomery=montgomery, offset=c.offset)
        scal = (c.alpha, c.beta, c.gamma, c.ks, c.n)
        for tile_log in tile_logs:
            dom.set_option("poly_tile_log", 0 if tile_log == 10 else tile_log)
            w, s = host_columns(c, c.wires, c.M), host_columns(c, c.sigmas, c.M)
            q = None if c.selectors is None else host_columns(c, c.selectors, c.M)
            got = dom.plonk_quotient(w, s, z, *scal, selectors=q, pi=pi, **kw)
            assert isinstance(got, np.ndarray)
            report_mismatches(got.tobytes(), want, (name, tile_log, "host memory"))
            g = lambda a: None if a is None else torch.from_numpy(a.copy()).cuda()
            out = torch.full((c.M, 32), 0x55, dtype=torch.uint8, device="cuda")
            res = dom.plonk_quotient(g(w), g(s), g(z), *scal, selectors=g(q), pi=g(pi), out=out, **kw)
            assert res.is_cuda and res.data_ptr() == out.data_ptr()
            report_mismatches(raw_of(res), want, (name, tile_log, "GPU tensors, out="))
            stride = c.M + 3
            ws, ss = g(host_columns(c, c.wires, stride)), g(host_columns(c, c.sigmas, stride))
            qs = None if c.selectors is None else g(host_columns(c, c.selectors, stride))
            res = dom.plonk_quotient(ws, ss, g(z), *scal, selectors=qs, pi=g(pi), **kw)
            report_mismatches(raw_of(res), want, (name, tile_log, "stride M + 3"))
            lists = [[g(col) for col in cols] for cols in (w, s)]
            ql = None if q is None else [g(col) for col in q]
            res = dom.plonk_quotient(lists[0], lists[1], g(z), *scal, selectors=ql, pi=g(pi), **kw)
            report_mismatches(raw_of(res), want, (name, tile_log, "lists of vectors"))
        dom.set_option("poly_tile_log", 0)


@pytest.mark.parametrize("field", FIELDS)
def test_rows_with_an_upper_table_entry(domains, torch_, field):
    """K = 15, n = 2^12: the first size whose rows read a non-zero entry of the upper twiddle table (NTT_LO_LOG = 14).  Random 256-bit
    patterns as arkworks images, every row against the model"""
    torch = torch_
    K, n, M = 15, 1 << 12, 1 << 15
    r = nc.modulus(field)
    dom = domains(field, K)
    rng = np.random.default_rng(0x15 + len(field))
    raw = rng.integers(0, 256, size=(25, M, 32), dtype=np.uint8)
    inv = pow(nc.MONT, -1, r)

    def vals_of(v):
        b = v.tobytes()
        return [int.from_bytes(b[32 * i:32 * i + 32], "little") * inv % r for i in range(M)]

    vals = [vals_of(v) for v in raw]
    prng = random.Random(0xF15)
    alpha, beta, gamma = (prng.randrange(1, r) for _ in range(3))
    ks = qc.sc.coset_representatives(field, 5)
    want = qc.ref_quotient_rows(field, K, n, vals[0:5], vals[5:10], vals[10:23], vals[23], vals[24], ks, alpha, beta, gamma)
    t = torch.from_numpy(raw).cuda()
    got = dom.plonk_quotient(t[0:5], t[5:10], t[23], alpha, beta, gamma, ks, n, selectors=t[10:23], pi=t[24])
    report_mismatches(raw_of(got), nc.encode(field, want, False), "K = 15")
    assert dom.query("quotient_work_bytes") >= M * 32


# ---- the linear combination --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("montgomery", [True, False])
@pytest.mark.parametrize("field", FIELDS)
def test_linear_combination_case_list(domains, torch_, field, montgomery):
    """the host build's cases from host memory and from GPU tensors, and with out= the first column (the longest moved there)"""
    torch = torch_
    r = nc.modulus(field)
    dom = domains(field, 4)
    for cols, coeffs in qc.lincomb_cases(field):
        want = nc.encode(field, qc.ref_lincomb([pc.values(field, c, not montgomery) for c in cols], coeffs, r), not montgomery)
        n = len(want) // 32
        raws = [pc.to_raw(c) for c in cols]
        got = dom.linear_combination(raws, coeffs, montgomery=montgomery)
        assert raw_of(got) == want, ([len(c) for c in cols], "host memory")
        tens = [dev(torch, x) for x in raws]
        got = dom.linear_combination(tens, coeffs, montgomery=montgomery)
        assert got.is_cuda and raw_of(got) == want, ([len(c) for c in cols], "GPU tensors")
        assert [raw_of(t) for t in tens] == raws                    # the inputs are left alone
        if n:
            first = max(range(len(cols)), key=lambda j: len(cols[j]))
            order = [first] + [j for j in range(len(cols)) if j != first]
            tens = [tens[j] for j in order]
            got = dom.linear_combination(tens, [coeffs[j] for j in order], montgomery=montgomery, out=tens[0])
            assert got.data_ptr() == tens[0].data_ptr() and raw_of(tens[0]) == want, ([len(c) for c in cols], "out = column 0")


def test_linear_combination_at_size_against_scale_and_add(domains, torch_):
    """2^20 + 3 elements, 15 vectors of BLS12-381 (four of them shorter): one call against 15 scale and 14 add calls, compared on the GPU"""
    torch = torch_
    field, n, m = "bls12_381", (1 << 20) + 3, 15
    r = nc.modulus(field)
    dom = domains(field, 4)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x11C0)
    lens = [n - (0, 1, 255, 1 << 19)[j % 4] if j % 4 and j < 8 else n for j in range(m)]
    cols = [torch.randint(0, 256, (ln, 32), dtype=torch.uint8, device="cuda", generator=g) for ln in lens]
    prng = random.Random(0x11C1)
    coeffs = [prng.randrange(r) for _ in range(m)]
    got = dom.linear_combination(cols, coeffs)
    acc = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    dom.scale(cols[0], coeffs[0], out=acc)
    for j in range(1, m):
        tmp = dom.scale(cols[j], coeffs[j])
        dom.add(acc[:lens[j]], tmp, out=acc[:lens[j]])
    assert got.shape == acc.shape and torch.equal(got, acc)


# ---- round 3 end to end ------------------------------------------------------------------------------------------------------------

class Round3:
    """the third round of the reference's prover for a circuit of qc.Circuit: every vector stays in device memory between the calls;
    the coefficient vectors are downloaded for the checks alone"""

    def __init__(self, torch, dom_n, dom_M, c, seed):
        field, n = c.field, c.n
        r = nc.modulus(field)
        rng = random.Random(seed)
        enc = lambda vals: dev(torch, nc.encode(field, vals, False))
        dec = lambda t: nc.decode(field, raw_of(t), False)
        self.alpha, self.beta, self.gamma = (rng.randrange(1, r) for _ in range(3))
        W, S = torch.stack([enc(col) for col in c.wires]), torch.stack([enc(col) for col in c.sigmas])
        # 1, 2: the wires' coefficients, blinded as the reference does ((b0 + b1 X) Z_H)
        self.wires = [qc.blind(dec(dom_n.ifft(W[j])), n, [rng.randrange(r), rng.randrange(r)], r) for j in range(5)]
        # 3: z on H_n from the (unblinded) values, then its coefficients with three blinders
        z, self.total = dom_n.permutation_product(W, S, self.beta, self.gamma, c.ks)
        self.z = qc.blind(dec(dom_n.ifft(z)), n, [rng.randrange(r) for _ in range(3)], r)
        self.sigmas_d = [dom_n.ifft(S[j]) for j in range(5)]
        self.selectors_d = [dom_n.ifft(enc(col)) for col in c.selectors]
        self.pi_d = dom_n.ifft(enc(c.pi))
        self.sigmas, self.selectors, self.pi = [dec(t) for t in self.sigmas_d], [dec(t) for t in self.selectors_d], dec(self.pi_d)
        # 4: the 25 coset_ffts onto the quotient domain (a shorter input is zero-extended: in_len)
        cf = dom_M.coset_fft
        self.evals = dict(wires=[cf(enc(p)) for p in self.wires], sigmas=[cf(t) for t in self.sigmas_d], selectors=[cf(t) for t in self.selectors_d],
                          z=cf(enc(self.z)), pi=cf(self.pi_d))
        self.c, self.dom_M = c, dom_M

    def quotient(self):
        """5, 6: the rows, then coset_ifft: (the coefficients as integers, the rows' bytes)"""
        e = self.evals
        rows = self.dom_M.plonk_quotient(e["wires"], e["sigmas"], e["z"], self.alpha, self.beta, self.gamma, self.c.ks, self.c.n,
                                         selectors=e["selectors"], pi=e["pi"])
        assert rows.is_cuda
        return nc.decode(self.c.field, raw_of(self.dom_M.coset_ifft(rows)), False), raw_of(rows)


@pytest.mark.parametrize("field", FIELDS)
def test_round_three_end_to_end(domains, torch_, field):
    torch = torch_
    k, K = 6, 9
    n, r = 1 << k, nc.modulus(field)
    dom_n, dom_M = domains(field, k), domains(field, K)
    c = qc.Circuit(field, k, 0x3A + len(field))
    rd = Round3(torch, dom_n, dom_M, c, 0x3B)
    assert rd.total == 1
    t, rows = rd.quotient()
    # (a) the degree split_quotient_polynomial demands
    top = 5 * (n + 1) + 2
    assert t[top] != 0 and not any(t[top + 1:])
    # (b) the identity at a random point, in Python integers from the downloaded coefficients
    zeta = random.Random(0x3C).randrange(2, r)
    ev = lambda p, x=zeta: qc.poly_eval(p, x, r)
    zh = (pow(zeta, n, r) - 1) % r
    l1 = zh * pow(n * (zeta - 1) % r, -1, r) % r
    w = [ev(p) for p in rd.wires]
    a, b = ev(rd.z), ev(rd.z, zeta * nc.root_of_unity(field, k) % r)
    for j in range(5):
        a = a * (w[j] + rd.beta * c.ks[j] * zeta + rd.gamma) % r
        b = b * (w[j] + rd.beta * ev(rd.sigmas[j]) + rd.gamma) % r
    rhs = (qc.gate(w, [ev(q) for q in rd.selectors], ev(rd.pi), r) + rd.alpha * (a - b) + rd.alpha * rd.alpha * l1 * (ev(rd.z) - 1)) % r
    assert ev(t) * zh % r == rhs
    # (d) the result does not depend on the inversion's tile
    dom_M.set_option("poly_tile_log", 4)
    t4, rows4 = rd.quotient()
    dom_M.set_option("poly_tile_log", 0)
    assert rows4 == rows and t4 == t
    # (c) one wire value changed: the numerator is no multiple of Z_H and the high coefficients are not all zero
    bad = Round3(torch, dom_n, dom_M, c.broken(), 0x3B)
    tb, _ = bad.quotient()
    assert any(tb[top + 1:])


@pytest.mark.parametrize("field", FIELDS)
def test_rounds_four_and_five_opening(domains, torch_, field):
    """the batched opening polynomial as a linear combination of the wires, the sigmas and z with the powers of a random v, then
    divide_by_linear at zeta: the remainder is the same combination of the evaluate values"""
    torch = torch_
    k = 6
    n, r = 1 << k, nc.modulus(field)
    dom = domains(field, k)
    rng = random.Random(0x45 + len(field))
    polys = [[rng.randrange(r) for _ in range(ln)] for ln in [n + 2] * 5 + [n] * 5 + [n + 3]]
    tens = [dev(torch, nc.encode(field, p, False)) for p in polys]
    v, zeta = rng.randrange(2, r), rng.randrange(2, r)
    powers = [pow(v, j, r) for j in range(len(polys))]
    f = dom.linear_combination(tens, powers)
    assert f.is_cuda and raw_of(f) == nc.encode(field, qc.ref_lincomb(polys, powers, r), False)
    q, rem = dom.divide_by_linear(f, zeta)
    assert q.shape[0] == n + 2 and rem == sum(c * dom.evaluate(t, zeta) for c, t in zip(powers, tens)) % r


# ---- errors that need a handle -------------------------------------------------------------------------------------------------------

def test_refusals_judged_against_the_handle(domains, torch_, ea):
    torch = torch_
    field = "bls12_381"
    r = nc.modulus(field)
    c = qc.Rows(field, 5, 4, 5, 0xE44)
    dom = domains(field, 5)
    M, stride = c.M, c.M + 3
    g = lambda a: torch.from_numpy(a).cuda()
    ws, ss, qs = (g(host_columns(c, x, stride)) for x in (c.wires, c.sigmas, c.selectors))
    z = g(np.frombuffer(pc.to_raw(c.raw_z(False)) * 2, dtype=np.uint8).reshape(2 * M, 32).copy())
    out = torch.empty((M, 32), dtype=torch.uint8, device="cuda")
    ks, alpha, beta, gamma = (nc.encode(field, v, False) for v in (c.ks, [c.alpha], [c.beta], [c.gamma]))
    call = dom._lib.mi355_msm_domain_plonk_quotient_device
    tail = (ks, alpha, beta, gamma, None, 0, None)
    _check(ea, call(dom.handle, out.data_ptr(), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 4, *tail))
    torch.cuda.synchronize()
    c.pi = None
    assert raw_of(out) == nc.encode(field, c.model(False), False)
    for args, word in (((out.data_ptr(), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, M - 1, 4), "stride"),
                       ((ws.data_ptr() + 32 * stride, ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 4), "overlaps"),
                       ((qs.data_ptr() + 32 * (12 * stride + M - 1), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 4), "overlaps"),
                       ((z.data_ptr() + 32 * (M - 1), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 4), "overlaps"),
                       ((out.data_ptr(), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 32), "ratio"),
                       ((out.data_ptr(), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 1), "ratio"),
                       ((out.data_ptr(), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 64), "ratio")):
        with pytest.raises(ea.MsmError, match=word) as e:
            _check(ea, call(dom.handle, *args, *tail))
        assert e.value.code == -1
    # an offset inside the domain (its n-th power is a root of unity of order `ratio`), and one that is 0 modulo r
    om = nc.root_of_unity(field, 5)
    for offset, word in ((pow(om, 3, r), "root of unity"), (1, "root of unity")):
        with pytest.raises(ea.MsmError, match=word):
            dom.plonk_quotient(ws, ss, z[:M], c.alpha, c.beta, c.gamma, c.ks, 4, selectors=qs, offset=offset)
    with pytest.raises(ea.MsmError, match="offset is zero"):
        _check(ea, call(dom.handle, out.data_ptr(), ws.data_ptr(), ss.data_ptr(), qs.data_ptr(), z.data_ptr(), None, 5, stride, 4, ks, alpha, beta, gamma,
                        r.to_bytes(32, "little"), 1, None))
    # ratio >= M: a domain of 8 points over a constraint domain of 1 row
    small = domains(field, 3)
    one = torch.zeros((1, 8, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(ea.MsmError, match="ratio"):
        small.plonk_quotient(one, one, one[0], 2, 3, 4, [1], 1)


# ---- speed ---------------------------------------------------------------------------------------------------------------------------

# Modelled without a run, from the products executed per row, against the forward NN transform of the same handle, whose
# products per element at 2^20 are those of DESIGN.md 4e (three passes of 7 + 7 + 6 levels: 20 / 2 in the butterflies, 2 x 2 in the
# two-level twiddles of the two inter-pass stores, 2 in the conversions = 16):
#   rows       27 conversions of the loaded elements (5 wires, 5 sigmas, 13 selectors, z twice, pi, 1 / (x - 1)) + x 2 + the gate 31 (per
#              column below the fifth: q w, w^2, w^4, w^5, q w^5 = 5; w w' and q_mul times it at the odd ones 2 x 2; the running product
#              of the wires 5; q_ecc and q_o 2) + the permutation 5 x 4 + alpha 1 + (z - 1) / (n (x - 1)) 1 + 1 / Z_H 1 + the store 1 = 84
#   inversion  x - 1: 3; the three launches of 4f: 12.2
# 99.2 products a row.
MODEL_RATIO = 99.2 / 16


def speed_bound():
    """(bound on plonk_quotient / forward transform, source): 1.5 x the ratio profiles/quotient.txt recorded, or 2 x the modelled ratio"""
    path = os.path.join(ROOT, "profiles", "quotient.txt")
    if os.path.exists(path):
        m = re.search(r"^bls12_381 ratio plonk_quotient 2\^20 / forward NN 2\^20: ([0-9.]+)", open(path).read(), flags=re.M)
        if m:
            return 1.5 * float(m.group(1)), "profiles/quotient.txt"
    return 2 * MODEL_RATIO, "the model"


def test_speed_guard_against_the_transform(domains, torch_):
    """BLS12-381, M = 2^20, n = 2^17, device-resident random bytes, warmed up, median of 5: the rows against the forward NN transform of
    the same handle, which this change does not touch, run in the same test on the same box.  Bound: 1.5 x the ratio
    profiles/quotient.txt recorded (tools/quotient_bench.py; the margin covers box-to-box spread and clock differences under the power
    limit), or 2 x the modelled ratio above without that file."""
    torch = torch_
    M = 1 << 20
    dom = domains("bls12_381", 20)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED)
    t = torch.randint(0, 256, (25, M, 32), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((M, 32), dtype=torch.uint8, device="cuda")

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

    t_ntt = median5(lambda: dom.fft(t[23], out=out))
    t_q = median5(lambda: dom.plonk_quotient(t[0:5], t[5:10], t[23], 0x1234567, 0x89ABCDE, 0xF012345, [1, 7, 49, 343, 2401], M // 8, selectors=t[10:23], pi=t[24],
                                             out=out))
    bound, source = speed_bound()
    print("2^20: plonk_quotient %.3f ms, forward NN %.3f ms, ratio %.4f, bound %.4f from %s" % (1e3 * t_q, 1e3 * t_ntt, t_q / t_ntt, bound, source))
    assert t_q / t_ntt <= bound
