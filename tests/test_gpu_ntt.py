"""GPU: radix-2 domains over the scalar fields (mi355_msm_domain_*, csrc/ntt.hpp) through the Python layer.  Expected values come from
outside the code under test: the big-integer model of tests/ntt_cases.py at small sizes, closed forms at size (a geometric input, a
handful of impulses, Horner at three points), schoolbook products, and the CPU oracle's MSM for the chain into ctx.run."""
import ctypes
import os
import random
import re
import statistics
import time

import numpy as np
import pytest

import ntt_cases as nc
import stream_cases as st
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
        d.set_option("pass_log", 0)
        return d

    yield get
    for d in made.values():
        d.close()


_MODEL = {}


def model(field, k, kind, seed=0x77, in_len=None, order=0, offset=None):
    """(input integers, expected integers), computed once per case"""
    key = (field, k, kind, seed, in_len, order, offset)
    if key not in _MODEL:
        n = 1 << k
        x = nc.random_values(field, n, seed + k)
        cut = n if in_len is None else in_len
        _MODEL[key] = (x, nc.transform(field, k, kind, [v if i < cut else 0 for i, v in enumerate(x)], offset=offset, order_flags=order))
    return _MODEL[key]


CALLS = {nc.FORWARD: "fft", nc.INVERSE: "ifft", nc.COSET_FORWARD: "coset_fft", nc.COSET_INVERSE: "coset_ifft"}


def call(dom, kind, values, **kw):
    return getattr(dom, CALLS[kind])(values, **kw)


def dev(torch, raw, shape=None):
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    return t.reshape(shape if shape else (-1, 32))


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else bytes(t)


# ---- small sizes, byte-equal to the model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", range(18))
def test_small_sizes_against_the_model(domains, torch_, field, k):
    """forward and inverse at every k; the coset pair at k in {0, 1, 5, 11, 17}; device tensors, default pass_log"""
    dom = domains(field, k)
    assert dom.size == 1 << k and dom.log_size_of_group == k
    kinds = [nc.FORWARD, nc.INVERSE] + ([nc.COSET_FORWARD, nc.COSET_INVERSE] if k in (0, 1, 5, 11, 17) else [])
    for kind in kinds:
        x, y = model(field, k, kind)
        got = call(dom, kind, dev(torch_, nc.encode(field, x, False)))
        assert raw_of(got) == nc.encode(field, y, False), (field, k, kind)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", (7, 10, 11, 13))
def test_forced_pass_sizes(domains, torch_, field, k):
    """pass_log 2, 3 and 5: pass boundaries, a ragged last pass, three- and four-pass (and longer) chains"""
    dom = domains(field, k)
    for pass_log in (2, 3, 5):
        dom.set_option("pass_log", pass_log)
        assert dom.query("pass_log") == pass_log and dom.query("passes") == -(-k // pass_log)
        for kind in (nc.FORWARD, nc.INVERSE):
            x, y = model(field, k, kind)
            got = call(dom, kind, dev(torch_, nc.encode(field, x, False)))
            assert raw_of(got) == nc.encode(field, y, False), (field, k, pass_log, kind)
    dom.set_option("pass_log", 0)
    assert dom.query("pass_log") == 8


# ---- contract corners at k = 10 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_inputs_above_the_modulus(domains, torch_, field):
    k, n = 10, 1024
    dom = domains(field, k)
    raw = b"".join(v.to_bytes(32, "little") for v in (nc.edge_values(field) * 171)[:n])
    for montgomery in (True, False):
        vals = nc.decode(field, raw, not montgomery)
        for kind in range(4):
            got = call(dom, kind, dev(torch_, raw), montgomery=montgomery)
            assert raw_of(got) == nc.encode(field, nc.transform(field, k, kind, vals), not montgomery), (kind, montgomery)


@pytest.mark.parametrize("field", FIELDS)
def test_short_inputs_and_batches(domains, torch_, field):
    """in_len 0, 1 and n - 1 (zero-extended); batches of 1, 2 and 5 distinct vectors; in place against out of place"""
    k, n = 10, 1024
    dom = domains(field, k)
    x, _ = model(field, k, nc.FORWARD)
    for in_len in (0, 1, n - 1):
        want = nc.encode(field, nc.transform(field, k, nc.FORWARD, x[:in_len]), False)
        assert raw_of(dom.fft(nc.encode(field, x[:in_len], False))) == want                      # host pointers
        if in_len:
            assert raw_of(dom.fft(dev(torch_, nc.encode(field, x[:in_len], False)))) == want     # device pointers
    for batch in (1, 2, 5):
        vecs = [model(field, k, nc.INVERSE, seed=0x900 + b) for b in range(batch)]
        raw = b"".join(nc.encode(field, v, False) for v, _ in vecs)
        want = b"".join(nc.encode(field, y, False) for _, y in vecs)
        t = dev(torch_, raw, (batch, n, 32))
        got = dom.ifft(t)
        assert tuple(got.shape) == (batch, n, 32) and raw_of(got) == want
        assert raw_of(dom.ifft(np.frombuffer(raw, dtype=np.uint8).reshape(batch, n, 32))) == want
        for pass_log in (0, 5):   # one pass (copied back) and two
            dom.set_option("pass_log", pass_log)
            t2 = t.clone()
            assert dom.ifft(t2, out=t2) is t2 and raw_of(t2) == want
        dom.set_option("pass_log", 0)


@pytest.mark.parametrize("field", FIELDS)
def test_host_and_device_pointers_and_streams(domains, torch_, delay, field):
    torch = torch_
    k = 10
    dom = domains(field, k)
    for kind in range(4):
        x, y = model(field, k, kind)
        raw, want = nc.encode(field, x, False), nc.encode(field, y, False)
        assert dom_bytes(call(dom, kind, raw)) == want
        s = torch.cuda.Stream()
        d = st.late(torch, raw, s, delay, shape=(-1, 32))                             # produced LATE on s: poison until then
        assert st.window_open(d.produced)
        with torch.cuda.stream(s):
            got = call(dom, kind, d)
        s.synchronize()
        assert st.closed(d)
        assert raw_of(got) == want


@pytest.fixture(scope="module")
def delay(torch_):
    """the calibrated delay of tests/stream_cases.py, once for the module"""
    return st.Delay(torch_, torch_.cuda.Stream())


def dom_bytes(out):
    return out if isinstance(out, bytes) else raw_of(out)


@pytest.mark.parametrize("field", FIELDS)
def test_orders_and_offsets(domains, torch_, field):
    """NR then RN equals NN then NN; NR is the bit-reversed NN; offset 1 is the plain transform; a custom offset"""
    k, n = 10, 1024
    dom = domains(field, k)
    r = nc.modulus(field)
    x, y = model(field, k, nc.FORWARD)
    t = dev(torch_, nc.encode(field, x, False))
    nr = dom.fft(t, order="NR")
    assert raw_of(nr) == nc.encode(field, [y[nc.bitrev(i, k)] for i in range(n)], False)
    assert raw_of(dom.ifft(nr, order="RN")) == raw_of(dom.ifft(dom.fft(t))) == nc.encode(field, x, False)
    cnr = dom.coset_fft(t, order="NR")
    assert raw_of(dom.coset_ifft(cnr, order="RN")) == nc.encode(field, x, False)
    assert raw_of(dom.coset_fft(t, offset=1)) == raw_of(dom.fft(t))
    assert raw_of(dom.coset_ifft(t, offset=1)) == raw_of(dom.ifft(t))
    off = 0xC0FFEE * 31 % r
    for kind in (nc.COSET_FORWARD, nc.COSET_INVERSE):
        for montgomery in (True, False):
            xs, ys = model(field, k, kind, offset=off)
            got = call(dom, kind, dev(torch_, nc.encode(field, xs, not montgomery)), offset=off, montgomery=montgomery)
            assert raw_of(got) == nc.encode(field, ys, not montgomery)
    assert dom.element(1) == dom.group_gen == nc.root_of_unity(field, k) and dom.size_inv == pow(n, -1, r)
    assert dom.element(n - 1) == pow(nc.root_of_unity(field, k), n - 1, r) and dom.element(0) == 1


def test_error_paths(ea, domains, torch_):
    """argument errors: -1 with a message, decided before any device call"""
    lib = ea.load_library()
    dom = domains("bls12_381", 10)
    h = dom.handle
    buf = torch_.zeros((2048, 32), dtype=torch_.uint8, device="cuda")
    p = buf.data_ptr()

    def refused(err, word):
        assert err.code == -1
        msg = ctypes.string_at(err.message).decode()
        assert word in msg, msg

    refused(lib.mi355_msm_domain_transform_device(None, p, p, 1024, 1, 0, 0, None, None), "null")
    refused(lib.mi355_msm_domain_transform_device(h, None, p, 1024, 1, 0, 0, None, None), "null")
    refused(lib.mi355_msm_domain_transform_device(h, p, None, 1024, 1, 0, 0, None, None), "null")
    refused(lib.mi355_msm_domain_transform(h, None, None, 0, 1, 0, 0, None), "null")
    refused(lib.mi355_msm_domain_transform_device(h, p, p, 1025, 1, 0, 0, None, None), "in_len")
    refused(lib.mi355_msm_domain_transform_device(h, p + 32, p, 1024, 1, 0, 0, None, None), "overlap")
    refused(lib.mi355_msm_domain_transform_device(h, p + 32 * 1024, p, 1024, 2, 0, 0, None, None), "overlap")
    refused(lib.mi355_msm_domain_transform_device(h, p, p, 1024, 1, 0, 8, None, None), "flag")
    refused(lib.mi355_msm_domain_transform_device(h, p, p, 1024, 1, 1, 2, None, None), "forward")
    refused(lib.mi355_msm_domain_transform_device(h, p, p, 1024, 1, 0, 4, None, None), "inverse")
    refused(lib.mi355_msm_domain_transform_device(h, p, p, 1024, 1, 4, 0, None, None), "kind")
    refused(lib.mi355_msm_domain_transform_device(h, p, p, 1024, 1, 0, 0, bytes(32), None), "offset")
    refused(lib.mi355_msm_domain_transform_device(h, p, p, 1024, 1, 2, 0, bytes(32), None), "zero")
    refused(lib.mi355_msm_domain_mul_device(h, p, None, p, 4, 0, None), "null")
    refused(lib.mi355_msm_domain_mul_device(h, p, p, p, 4, 2, None), "flag")
    refused(lib.mi355_msm_domain_set_option(h, b"pass_log", 11), "pass_log")
    refused(lib.mi355_msm_domain_set_option(h, b"nothing", 1), "unknown")
    assert raw_of(buf) == bytes(2048 * 32)            # no refused call wrote anything
    new = ctypes.c_void_p()
    refused(lib.mi355_msm_domain_create(ctypes.byref(new), 1, -1, (1 << 28) + 1), "2^28")
    refused(lib.mi355_msm_domain_create(ctypes.byref(new), 1, -1, (1 << 32) + 1), "2-adicity")
    refused(lib.mi355_msm_domain_create(ctypes.byref(new), 0, -1, (1 << 32) + 1), "2^28")
    refused(lib.mi355_msm_domain_create(ctypes.byref(new), 9, -1, 16), "curve")
    refused(lib.mi355_msm_domain_create(None, 0, -1, 16), "null")
    assert not new.value
    with pytest.raises(ea.MsmError):
        dom.fft(bytes(32 * 1025))
    with pytest.raises(ValueError):
        dom.fft(bytes(32), order="RR")


# ---- at size: closed forms ----------------------------------------------------------------------------------------------------------

def sample_indices(n, seed, count=4096):
    rng = random.Random(seed)
    return sorted(set(rng.randrange(n) for _ in range(count)) | {0, 1, n // 2 - 1, n // 2, n - 1})


def rows_at(torch, t, idx):
    sel = t[torch.tensor(idx, device=t.device)].cpu().numpy()
    return [int.from_bytes(bytes(row), "little") for row in sel]


@pytest.mark.parametrize("field", FIELDS)
def test_geometric_input_at_2_22(domains, torch_, field):
    """in[j] = z^j, so out[i] = (z^n - 1) / (z omega^i - 1): every input position carries its own weight"""
    k = 22
    n, r = 1 << k, nc.modulus(field)
    z = 0x1234567 * 0x89ABCDEF % r
    vals, acc = bytearray(32 * n), nc.MONT % r      # arkworks images: z^j * 2^256
    for j in range(n):
        vals[32 * j:32 * j + 32] = acc.to_bytes(32, "little")
        acc = acc * z % r
    out = domains(field, k).fft(dev(torch_, vals))
    idx = sample_indices(n, 0x6E0)
    omega = nc.root_of_unity(field, k)
    top = (pow(z, n, r) - 1) % r
    got = rows_at(torch_, out, idx)
    for i, g in zip(idx, got):
        assert g == top * pow(z * pow(omega, i, r) - 1, -1, r) % r * nc.MONT % r, i


@pytest.mark.parametrize("field", FIELDS)
def test_five_impulses_at_2_24(domains, torch_, field):
    """impulses at 0, 1, n/2, n - 1 and one random index: out[i] = sum c_j (g omega^i)^j, plain and over the coset"""
    torch = torch_
    k = 24
    n, r = 1 << k, nc.modulus(field)
    rng = random.Random(0x1A9)
    where = [0, 1, n // 2, n - 1, rng.randrange(2, n // 2)]
    coef = [rng.randrange(1, r) for _ in where]
    t = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    for j, c in zip(where, coef):
        t[j] = torch.frombuffer(bytearray(c.to_bytes(32, "little")), dtype=torch.uint8).cuda()
    dom = domains(field, k)
    omega = nc.root_of_unity(field, k)
    idx = sample_indices(n, 0x1AA)
    for kind, g in ((nc.FORWARD, 1), (nc.COSET_FORWARD, nc.generator(field))):
        out = call(dom, kind, t, montgomery=False)
        for i, got in zip(idx, rows_at(torch, out, idx)):
            e = g * pow(omega, i, r) % r
            assert got == sum(c * pow(e, j, r) for j, c in zip(where, coef)) % r, (kind, i)
        del out


@pytest.mark.parametrize("field", FIELDS)
def test_dense_random_at_2_20(domains, torch_, field):
    """three outputs by Horner on the CPU"""
    k = 20
    n, r = 1 << k, nc.modulus(field)
    raw = np.random.default_rng(0xD5E).integers(0, 256, size=(n, 32), dtype=np.uint8)
    coeffs = [int.from_bytes(bytes(row), "little") % r for row in raw]
    out = domains(field, k).fft(torch_.from_numpy(raw).cuda(), montgomery=False)
    omega = nc.root_of_unity(field, k)
    idx = [1, n // 2 + 3, n - 1]
    for i, got in zip(idx, rows_at(torch_, out, idx)):
        e, acc = pow(omega, i, r), 0
        for c in reversed(coeffs):
            acc = (acc * e + c) % r
        assert got == acc, i


def random_canonical(torch, shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 256, shape + (32,), dtype=torch.uint8, device="cuda", generator=g)
    t[..., 31] &= 0x0F        # below 2^252: canonical in both fields
    return t


@pytest.mark.parametrize("field", FIELDS)
def test_round_trips_at_2_22(domains, torch_, field):
    torch = torch_
    dom = domains(field, 22)
    x = random_canonical(torch, (1 << 22,), 0x22)
    assert torch.equal(dom.ifft(dom.fft(x)), x)
    assert torch.equal(dom.coset_ifft(dom.coset_fft(x)), x)
    assert torch.equal(dom.ifft(dom.fft(x, order="NR"), order="RN"), x)
    assert torch.equal(dom.coset_ifft(dom.coset_fft(x, order="NR"), order="RN"), x)
    y = dom.fft(x)
    assert not torch.equal(y, x)
    z = x.clone()
    assert dom.fft(z, out=z) is z and torch.equal(z, y)      # in place at size


@pytest.mark.parametrize("field", FIELDS)
def test_batch_of_four_at_2_20(domains, torch_, field):
    torch = torch_
    dom = domains(field, 20)
    x = random_canonical(torch, (4, 1 << 20), 0x44)
    got = dom.fft(x)
    for b in range(4):
        assert torch.equal(got[b], dom.fft(x[b].contiguous())), b
    assert torch.equal(dom.ifft(got), x)


# ---- polynomial products ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_polynomial_product(domains, torch_, field):
    """degree below 2^9 each, through fft, fft, mul, ifft at n = 2^10, against schoolbook multiplication"""
    r = nc.modulus(field)
    dom = domains(field, 10)
    a, b = nc.random_values(field, 512, 0xAA), nc.random_values(field, 512, 0xBB)
    want = [0] * 1024
    for i, u in enumerate(a):
        for j, v in enumerate(b):
            want[i + j] = (want[i + j] + u * v) % r
    for montgomery in (True, False):
        ea_, eb_ = dom.fft(dev(torch_, nc.encode(field, a, not montgomery)), montgomery=montgomery), dom.fft(dev(torch_, nc.encode(field, b, not montgomery)), montgomery=montgomery)
        prod = dom.ifft(dom.mul(ea_, eb_, montgomery=montgomery), montgomery=montgomery)
        assert raw_of(prod) == nc.encode(field, want, not montgomery)
    # the product alone, host pointers, inputs above the modulus included
    edges = nc.edge_values(field)
    ra, rb = b"".join(v.to_bytes(32, "little") for v in edges for _ in edges), b"".join(v.to_bytes(32, "little") for _ in edges for v in edges)
    for montgomery in (True, False):
        va, vb = nc.decode(field, ra, not montgomery), nc.decode(field, rb, not montgomery)
        assert dom_bytes(dom.mul(ra, rb, montgomery=montgomery)) == nc.encode(field, [u * v for u, v in zip(va, vb)], not montgomery)


@pytest.mark.parametrize("field", FIELDS)
def test_sparse_product_at_2_20(domains, torch_, field):
    torch = torch_
    k = 20
    n, r = 1 << k, nc.modulus(field)
    rng = random.Random(0x5BA)
    dom = domains(field, k)

    def sparse():
        terms = {rng.randrange(n // 2): rng.randrange(1, r) for _ in range(8)}
        terms[n // 2 - 1] = rng.randrange(1, r)
        t = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        for j, c in terms.items():
            t[j] = torch.frombuffer(bytearray(c.to_bytes(32, "little")), dtype=torch.uint8).cuda()
        return terms, t

    (ta, a), (tb, b) = sparse(), sparse()
    want = {}
    for i, u in ta.items():
        for j, v in tb.items():
            want[i + j] = (want.get(i + j, 0) + u * v) % r
    prod = dom.ifft(dom.mul(dom.fft(a, montgomery=False), dom.fft(b, montgomery=False), montgomery=False), montgomery=False)
    idx = sorted(want)
    assert rows_at(torch, prod, idx) == [want[i] for i in idx]
    assert int(torch.count_nonzero(prod.any(dim=1))) == sum(1 for v in want.values() if v)


# ---- into the MSM ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_ifft_feeds_the_msm(ea, oracle, domains, torch_, field):
    """2^12 evaluations on the GPU -> ifft -> ctx.run under scalars_montgomery, byte-equal to the CPU oracle's MSM over the model's
    coefficients; again with normal-form elements and the option off"""
    torch = torch_
    k, n = 12, 4096
    curve = CURVE_OF[field]
    cid = ea.CURVE_IDS[curve]
    dom = domains(field, k)
    evals, coeffs = model(field, k, nc.INVERSE, seed=0x3141)
    bases = ea.generate_points(n, distinct=n, seed=0xBA5E, curve=curve)
    scal = np.frombuffer(nc.encode(field, coeffs, True), dtype=np.uint8).reshape(n, 32)
    exp = ctypes.create_string_buffer(ea.projective_bytes(curve))
    assert oracle.oracle_msm(cid, bases.ctypes.data, ea.affine_stride(curve), scal.ctypes.data, n, exp, 0) == 0
    ctx = ea.multi_scalar_mult_init(torch.from_numpy(bases).cuda(), curve)
    try:
        for montgomery in (True, False):
            d = dom.ifft(dev(torch, nc.encode(field, evals, not montgomery)), montgomery=montgomery)
            assert d.is_cuda
            ctx.set_option("scalars_montgomery", 1 if montgomery else 0)
            assert ctx.run(d)[0] == exp.raw, montgomery
    finally:
        ctx.close()


# ---- speed ------------------------------------------------------------------------------------------------------------------------------

# Modelled without a run, from counts: a forward transform of 2^22 elements of BLS12-381 Fr is three passes (8 + 7 + 7 levels).
#   multiply-adds per element: 22 levels x 153 / 2 (one 9 x 29 product per butterfly) + 2 inter-pass stores x 2 products (two-level
#   twiddle) + 2 conversions, 153 each: 1683 + 612 + 306 = 2601; x 2^22 = 1.09e10.
#   v_mad_u64_u32 issues at 4.3 cycles per wave: 256 CUs x 4 SIMDs x 64 lanes / 4.3 x 2.4 GHz = 3.66e13 / s -> 0.30 ms;
#   the column shifts, masks, carries and index arithmetic cost about as much again -> 0.6 ms.
#   bytes: 3 passes x 2 x 128 MiB = 0.81 GB, 0.2 ms at 4 TB/s, under the arithmetic.
# One MSM of 2^22 pairs on BLS12-381 G1 takes 11.2 ms, so the modelled ratio is 0.6 / 11.2.
MODEL_RATIO = 0.6 / 11.2


def speed_bound():
    """(bound on transform / MSM, source): 1.5 x the ratio profiles/ntt.txt recorded, or 2 x the modelled ratio without that file"""
    path = os.path.join(ROOT, "profiles", "ntt.txt")
    if os.path.exists(path):
        m = re.search(r"^bls12_381 ratio forward NN 2\^22 / msm 2\^22: ([0-9.]+)", open(path).read(), flags=re.M)
        if m:
            return 1.5 * float(m.group(1)), "profiles/ntt.txt"
    return 2 * MODEL_RATIO, "the model"


def test_speed_guard_against_the_msm(ea, domains, torch_):
    """BLS12-381: forward NN at 2^22 on device-resident data, warmed up, median of 5, against one ctx.run of 2^22 pairs on BLS12-381
    G1 in the same test on the same box.  Bound: 1.5 x the ratio profiles/ntt.txt recorded (tools/ntt_bench.py; the margin covers
    box-to-box spread and clock differences under the power limit), or 2 x the modelled ratio above without that file."""
    torch = torch_
    n = 1 << 22
    dom = domains("bls12_381", 22)
    x = random_canonical(torch, (n,), 0x5EED)
    out = torch.empty_like(x)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    dom.fft(x, out=out)
    t_ntt = statistics.median(once(lambda: dom.fft(x, out=out)) for _ in range(5))
    bases = ea.generate_points(n, distinct=1 << 15, seed=0x5EED, curve="bls12_381_g1")
    ctx = ea.multi_scalar_mult_init(torch.from_numpy(bases).cuda(), "bls12_381_g1")
    try:
        ctx.run(x)
        t_msm = once(lambda: ctx.run(x))
    finally:
        ctx.close()
    bound, source = speed_bound()
    print("2^22: forward NN %.3f ms (device %.3f ms), MSM %.3f ms, ratio %.4f, bound %.4f from %s"
          % (1e3 * t_ntt, dom.query("last_device_us") / 1e3, 1e3 * t_msm, t_ntt / t_msm, bound, source))
    assert t_ntt / t_msm <= bound
