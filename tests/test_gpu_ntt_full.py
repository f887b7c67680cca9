"""GPU: the radix-2 domains (mi355_msm_domain_*, csrc/ntt.hpp) at size, every output compared.  Up to 2^22 the expected vectors come
from the CPU oracle's plain NTT (oracle/ntt_oracle.c, pinned by tests/test_ntt_oracle.py), computed once per module; at 2^25 (the
first default plan of four passes) and 2^28 (the largest domain) from the oracle's 2^22 vector by decimation -- the transform of a
vector of 2^22 coefficients, zero-extended, holds the 2^22-point transform at every 8th (64th) output -- and from the modulation
identity fft(x[j] w^(m j))[i] = fft(x)[i + m] at full density, which reaches every output.  A mismatch reports how many elements
differ, the first few indices and their tiles (index >> 10: a block of the kernel owns 1024 elements), which points at a pass."""
import ctypes
import random

import numpy as np
import pytest

import ntt_cases as nc

pytestmark = pytest.mark.gpu

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
CALLS = {nc.FORWARD: "fft", nc.INVERSE: "ifft", nc.COSET_FORWARD: "coset_fft", nc.COSET_INVERSE: "coset_ifft"}
IMPULSE_AT = 0x4C3B            # odd and above 2^14: its powers of the root take both levels of the twiddle table
MIN_FREE_AT_2_28 = 72 << 30    # seven vectors of 8 GiB and some room


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def domains(ea):
    """one domain per (field, k <= 22) for the whole module; the larger ones live inside their tests"""
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


_INPUT, _EXPECTED = {}, {}


def random_bytes(n, seed):
    """(n, 32) uint8 from the host's generator, drawn as 64-bit words"""
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64).view(np.uint8).reshape(n, 32)


def host_input(field, k, which=0):
    """2^k random 256-bit values (about seven in eight of them above the modulus), fixed per (field, k, which)"""
    key = (field, k, which)
    if key not in _INPUT:
        _INPUT[key] = random_bytes(1 << k, 0xF0117 + 1000 * k + 10 * which + nc.FIELD_IDS[field])
        _INPUT[key].setflags(write=False)
    return _INPUT[key]


def expected(oracle, field, k, kind, flags=0, in_len=None, offset=None, which=0):
    """the oracle's transform of host_input(field, k, which)[:in_len], computed once; `offset` an integer or None"""
    key = (field, k, kind, flags, in_len, offset, which)
    if key not in _EXPECTED:
        off = None if offset is None else nc.encode(field, [offset], bool(flags & nc.FLAG_NORMAL))
        x = host_input(field, k, which)
        _EXPECTED[key] = nc.oracle_ntt(oracle, field, k, kind, flags, x, in_len=len(x) if in_len is None else in_len, offset=off)
        _EXPECTED[key].setflags(write=False)
    return _EXPECTED[key]


def dev(torch, arr):
    return torch.from_numpy(np.array(arr, copy=True)).cuda()


def assert_same(torch, got, want, what):
    """every byte; on a mismatch: the count, the first indices and their tiles"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    g, w = got.reshape(-1, 32), want.reshape(-1, 32)
    count, first = 0, []
    for at in range(0, g.shape[0], 1 << 22):      # in pieces: the masks of an 8 GiB vector stay small
        bad = (g[at:at + (1 << 22)] != w[at:at + (1 << 22)]).any(dim=1).nonzero().flatten()
        count += int(bad.numel())
        if len(first) < 8:
            first += [at + int(i) for i in bad[:8 - len(first)].tolist()]
    pytest.fail("%s: %d of %d elements differ; first indices %s, tiles %s" % (what, count, g.shape[0], first, [i >> 10 for i in first]))


def kw_of(flags):
    order = "NR" if flags & nc.FLAG_NR else "RN" if flags & nc.FLAG_RN else "NN"
    return {"montgomery": not (flags & nc.FLAG_NORMAL), "order": order}


def check(torch, oracle, dom, field, k, kind, flags=0, in_len=None, offset=None):
    """one call on host_input(field, k)[:in_len] against the oracle; offset None: the call's default, the generator"""
    x = host_input(field, k)
    kw = kw_of(flags) if offset is None else dict(kw_of(flags), offset=offset)
    got = getattr(dom, CALLS[kind])(dev(torch, x if in_len is None else x[:in_len]), **kw)
    want = dev(torch, expected(oracle, field, k, kind, flags, in_len, offset))
    assert_same(torch, got, want, "%s 2^%d %s flags %d in_len %s offset %s" % (field, k, CALLS[kind], flags, in_len, offset))


def offsets_of(field):
    r = nc.modulus(field)
    return 0xC0FFEE * 31 % r, r - 5


# ---- 2^18: plan 6 + 6 + 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_four_kinds_at_2_18(oracle, domains, torch_, field):
    dom = domains(field, 18)
    assert dom.query("passes") == 3
    for kind in range(4):
        check(torch_, oracle, dom, field, 18, kind)


@pytest.mark.parametrize("field", FIELDS)
def test_offsets_in_sequence_at_2_18(oracle, ea, torch_, field):
    """one handle of its own: the offset tables are built for g1, rebuilt for 1 / g1, for g2, for the generator and for 1 / g2, each time
    on the caller's stream just ahead of the passes that read them"""
    g1, g2 = offsets_of(field)
    with ea.Radix2EvaluationDomain(1 << 18, CURVE_OF[field]) as dom:
        for kind, offset in ((nc.COSET_FORWARD, g1), (nc.COSET_INVERSE, g1), (nc.COSET_FORWARD, g2), (nc.COSET_FORWARD, None), (nc.COSET_INVERSE, g2)):
            check(torch_, oracle, dom, field, 18, kind, offset=offset)


@pytest.mark.parametrize("field", FIELDS)
def test_batch_of_three_at_2_18(oracle, domains, torch_, field):
    """three distinct vectors: out of place; in place over an odd pass count (the result is copied back from the work vectors) and over
    an even one (pass_log 5: 5 + 5 + 4 + 4)"""
    torch = torch_
    dom = domains(field, 18)
    x = torch.stack([dev(torch, host_input(field, 18, which)) for which in range(3)])
    want = torch.stack([dev(torch, expected(oracle, field, 18, nc.FORWARD, which=which)) for which in range(3)])
    assert_same(torch, dom.fft(x), want, field + " batch of 3, out of place")
    for pass_log, passes in ((0, 3), (5, 4)):
        dom.set_option("pass_log", pass_log)
        assert dom.query("passes") == passes
        t = x.clone()
        assert dom.fft(t, out=t) is t
        assert_same(torch, t, want, "%s batch of 3, in place, %d passes" % (field, passes))
    dom.set_option("pass_log", 0)


# ---- 2^20: plan 7 + 7 + 6 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_four_kinds_at_2_20(oracle, domains, torch_, field):
    dom = domains(field, 20)
    assert dom.query("passes") == 3
    for kind in range(4):
        check(torch_, oracle, dom, field, 20, kind)


@pytest.mark.parametrize("field", FIELDS)
def test_orders_and_normal_form_at_2_20(oracle, domains, torch_, field):
    dom = domains(field, 20)
    check(torch_, oracle, dom, field, 20, nc.FORWARD, nc.FLAG_NR)
    check(torch_, oracle, dom, field, 20, nc.INVERSE, nc.FLAG_RN)
    check(torch_, oracle, dom, field, 20, nc.FORWARD, nc.FLAG_NORMAL)


@pytest.mark.parametrize("field", FIELDS)
def test_short_inputs_at_2_20(oracle, domains, torch_, field):
    dom = domains(field, 20)
    n = 1 << 20
    for in_len in (1, n // 2 + 1, n - 1):
        check(torch_, oracle, dom, field, 20, nc.FORWARD, in_len=in_len)


# ---- 2^22: plan 8 + 7 + 7 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_forward_and_coset_inverse_at_2_22(oracle, domains, torch_, field):
    """(the forward vector is what the 2^25 and 2^28 tests decimate to)"""
    dom = domains(field, 22)
    assert dom.query("passes") == 3
    check(torch_, oracle, dom, field, 22, nc.FORWARD)
    check(torch_, oracle, dom, field, 22, nc.COSET_INVERSE)


# ---- 2^25 and 2^28: decimation and modulation --------------------------------------------------------------------------------------------

def random_canonical(torch, n, seed, on_host):
    """n random elements below 2^252 (canonical in both fields, so that a round trip returns the very bytes)"""
    if on_host:
        t = torch.from_numpy(random_bytes(n, seed)).cuda()
    else:
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        t = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        for at in range(0, n, 1 << 24):
            t[at:at + (1 << 24)].random_(0, 256, generator=g)
    t[:, 31] &= 0x0F
    return t


def check_decimation(torch, oracle, dom, field, k):
    """fft of the 2^22 input, zero-extended to 2^k: out[2^(k-22) i] = Y22[i] for every i (w_(2^k)^(2^(k-22)) is the root of the 2^22 domain)"""
    y22 = dev(torch, expected(oracle, field, 22, nc.FORWARD))
    out = dom.fft(dev(torch, host_input(field, 22)))
    assert tuple(out.shape) == (1 << k, 32)
    assert_same(torch, out[::1 << (k - 22)], y22, "%s 2^%d decimation to 2^22 (indices and tiles of the 2^22 vector)" % (field, k))


def impulse_response(torch, dom, field, k):
    """w = fft(e_m), m = IMPULSE_AT: w[j] = omega^(m j); 64 entries against pow"""
    n, r, m = 1 << k, nc.modulus(field), IMPULSE_AT
    e = torch.zeros((m + 1, 32), dtype=torch.uint8, device="cuda")     # in_len = m + 1, zero-extended
    e[m] = torch.frombuffer(bytearray(nc.encode(field, [1], False)), dtype=torch.uint8).cuda()
    w = dom.fft(e)
    rng = random.Random(0x1A9 + k)
    idx = sorted({0, 1, n // 2, n - 1} | {rng.randrange(n) for _ in range(60)})
    rows = w[torch.tensor(idx, device="cuda")].cpu().numpy()
    omega = nc.root_of_unity(field, k)
    for j, row in zip(idx, rows):
        assert bytes(row) == nc.encode(field, [pow(omega, m * j, r)], False), (field, k, j)
    return w


def assert_rolled(torch, got, base, what):
    """got == roll(base, -m) along the elements, without building the rolled vector"""
    n, m = base.shape[0], IMPULSE_AT
    assert_same(torch, got[:n - m], base[m:], what + " (indices i: out[i] against fft(x)[i + m])")
    assert_same(torch, got[n - m:], base[:m], what + " (the last m outputs, which wrap)")


@pytest.mark.parametrize("field", FIELDS)
def test_four_passes_at_2_25(oracle, ea, torch_, field):
    """7 + 7 + 6 + 5, 1 GiB per vector: decimation to the oracle's 2^22 vector, modulation for fft and coset_fft, round trips"""
    torch = torch_
    k, n = 25, 1 << 25
    with ea.Radix2EvaluationDomain(n, CURVE_OF[field]) as dom:
        assert dom.query("passes") == 4
        check_decimation(torch, oracle, dom, field, k)
        w = impulse_response(torch, dom, field, k)
        x = random_canonical(torch, n, 0x25 + nc.FIELD_IDS[field], on_host=True)
        xw = dom.mul(x, w)
        del w
        fx = dom.fft(x)
        assert_rolled(torch, dom.fft(xw), fx, field + " 2^25 fft of the modulated vector")
        assert_same(torch, dom.ifft(fx), x, field + " 2^25 ifft(fft(x))")
        del fx
        cx = dom.coset_fft(x)
        assert_rolled(torch, dom.coset_fft(xw), cx, field + " 2^25 coset_fft of the modulated vector")
        del cx, xw
        assert_same(torch, dom.coset_ifft(dom.coset_fft(x, order="NR"), order="RN"), x, field + " 2^25 coset_ifft(coset_fft(x, NR), RN)")


@pytest.mark.parametrize("field", FIELDS)
def test_the_largest_domain_2_28(oracle, ea, torch_, field):
    """7 + 7 + 7 + 7, 8 GiB per vector: decimation, modulation and the round trip for fft; every tensor goes as soon as it has been
    compared.  (The full-length vector is drawn on the device: 8 GiB from the host's generator would take longer than the test.)"""
    torch = torch_
    free = torch.cuda.mem_get_info()[0]
    if free < MIN_FREE_AT_2_28:
        pytest.skip("%.1f GiB of device memory free; this test needs %d GiB" % (free / 2**30, MIN_FREE_AT_2_28 >> 30))
    k, n = 28, 1 << 28
    with ea.Radix2EvaluationDomain(n, CURVE_OF[field]) as dom:
        assert dom.query("passes") == 4
        check_decimation(torch, oracle, dom, field, k)
        w = impulse_response(torch, dom, field, k)
        x = random_canonical(torch, n, 0x28 + nc.FIELD_IDS[field], on_host=False)
        xw = dom.mul(x, w)
        del w
        fx = dom.fft(x)
        fxw = dom.fft(xw, out=xw)
        assert_rolled(torch, fxw, fx, field + " 2^28 fft of the modulated vector")
        del fxw, xw
        back = dom.ifft(fx, out=fx)
        assert_same(torch, back, x, field + " 2^28 ifft(fft(x))")
        del back, fx, x
    torch.cuda.empty_cache()


# ---- the pointwise product and host staging, against Python integers -----------------------------------------------------------------------

def product_case(field, n, seed):
    """(a bytes, b bytes): random 256-bit values, the corners of the input range at the front"""
    rng = random.Random(seed)
    edges = nc.edge_values(field)
    a = [rng.getrandbits(256) for _ in range(n)]
    b = [rng.getrandbits(256) for _ in range(n)]
    for i in range(min(n, len(edges))):
        a[i], b[i] = edges[i], edges[-1 - i]
    return b"".join(v.to_bytes(32, "little") for v in a), b"".join(v.to_bytes(32, "little") for v in b)


def product_expected(field, ra, rb, montgomery):
    va, vb = nc.decode(field, ra, not montgomery), nc.decode(field, rb, not montgomery)
    return nc.encode(field, [u * v for u, v in zip(va, vb)], not montgomery)


@pytest.mark.parametrize("field", FIELDS)
def test_product_lengths_off_the_block_size(domains, torch_, field):
    """device pointers: 1, 255, 257 and 1000 elements (a block of the kernel is 256 lanes); the bytes past the end stay as they were"""
    torch = torch_
    dom = domains(field, 10)
    for n in (1, 255, 257, 1000):
        ra, rb = product_case(field, n, 0xAB + n)
        a, b = (torch.frombuffer(bytearray(v), dtype=torch.uint8).cuda().reshape(n, 32) for v in (ra, rb))
        for montgomery in (True, False):
            out = torch.full((n + 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
            head = out[:n]
            assert dom.mul(a, b, montgomery=montgomery, out=head) is head
            assert out[:n].cpu().numpy().tobytes() == product_expected(field, ra, rb, montgomery), (n, montgomery)
            assert bool((out[n] == 0xA5).all()), (n, montgomery)


@pytest.mark.parametrize("field", FIELDS)
def test_product_of_several_host_pieces(ea, field):
    """host pointers at a domain of 16: 3 * 16 + 5 elements go through the staged vector in three whole pieces and a ragged one"""
    n = 3 * 16 + 5
    ra, rb = product_case(field, n, 0x1605)
    with ea.Radix2EvaluationDomain(16, CURVE_OF[field]) as dom:
        for montgomery in (True, False):
            assert bytes(dom.mul(ra, rb, montgomery=montgomery)) == product_expected(field, ra, rb, montgomery), montgomery


@pytest.mark.parametrize("field", FIELDS)
def test_host_batch_of_short_vectors(ea, field):
    """host pointers, batch 3, in_len = n/2 + 1 at 2^10 on one handle, through the C ABI (the Python layer zero-extends single vectors
    only): the second and third vectors are staged over the first one's output, which stays beyond in_len and has to be read as
    zero; two passes (the default) and one (pass_log 10, copied back from the work vector)"""
    k, n = 10, 1024
    in_len = n // 2 + 1
    lib = ea.load_library()
    rng = np.random.default_rng(0x57A6E)
    with ea.Radix2EvaluationDomain(n, CURVE_OF[field]) as dom:
        for kind, pass_log in ((nc.FORWARD, 0), (nc.COSET_INVERSE, 0), (nc.FORWARD, 10)):
            dom.set_option("pass_log", pass_log)
            raw = rng.integers(0, 256, size=(3, n, 32), dtype=np.uint8)      # the call reads in_len elements of each vector
            out = np.zeros((3, n, 32), dtype=np.uint8)
            err = lib.mi355_msm_domain_transform(dom.handle, out.ctypes.data, raw.ctypes.data, in_len, 3, kind, 0, None)
            assert err.code == 0, ctypes.string_at(err.message).decode()
            for b in range(3):
                vals = nc.decode(field, raw[b, :in_len].tobytes(), False)
                assert out[b].tobytes() == nc.encode(field, nc.transform(field, k, kind, vals), False), (kind, pass_log, b)
