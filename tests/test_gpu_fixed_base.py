"""GPU: batch fixed-base multiplication (mi355_msm_fixed_*, csrc/fixed_base.hpp) through the Python layer.  Expected values come
from outside the code under test: the CPU oracle (one-pair MSMs: k * g for canonical k), the Python model (scalars at or above 2^255,
which the oracle's 255-bit window rule does not read), the engine's own MSM (linearity at size, one-pair runs)."""
import ctypes
import random
import statistics
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fixed_base_cases as fc
import pymodel as pm
import stream_cases as st

pytestmark = pytest.mark.gpu

M256 = fc.M256


def scalars_bytes(ks):
    return pm.encode_scalars(ks)


def oracle_mul(oracle, curve, img, ks):
    """[k * g as a normalised Projective image] by one-pair oracle MSMs (7 - 30 ms each; the calls release the GIL)."""
    def one(k):
        out = ctypes.create_string_buffer(curve.projective_bytes)
        b = ctypes.create_string_buffer(img, len(img))
        s = ctypes.create_string_buffer(int(k).to_bytes(32, "little"), 32)
        assert oracle.oracle_msm(curve.curve_id, b, curve.affine_stride, s, 1, out, 1) == 0
        return out.raw
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, ks))


def affine_of_projective(curve, img):
    """normalised Projective image -> Affine image: the same coordinate bytes; (1, 1, 0) -> zeros with the flag set"""
    cb = curve.coord_bytes
    if img[2 * cb:] == bytes(cb):
        return bytes(2 * cb) + b"\x01" + bytes(7)
    return img[:2 * cb] + bytes(8)


def rows(out, size):
    """images of a result (bytes, numpy or torch, any stride) as a list of `size`-byte strings"""
    if hasattr(out, "cpu"):
        out = out.cpu().numpy()
    if isinstance(out, (bytes, bytearray)):
        return [bytes(out[i:i + size]) for i in range(0, len(out), size)]
    return [bytes(r[:size]) for r in out]


def device_scalars(torch, raw, stream, delay):
    """the scalars as a GPU tensor PRODUCED LATE on `stream` (tests/stream_cases.py: poison until tens of milliseconds of device work
    have passed there), so that a call that ignored the stream would read the poison instead"""
    return st.late(torch, raw, stream, delay)


@pytest.fixture(scope="module")
def delay():
    """the calibrated delay of tests/stream_cases.py, once for the module"""
    import torch

    return st.Delay(torch, torch.cuda.Stream())


# ---- 1. bytes, small ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fc.CURVE_NAMES)
def test_bytes_small(ea, oracle, delay, name):
    import torch

    curve = pm.CURVES[name]
    rng = random.Random(0x51AB + curve.curve_id)
    canon = [rng.randrange(curve.r) for _ in range(2000)]
    big = [rng.getrandbits(255) | (1 << 255) for _ in range(32)]
    stream = torch.cuda.Stream()
    for label, P in fc.bases(name):
        img = fc.base_image(curve, P)
        exp = fc.Expect(curve, P)
        with ea.FixedBase.get_window_table(img, curve=name) as table:
            w = table.query("window_bits")
            edge = list(dict.fromkeys(fc.edge_scalars(curve, w)))
            ks = canon + edge + big
            want_p = oracle_mul(oracle, curve, img, canon) + [curve.encode_projective_normalized(exp(k)) for k in edge + big]
            want_a = [affine_of_projective(curve, p) for p in want_p]
            assert want_a[2000:] == [curve.encode_affine(exp(k)) for k in edge + big]
            raw = scalars_bytes(ks)
            got_a = table.msm(raw)
            got_p = table.msm(raw, projective=True)
            assert isinstance(got_a, bytes) and len(got_a) == len(ks) * curve.affine_stride
            bad = [i for i, (g, e) in enumerate(zip(rows(got_a, curve.affine_stride), want_a)) if g != e]
            assert not bad, (name, label, "affine", bad[:8], [hex(ks[i]) for i in bad[:4]])
            bad = [i for i, (g, e) in enumerate(zip(rows(got_p, curve.projective_bytes), want_p)) if g != e]
            assert not bad, (name, label, "projective", bad[:8])
            # device pointers, a non-default stream, the scalars produced on it by a preceding kernel
            d = device_scalars(torch, raw, stream, delay)
            assert st.window_open(d.produced)
            with torch.cuda.stream(stream):
                dev_a = table.msm(d)
                dev_p = table.msm(d, projective=True)
            stream.synchronize()
            assert st.closed(d)
            assert dev_a.is_cuda and tuple(dev_a.shape) == (len(ks), curve.affine_stride)
            assert dev_a.cpu().numpy().tobytes() == got_a
            assert dev_p.cpu().numpy().tobytes() == got_p
            # numpy in, numpy out
            arr = table.msm(np.frombuffer(raw, dtype=np.uint8))
            assert isinstance(arr, np.ndarray) and arr.tobytes() == got_a
            assert table.msm(b"") == b""


# ---- 2. window and chunk independence --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g1"])
def test_window_and_chunk_independence(ea, oracle, name):
    import torch

    curve = pm.CURVES[name]
    n = (1 << 18) + 3
    Q = dict(fc.bases(name))["off the subgroup"]
    img = fc.base_image(curve, Q)
    rs = np.random.RandomState(18 + curve.curve_id)
    raw = rs.randint(0, 256, size=32 * n, dtype=np.uint8)      # all 256 bits in use
    d = torch.from_numpy(raw).cuda()
    ref = None
    for w in (0, 16, 11, 5, 1):
        with ea.FixedBase.get_window_table(img, curve=name, window=w) as table:
            assert w == 0 or table.query("window_bits") == w
            assert table.query("levels") == (256 + table.query("window_bits") - 1) // table.query("window_bits")
            got = table.msm(d).cpu().numpy()
            if ref is None:
                ref = got
                head = [int.from_bytes(raw[32 * i:32 * i + 32].tobytes(), "little") for i in range(8)]
                exp = fc.Expect(curve, Q)
                assert rows(got[:8], curve.affine_stride) == [curve.encode_affine(exp(k)) for k in head]
                # a small chunk cap and a wider stride change nothing but the stride
                table.set_option("max_chunk", 4099)
                chunked = table.msm(d, stride=120).cpu().numpy()
                assert chunked.shape == (n, 120)
                assert np.array_equal(chunked[:, :curve.affine_stride], ref) and not chunked[:, curve.affine_stride:].any()
                host = table.msm(raw, stride=120)
                assert np.array_equal(host, chunked)
                table.set_option("max_chunk", 0)
                assert table.query("max_chunk") == 1 << 22
            else:
                assert np.array_equal(got, ref), (name, w)


# ---- 3. bytes at size, through linearity --------------------------------------------------------------------------------------

def weighted_sum(c, s_words):
    """sum c_i * s_i for c (n,) uint64 and s (n, 4) uint64 little-endian words, exactly: 16-bit pieces, int64 dot products whose
    partial sums stay below 2^32 * 2^20 per block"""
    total = 0
    n = len(c)
    for lo in range(0, n, 1 << 20):
        c16 = c[lo:lo + (1 << 20)].view(np.uint16).reshape(-1, 4).astype(np.int64)
        s16 = s_words[lo:lo + (1 << 20)].view(np.uint16).reshape(-1, 16).astype(np.int64)
        m = c16.T @ s16
        for a in range(4):
            for b in range(16):
                total += int(m[a, b]) << (16 * (a + b))
    return total


@pytest.mark.parametrize("name,logn", [("bls12_377_g1", 22), ("bls12_381_g1", 22), ("bls12_377_g2", 22), ("bls12_381_g2", 22), ("bls12_377_g1", 24)])
def test_bytes_at_size_through_linearity(ea, oracle, name, logn):
    import torch

    curve = pm.CURVES[name]
    n = 1 << logn
    r = curve.r
    g = curve.generator()
    img = fc.base_image(curve, g)
    rs = np.random.RandomState(logn * 10 + curve.curve_id)
    s = rs.randint(0, 1 << 63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=(n, 4)).astype(np.uint64)
    s[:, 3] &= np.uint64((1 << 60) - 1)                        # 252-bit scalars: below r on both families
    assert r > 1 << 252
    special = rs.choice(n, size=n // 1000, replace=False)
    for t, i in enumerate(special):                            # 0, r, 2r in turn: multiples of r, so infinities occur
        v = (0, r, 2 * r)[t % 3]
        assert v < 1 << 256
        s[i] = np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64)
    assert int((~s.any(axis=1)).sum()) == len(range(0, len(special), 3))      # no random scalar is zero
    c = rs.randint(0, 1 << 63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=n).astype(np.uint64)
    total = weighted_sum(c, s) % r
    assert weighted_sum(c[:1000], s[:1000]) == sum(int(ci) * int.from_bytes(si.tobytes(), "little") for ci, si in zip(c[:1000], s[:1000]))
    want = oracle_mul(oracle, curve, img, [total])[0]

    d_s = torch.from_numpy(s.view(np.uint8).reshape(-1)).cuda()
    coeff = np.zeros((n, 4), dtype=np.uint64)
    coeff[:, 0] = c
    d_c = torch.from_numpy(coeff.view(np.uint8).reshape(-1)).cuda()
    with ea.FixedBase.get_window_table(img, curve=name, expected_scalars=n) as table:
        out = table.msm(d_s)                                    # Affine images, still on the device
    assert out.is_cuda and tuple(out.shape) == (n, curve.affine_stride)
    ctx = ea.MultiScalarMultContext(name)
    try:
        chk = ctx.check_bases(out)
        assert chk.ok and not chk.status.any()
        assert chk.counts["flagged_infinity"] == len(special)
        ctx.set_bases(out)
        got = ctx.run(d_c)[0]
    finally:
        ctx.close()
    assert got == want, (name, logn)


# ---- 4. the Fr entry -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g1"])
def test_fr_montgomery_entry(ea, name):
    curve = pm.CURVES[name]
    r = curve.r
    rng = random.Random(4 + curve.curve_id)
    rinv = pow(1 << 256, -1, r)
    ks = [rng.randrange(r) for _ in range(1000)] + [0, 1, r - 1]
    images = [k * (1 << 256) % r for k in ks]
    # non-canonical 256-bit "images": fr_from_montgomery is defined as a * 2^-256 mod r for any a
    wild = [r, r + 1, 2 * r - 1, M256, 1 << 255, (1 << 255) + 12345] + [rng.getrandbits(256) | (1 << 255) for _ in range(64)]
    with ea.FixedBase.get_window_table(fc.base_image(curve, curve.generator()), curve=name) as table:
        assert table.msm(scalars_bytes(images), montgomery=True) == table.msm(scalars_bytes(ks))
        assert table.msm(scalars_bytes(wild), montgomery=True) == table.msm(scalars_bytes([a * rinv % r for a in wild]))
        # arkworks' shape: Fr images in, Projective images out
        assert ea.FixedBase.msm(table, scalars_bytes(images[:50])) == table.msm(scalars_bytes(ks[:50]), projective=True)
    assert ea.fixed_base_msm(fc.base_image(curve, curve.generator()), scalars_bytes([5]), curve=name) == curve.encode_affine(
        curve.mul(5, curve.generator()))


# ---- 5. the same as the engine -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", fc.CURVE_NAMES)
def test_projective_output_equals_one_pair_msms(ea, name):
    curve = pm.CURVES[name]
    rng = random.Random(55 + curve.curve_id)
    ks = [rng.randrange(curve.r) for _ in range(500 - 12)] + fc.edge_scalars(curve, 16)
    assert len(ks) == 500
    raw = scalars_bytes(ks)
    pb = curve.projective_bytes
    for label, P in fc.bases(name)[:2]:                        # the generator and a point off the subgroup
        img = fc.base_image(curve, P)
        ctx = ea.MultiScalarMultContext(name)
        try:
            ctx.set_bases(img)
            want = ctx.run(raw, npoints=1)                      # 500 batches of one pair
        finally:
            ctx.close()
        with ea.FixedBase.get_window_table(img, curve=name) as table:
            got = table.msm(raw, projective=True)
        assert rows(got, pb) == want, (name, label)


# ---- 6. errors and lifetime -----------------------------------------------------------------------------------------------

def test_errors_and_lifetime(ea):
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    img = fc.base_image(curve, curve.generator())
    lib = ea.load_library()
    raw = scalars_bytes(fc.random_scalars256(100, 6))
    with pytest.raises(ValueError):
        ea.FixedBase.get_window_table(img[:-1], curve=name)
    with pytest.raises(ValueError):
        ea.FixedBase.get_window_table(img + bytes(96), curve=name)
    with ea.FixedBase.get_window_table(img, curve=name, window=4) as warm:      # code objects, streams: what a first call leaves behind
        warm.msm(raw)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    table = ea.FixedBase.get_window_table(img, curve=name, window=16)
    table_bytes = table.query("table_bytes")
    assert table_bytes >= (16 << 16) * 128 and table.query("signed_digits") == 0 and table.query("build_us") > 0
    assert torch.cuda.mem_get_info()[0] <= free_before - table_bytes // 2
    good = table.msm(raw)
    with pytest.raises(ValueError):
        table.msm(raw[:-1])
    with pytest.raises(ValueError):
        table.msm(raw, stride=102)
    out = ctypes.create_string_buffer(104 * 100)
    buf = ctypes.create_string_buffer(raw, len(raw))
    for args in ((out, 100, buf, 100, 0), (out, 106, buf, 100, 0), (out, 104, buf, 100, 4), (out, 104, buf, 100, 0x80000000), (None, 104, buf, 100, 0),
                 (out, 104, None, 100, 0), (out, 104, buf, 100, 2)):      # (the last: a Projective image does not fit a 104-byte stride)
        err = lib.mi355_msm_fixed_mul(table.handle, *args)
        assert err.code == -1 and err.message and ctypes.string_at(err.message)
        ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
    with pytest.raises(ea.MsmError):
        table.query("no_such_key")
    assert table.msm(raw) == good                               # the handle still works, and gives the same bytes
    assert table.query("last_mul_us") > 0
    table.close()
    table.close()
    with pytest.raises(ea.MsmError):
        table.msm(raw)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free_before - table_bytes // 4
    for bad_w in (-1, 21):
        h = ctypes.c_void_p()
        err = lib.mi355_msm_fixed_create(ctypes.byref(h), curve.curve_id, -1, img, bad_w, 0)
        assert err.code == -1 and not h.value
        ctypes.CDLL(None).free(ctypes.c_void_p(err.message))


def test_auto_window_rule(ea):
    """what a handle chooses: the cheapest of levels(w) * (2 * 2^w + n) with the table inside the Infinity Cache"""
    for name, cap in (("bls12_381_g1", 16), ("bls12_381_g2", 15)):
        curve = pm.CURVES[name]
        img = fc.base_image(curve, curve.generator())
        for n in (0, 1, 1 << 10, 1 << 24):
            best = cap if n == 0 else min(range(1, cap + 1), key=lambda w: ((256 + w - 1) // w) * (2 * (1 << w) + n))
            with ea.FixedBase.get_window_table(img, curve=name, expected_scalars=n) as table:
                assert table.query("window_bits") == best, (name, n)


# ---- 7. speed guard ------------------------------------------------------------------------------------------------------------

def test_speed_guard_against_the_msm_of_equal_size(ea):
    """BLS12-381 G1, n = 2^24, device scalars, warmed up, median of 5: one fixed-base call (table built, Affine output) against one
    MSM over 2^24 resident bases (context defaults, no tables).  Derived bound: 16 additions + normalisation per output against
    about 13 per pair is 1.3x; an un-overlapped one-lane gather costs about as much again as the additions: 2.6x.  Asserted: 3.0x."""
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    n = 1 << 24
    rs = np.random.RandomState(7)
    s = rs.randint(0, 1 << 63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=(n, 4)).astype(np.uint64)
    s[:, 3] &= np.uint64((1 << 60) - 1)
    d_s = torch.from_numpy(s.view(np.uint8).reshape(-1)).cuda()
    lib = ea.load_library()

    table = ea.FixedBase.get_window_table(fc.base_image(curve, curve.generator()), curve=name, expected_scalars=n)
    out = torch.zeros((n, curve.affine_stride), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def fixed_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        err = lib.mi355_msm_fixed_mul_device(table.handle, out.data_ptr(), curve.affine_stride, d_s.data_ptr(), n, 0, stream)
        assert err.code == 0
        return time.perf_counter() - t0

    fixed_once()
    t_fixed = statistics.median(fixed_once() for _ in range(5))
    w = table.query("window_bits")
    table.close()
    del out

    ctx = ea.MultiScalarMultContext(name)
    try:
        ctx.set_bases(ea.generate_points(n, curve=name))

        def msm_once():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.run(d_s)
            return time.perf_counter() - t0

        msm_once()
        t_msm = statistics.median(msm_once() for _ in range(5))
    finally:
        ctx.close()
    print("fixed-base 2^24 (w = %d): %.2f ms;  MSM 2^24: %.2f ms;  ratio %.2f" % (w, t_fixed * 1e3, t_msm * 1e3, t_fixed / t_msm))
    assert t_fixed <= 3.0 * t_msm, (t_fixed, t_msm)
