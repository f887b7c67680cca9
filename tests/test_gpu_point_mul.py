"""GPU: batch variable-base scalar multiplication (mi355_msm_mul_points, csrc/point_mul.hpp) through the Python layer.  Expected values
come from outside the code under test: the Python model (curve.mul), the fixed-base path (FixedBase.get_window_table(P).msm), the
engine's own MSM (linearity at size) and check_bases."""
import ctypes
import os
import random
import re
import statistics
import time

import numpy as np
import pytest

import point_mul_cases as pc
import pymodel as pm
import stream_cases as st
from conftest import ROOT

pytestmark = pytest.mark.gpu

fc = pc.fc
M256 = pc.M256


def rows(out, size):
    """images of a result (bytes, numpy or torch, any stride) as a list of `size`-byte strings"""
    if hasattr(out, "cpu"):
        out = out.cpu().numpy()
    if isinstance(out, (bytes, bytearray)):
        return [bytes(out[i:i + size]) for i in range(0, len(out), size)]
    return [bytes(r[:size]) for r in out]


def produced_on(torch, raw, stream, delay):
    """`raw` as a GPU tensor PRODUCED LATE on `stream` (tests/stream_cases.py: poison until tens of milliseconds of device work have
    passed there), so that a call that ignored the stream would read the poison instead"""
    return st.late(torch, raw, stream, delay)


@pytest.fixture(scope="module")
def delay():
    """the calibrated delay of tests/stream_cases.py, once for the module"""
    import torch

    return st.Delay(torch, torch.cuda.Stream())


def mismatches(got, want):
    return [i for i, (g, e) in enumerate(zip(got, want)) if g != e] + ([-1] if len(got) != len(want) else [])


@pytest.fixture(scope="module")
def ctxs(ea):
    """one context per curve for the whole module"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = ea.MultiScalarMultContext(name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


def pairwise_cases(name):
    """[(point, scalar, expected point)]: every base kind x the edge scalars, 50 random 256-bit scalars on the generator and on the
    point off the subgroup"""
    curve = pm.CURVES[name]
    edges = pc.pairwise_edge_scalars(curve)
    rnd = fc.random_scalars256(100, 0xB17E + curve.curve_id)
    cases = []
    for idx, (label, P, exp) in enumerate(pc.expects(name)):
        ks = edges + (rnd[:50] if idx == 0 else rnd[50:] if idx == 1 else [])
        cases += [(P, k, exp(k)) for k in ks]
    return cases


# ---- 1. bytes, small ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_pairwise_bytes_small(ea, ctxs, delay, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    cases = pairwise_cases(name)
    m = len(cases)
    pts = pc.point_images(curve, [c[0] for c in cases])
    raw = pm.encode_scalars([c[1] for c in cases])
    want_a = [curve.encode_affine(c[2]) for c in cases]
    want_p = [curve.encode_projective_normalized(c[2]) for c in cases]
    got_a = ctx.mul_points(pts, raw)
    got_p = ctx.mul_points(pts, raw, projective=True)
    assert isinstance(got_a, bytes) and len(got_a) == m * curve.affine_stride
    bad = mismatches(rows(got_a, curve.affine_stride), want_a)
    assert not bad, (name, "affine", bad[:8], [hex(cases[i][1]) for i in bad[:4]])
    bad = mismatches(rows(got_p, curve.projective_bytes), want_p)
    assert not bad, (name, "projective", bad[:8])
    # device pointers, a non-default stream, points and scalars produced on it by preceding kernels
    stream = torch.cuda.Stream()
    d_pts, d_s = st.late_many(torch, [pts, raw], stream, delay)             # (one producer in front of both)
    assert st.window_open(d_pts.produced) and st.window_open(d_s.produced)
    with torch.cuda.stream(stream):
        dev_a = ctx.mul_points(d_pts, d_s)
        dev_p = ctx.mul_points(d_pts, d_s, projective=True)
    stream.synchronize()
    assert st.closed(d_pts, d_s)
    assert dev_a.is_cuda and tuple(dev_a.shape) == (m, curve.affine_stride)
    assert dev_a.cpu().numpy().tobytes() == got_a
    assert dev_p.cpu().numpy().tobytes() == got_p
    # numpy in, numpy out; nothing in, nothing out
    arr = ctx.mul_points(np.frombuffer(pts, dtype=np.uint8), np.frombuffer(raw, dtype=np.uint8))
    assert isinstance(arr, np.ndarray) and arr.tobytes() == got_a
    assert ctx.mul_points(b"", b"") == b""
    # sizes that cross wave and block edges, built by repeating the cases from a moving start
    for n in (1, 63, 64, 65, 257):
        pick = [cases[(7 * n + i) % m] for i in range(n)]
        got = ctx.mul_points(pc.point_images(curve, [c[0] for c in pick]), pm.encode_scalars([c[1] for c in pick]))
        assert rows(got, curve.affine_stride) == [curve.encode_affine(c[2]) for c in pick], (name, n)


@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_pairwise_wave_trim(ea, ctxs, name):
    """the walk starts at the highest window that is non-zero in any lane of the wave: a wave of short scalars, a wave of 63 short
    scalars and one 256-bit scalar in lane 0 / in lane 63, a wave of zeros -- one block of four waves"""
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    kinds = pc.expects(name)[:2]                                 # the generator, a point off the subgroup
    rng = random.Random(0x7717 + curve.curve_id)
    short = [1, rng.getrandbits(17) | 1 << 16, rng.getrandbits(33) | 1 << 32, rng.getrandbits(63) | 1 << 62, rng.getrandbits(64) | 1 << 63, (1 << 64) - 1]
    long = fc.random_scalars256(100, 0xB17E + curve.curve_id)[0] | 1 << 255
    ks = [short[i % 6] for i in range(64)]
    ks += [long] + [short[i % 6] for i in range(63)]
    ks += [short[i % 6] for i in range(63)] + [long]
    ks += [0] * 64
    picks = [kinds[i % 2] for i in range(256)]
    pts = pc.point_images(curve, [p[1] for p in picks])
    want = [curve.encode_affine(p[2](k)) for p, k in zip(picks, ks)]
    for w in (0, 3, 5):
        ctx.set_option("mul_window", w)
        try:
            got = ctx.mul_points(pts, pm.encode_scalars(ks))
        finally:
            ctx.set_option("mul_window", 0)
        bad = mismatches(rows(got, curve.affine_stride), want)
        assert not bad, (name, w, bad[:8])


@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_uniform_bytes_small(ea, ctxs, delay, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    kinds = pc.expects(name)
    size = curve.affine_stride
    stream = torch.cuda.Stream()
    for k, nb in pc.uniform_edge_scalars(curve):
        for n in (1, 63, 64, 65, 257) if k == curve.r - 1 else (65,):
            pick = [kinds[(n + i) % len(kinds)] for i in range(n)]
            pts = pc.point_images(curve, [p[1] for p in pick])
            want = [p[2](k) for p in pick]
            kb = k.to_bytes(nb, "little")
            got = ctx.mul_points_by(pts, kb)
            assert rows(got, size) == [curve.encode_affine(v) for v in want], (name, hex(k), n)
            if n == 65:
                assert ctx.mul_points_by(pts, k) == got                 # an int is packed into the fewest words
                got_p = ctx.mul_points_by(pts, kb, projective=True)
                assert rows(got_p, curve.projective_bytes) == [curve.encode_projective_normalized(v) for v in want]
                d_pts = produced_on(torch, pts, stream, delay)
                assert st.window_open(d_pts.produced)
                with torch.cuda.stream(stream):
                    dev = ctx.mul_points_by(d_pts, kb)
                stream.synchronize()
                assert st.closed(d_pts)
                assert dev.is_cuda and dev.cpu().numpy().tobytes() == got
            if k == 1:
                # the canonical input images, byte for byte (a flagged infinity with junk coordinates comes back as the canonical one)
                assert rows(got, size) == [curve.encode_affine(p[1]) for p in pick]
    # the cofactor flag is the explicit k = cofactor
    h = pc.cofactor(curve)
    pts = pc.point_images(curve, [p[1] for p in kinds])
    got = ctx.mul_by_cofactor(pts)
    assert got == ctx.mul_points_by(pts, h) == pc.want_images(curve, [p[2](h) for p in kinds])
    assert ctx.mul_by_cofactor(pts, projective=True) == ctx.mul_points_by(pts, h, projective=True)
    assert ctx.mul_by_cofactor(b"") == b""
    assert ea.mul_by_cofactor(pts, curve=name) == got
    assert ea.mul_points_by(pts, 2, curve=name) == pc.want_images(curve, [p[2](2) for p in kinds])
    assert ea.mul_points(pts, pm.encode_scalars([2] * len(kinds)), curve=name) == pc.want_images(curve, [p[2](2) for p in kinds])


# ---- 2. equals the fixed-base path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_equals_fixed_base_path(ea, ctxs, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    n = 1 << 16
    rs = np.random.RandomState(16 + curve.curve_id)
    raw = rs.randint(0, 256, size=32 * n, dtype=np.uint8)       # all 256 bits in use
    d_s = torch.from_numpy(raw).cuda()
    for label, P in fc.bases(name)[:2]:                        # the generator, then the point off the subgroup
        img = fc.base_image(curve, P)
        d_pts = torch.from_numpy(np.frombuffer(img * n, dtype=np.uint8).copy()).cuda()
        with ea.FixedBase.get_window_table(img, curve=name) as table:
            want = table.msm(d_s).cpu().numpy()
            want_p = table.msm(d_s, projective=True).cpu().numpy()
        got = ctx.mul_points(d_pts, d_s).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (name, label)
        got_p = ctx.mul_points(d_pts, d_s, projective=True).cpu().numpy()
        assert np.array_equal(got_p, want_p), (name, label)


@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g1"])
def test_fr_montgomery_entry(ea, ctxs, name):
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    r = curve.r
    rng = random.Random(4 + curve.curve_id)
    rinv = pow(1 << 256, -1, r)
    ks = [rng.randrange(r) for _ in range(1000)] + [0, 1, r - 1]
    images = [k * (1 << 256) % r for k in ks]
    # non-canonical 256-bit "images": fr_from_montgomery is defined as a * 2^-256 mod r for any a
    wild = [r, r + 1, 2 * r - 1, M256, 1 << 255, (1 << 255) + 12345] + [rng.getrandbits(256) | (1 << 255) for _ in range(64)]
    pts = ea.generate_points(len(ks), distinct=len(ks), seed=44, curve=name)
    assert ctx.mul_points(pts, pm.encode_scalars(images), montgomery=True).tobytes() == ctx.mul_points(pts, pm.encode_scalars(ks)).tobytes()
    pts = pts[:len(wild)]
    got = ctx.mul_points(pts, pm.encode_scalars(wild), montgomery=True)
    assert got.tobytes() == ctx.mul_points(pts, pm.encode_scalars([a * rinv % r for a in wild])).tobytes()


# ---- 3. window and chunk independence --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_window_and_chunk_independence(ea, ctxs, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    n = 2 * 4099 + 5
    size = curve.affine_stride
    pts = ea.generate_points(n, distinct=n, seed=3, curve=name)
    rs = np.random.RandomState(3 + curve.curve_id)
    raw = rs.randint(0, 256, size=32 * n, dtype=np.uint8)
    d_pts, d_s = torch.from_numpy(pts).cuda(), torch.from_numpy(raw).cuda()
    ref = None
    try:
        for w in (0, 1, 3, 4, 5, 6):
            for chunk in (0, 4099):
                ctx.set_option("mul_window", w)
                ctx.set_option("mul_chunk", chunk)
                assert ctx.query("mul_window") == (w or 4)
                # (a window wider than the default halves the default chunk per extra bit: the work buffers stay within 2 GiB)
                assert ctx.query("mul_chunk") == (chunk or (1 << (19 if curve.ext == 1 else 18)) >> max(0, w - 4))
                got = ctx.mul_points(d_pts, d_s, out_stride=size + 16).cpu().numpy()
                assert got.shape == (n, size + 16) and not got[:, size:].any()
                if ref is None:
                    ref = got
                    head = [int.from_bytes(raw[32 * i:32 * i + 32].tobytes(), "little") for i in range(8)]
                    model = [curve.mul(k, curve.decode_affine(pts[i].tobytes())) for i, k in enumerate(head)]
                    assert rows(got[:8], size) == [curve.encode_affine(v) for v in model]
                else:
                    assert np.array_equal(got, ref), (name, w, chunk)
        # host pointers through the C ABI: the bytes between two images stay as they were
        ctx.set_option("mul_window", 0)
        out = np.full((n, size + 16), 0xA5, dtype=np.uint8)
        lib = ea.load_library()
        err = lib.mi355_msm_mul_points(ctx.context, pts.ctypes.data, n, size, raw.ctypes.data, 32, 0, out.ctypes.data, size + 16)
        assert err.code == 0
        assert np.array_equal(out[:, :size], ref[:, :size]) and (out[:, size:] == 0xA5).all()
        # the one-scalar path in chunks
        k = 0xDEADBEEFCAFEF00D1234567
        whole = ctx.mul_points_by(d_pts, k).cpu().numpy()
        ctx.set_option("mul_chunk", 0)
        assert np.array_equal(ctx.mul_points_by(d_pts, k).cpu().numpy(), whole)
        assert np.array_equal(ctx.mul_points_by(pts, k), whole)
    finally:
        ctx.set_option("mul_window", 0)
        ctx.set_option("mul_chunk", 0)
    default_chunk = 1 << (19 if curve.ext == 1 else 18)
    assert ctx.query("mul_chunk") == default_chunk and ctx.query("mul_window") == 4


# ---- 4. at size, through linearity ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g1", "bls12_381_g2"])
def test_at_size_through_linearity(ea, ctxs, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    n = (1 << 18) + 3
    r = curve.r
    assert r > 1 << 252
    rs = np.random.RandomState(180 + curve.curve_id)
    s = rs.randint(0, 1 << 63, size=(n, 4), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=(n, 4)).astype(np.uint64)
    s[:, 3] &= np.uint64((1 << 60) - 1)                        # 252-bit scalars: below r on both families
    special = rs.choice(n, size=n // 1000, replace=False)
    for t, i in enumerate(special):                            # 0 and r in turn: infinities occur
        s[i] = np.frombuffer((0, r)[t % 2].to_bytes(32, "little"), dtype=np.uint64)
    assert int((~s.any(axis=1)).sum()) == len(range(0, len(special), 2))      # no random scalar is zero
    c = rs.randint(0, 1 << 63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, size=n).astype(np.uint64)
    s_raw = s.view(np.uint8).reshape(-1)
    s_int = [int.from_bytes(s_raw[32 * i:32 * i + 32].tobytes(), "little") for i in range(n)]
    prod = np.frombuffer(b"".join((int(ci) * si % r).to_bytes(32, "little") for ci, si in zip(c, s_int)), dtype=np.uint8).copy()
    coeff = np.zeros((n, 4), dtype=np.uint64)
    coeff[:, 0] = c
    pts = ea.generate_points(n, seed=18, curve=name)
    d_pts = torch.from_numpy(pts).cuda()
    out = ctx.mul_points(d_pts, torch.from_numpy(s_raw).cuda())
    assert out.is_cuda and tuple(out.shape) == (n, curve.affine_stride)
    chk = ctx.check_bases(out)
    assert chk.ok and not chk.status.any()
    assert chk.counts["flagged_infinity"] == len(special)
    ctx.set_bases(out)
    got = ctx.run(torch.from_numpy(coeff.view(np.uint8).reshape(-1)).cuda())[0]
    ctx.set_bases(d_pts)
    want = ctx.run(torch.from_numpy(prod).cuda())[0]
    assert got == want, name


# ---- 5. cofactor clearing of decoded points ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_cofactor_clearing_of_decoded_points(ea, ctxs, name):
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    cb = curve.coord_bytes
    n = 4096
    recs = np.zeros((n, cb), dtype=np.uint8)                   # x = 1000, 1001, ... (G2: c0, with c1 = 0), no flag bits: the smaller y
    for i in range(n):
        recs[i, :8] = np.frombuffer((1000 + i).to_bytes(8, "little"), dtype=np.uint8)
    dec = ctx.decompress_points(recs)
    keep = dec.status == 0
    assert int(keep.sum()) * 3 >= n, int(keep.sum())
    pts = np.ascontiguousarray(dec.points[keep])
    m = len(pts)
    assert (ctx.check_bases(pts).status == 3).all()
    cleared = ctx.mul_by_cofactor(pts)
    chk = ctx.check_bases(cleared)
    assert chk.ok and not chk.status.any() and chk.counts["flagged_infinity"] == 0
    killed = ctx.mul_points_by(cleared, curve.r)
    assert rows(killed, curve.affine_stride) == [curve.encode_affine(None)] * m
    if curve.ext == 2:
        assert pc.cofactor(curve).bit_length() > 256            # the 64-byte scalar
    # a sample against the model
    for i in (0, m - 1):
        assert cleared[i].tobytes() == curve.encode_affine(curve.mul(pc.cofactor(curve), curve.decode_affine(pts[i].tobytes())))


# ---- 6. uniform equals pairwise ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_uniform_equals_pairwise(ea, ctxs, name):
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    n = 1000
    k = random.Random(0x6006 + curve.curve_id).getrandbits(256) | 1 << 255
    kinds = [fc.base_image(curve, P) for _, P in fc.bases(name)]
    gen = ea.generate_points(n, distinct=n, seed=6, curve=name)
    pts = b"".join(kinds[i % len(kinds)] if i % 3 == 0 else gen[i].tobytes() for i in range(n))
    assert ctx.mul_points_by(pts, k) == ctx.mul_points(pts, pm.encode_scalars([k] * n))
    assert ctx.mul_points_by(pts, k, projective=True) == ctx.mul_points(pts, pm.encode_scalars([k] * n), projective=True)


# ---- 7. errors and lifetime -----------------------------------------------------------------------------------------------

def test_errors_and_lifetime(ea):
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    lib = ea.load_library()
    n = 100
    pts = ea.generate_points(n, distinct=n, seed=7, curve=name)
    raw = pm.encode_scalars(fc.random_scalars256(n, 7))
    warm = ea.MultiScalarMultContext(name)                      # code objects, streams: what a first call leaves behind
    warm.mul_points(pts, raw)
    warm.close()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    ctx = ea.MultiScalarMultContext(name)
    big = ea.generate_points(1 << 16, seed=7, curve=name)
    ctx.mul_points(big, np.zeros(32 << 16, dtype=np.uint8))
    work = ctx.query("mul_work_bytes")
    assert work >= (8 << 16) * (224 + 128 + 56)
    assert torch.cuda.mem_get_info()[0] <= free_before - work // 2
    good = ctx.mul_points(pts, raw)
    pbuf = ctypes.create_string_buffer(pts.tobytes(), n * 104)
    sbuf = ctypes.create_string_buffer(raw, len(raw))
    out = ctypes.create_string_buffer(144 * n)
    k8 = ctypes.create_string_buffer(8)
    P, S, O = ctypes.addressof(pbuf), ctypes.addressof(sbuf), ctypes.addressof(out)
    K = ctypes.addressof(k8)
    bad_calls = [
        (None, n, 104, S, 32, 0, O, 104), (P, n, 104, None, 32, 0, O, 104), (P, n, 104, S, 32, 0, None, 104),      # null pointers
        (P, n, 96, S, 32, 0, O, 104), (P, n, 106, S, 32, 0, O, 104),                                            # input stride
        (P, n, 104, S, 32, 0, O, 100), (P, n, 104, S, 32, 0, O, 106), (P, n, 104, S, 32, 2, O, 104),            # output stride
        (P, n, 104, S, 16, 0, O, 104), (P, n, 104, S, 64, 0, O, 104), (P, n, 104, S, 0, 0, O, 104),             # pairwise scalars are 32 bytes
        (P, n, 104, K, 0, 4, O, 104), (P, n, 104, K, 6, 4, O, 104), (P, n, 104, K, 68, 4, O, 104), (P, n, 104, None, 8, 4, O, 104),
        (P, n, 104, K, 8, 8, O, 104), (P, n, 104, None, 8, 8, O, 104), (P, n, 104, K, 0, 12, O, 104),           # the cofactor takes no scalar
        (P, n, 104, S, 32, 16, O, 104), (P, n, 104, S, 32, 0x80000000, O, 104),                                 # unknown bits
        (P, n, 104, K, 8, 5, O, 104), (P, n, 104, None, 0, 9, O, 104),                                          # bit 0 with bit 2 / 3
    ]
    for args in bad_calls:
        for fn, extra in ((lib.mi355_msm_mul_points, ()), (lib.mi355_msm_mul_points_device, (None,))):
            err = fn(ctx.context, *args, *extra)
            assert err.code == -1 and err.message and ctypes.string_at(err.message), args
            ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
    err = lib.mi355_msm_mul_points(None, P, n, 104, S, 32, 0, O, 104)
    assert err.code == -1 and err.message
    ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
    with pytest.raises(ValueError):
        ctx.mul_points(pts, raw[:-32])
    with pytest.raises(ValueError):
        ctx.mul_points(pts, raw, out_stride=102)
    with pytest.raises(ValueError):
        ctx.mul_points_by(pts, b"\x01\x02\x03")
    with pytest.raises(ValueError):
        ctx.mul_points_by(pts, 1 << 512)
    for key, value in (("mul_window", 7), ("mul_window", -1), ("mul_chunk", -1)):
        with pytest.raises(ea.MsmError):
            ctx.set_option(key, value)
    # npoints = 0 succeeds and writes nothing
    err = lib.mi355_msm_mul_points(ctx.context, None, 0, 104, None, 32, 0, None, 104)
    assert err.code == 0
    # a sharded context refuses, with a message
    sharded = ea.MultiScalarMultContext(name, devices=[0, 0])
    try:
        with pytest.raises(ea.MsmError) as ei:
            sharded.mul_points(pts, raw)
        assert ei.value.code == -1 and "sharded" in ei.value.message
        with pytest.raises(ea.MsmError):
            sharded.mul_by_cofactor(pts)
    finally:
        sharded.close()
    assert np.array_equal(ctx.mul_points(pts, raw), good)       # the context still works, and gives the same bytes
    assert ctx.query("last_mul_us") > 0 and ctx.query("last_mul_device_us") > 0
    ctx.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free_before - work // 4


# ---- 8. speed guard ------------------------------------------------------------------------------------------------------------

MODELLED_PAIRWISE = 3088 / 3616     # field products: w = 4 path / [r]P by double-and-add (254 dbl x 9 + 133 madd x 10)
MODELLED_UNIFORM = 1.0              # 254 dbl + about 85 madd against 254 dbl + 133 madd, both one rolled loop


def speed_bounds():
    """(pairwise bound, uniform bound, source): 1.5 x the ratios profiles/point_mul.txt measured on BLS12-381 G1 at 2^20 points (the
    margin covers box-to-box spread and clock differences under power limits), or 2 x the modelled ratios when there is no such file"""
    path = os.path.join(ROOT, "profiles", "point_mul.txt")
    if os.path.exists(path):
        txt = open(path).read()
        mp = re.search(r"^bls12_381_g1 ratio pairwise w=4 / check_bases\(exact\): ([0-9.]+)", txt, flags=re.M)
        mu = re.search(r"^bls12_381_g1 ratio uniform k=r / check_bases\(exact\): ([0-9.]+)", txt, flags=re.M)
        if mp and mu:
            return 1.5 * float(mp.group(1)), 1.5 * float(mu.group(1)), "profiles/point_mul.txt"
    return 2 * MODELLED_PAIRWISE, 2 * MODELLED_UNIFORM, "model"


def test_speed_guard_against_check_bases_exact(ea):
    """BLS12-381 G1, 2^20 device-resident points, warmed up, median of 5, host clock: pairwise mul_points (w = 4: 256 doublings + 65
    mixed additions + the table of 7 mixed additions and 8 normalised records) and mul_points_by(r) (254 doublings + the additions of
    r's non-adjacent form) against check_bases(exact=True) on the same points (254 doublings + 133 mixed additions).
    Modelled ratios of field products: 3088 / 3616 = 0.85 and about 1.0.  Bound: 1.5 x the ratio profiles/point_mul.txt measured with
    tools/point_mul_bench.py (the `ratio` lines of BLS12-381 G1; this test reads them): measured 0.986 and 0.826, so the bounds are
    1.48 (pairwise) and 1.24 (uniform), DESIGN 4d.  Without that file: 2 x the modelled ratio, 1.70 and 2.0.  The bounds never
    come from this test's own timing of the code under test."""
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    n = 1 << 20
    bound_p, bound_u, source = speed_bounds()
    d_pts = torch.from_numpy(ea.generate_points(n, seed=8, curve=name)).cuda()
    rs = np.random.RandomState(8)
    d_s = torch.from_numpy(rs.randint(0, 256, size=32 * n, dtype=np.uint8)).cuda()
    out = torch.zeros((n, curve.affine_stride), dtype=torch.uint8, device="cuda")
    lib = ea.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    rbytes = ctypes.create_string_buffer(curve.r.to_bytes(32, "little"), 32)
    ctx = ea.MultiScalarMultContext(name)
    try:
        def timed(call):
            def once():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                return time.perf_counter() - t0
            once()
            return statistics.median(once() for _ in range(5))

        def pairwise():
            err = lib.mi355_msm_mul_points_device(ctx.context, d_pts.data_ptr(), n, curve.affine_stride, d_s.data_ptr(), 32, 0, out.data_ptr(),
                                                  curve.affine_stride, stream)
            assert err.code == 0

        def uniform():
            err = lib.mi355_msm_mul_points_device(ctx.context, d_pts.data_ptr(), n, curve.affine_stride, ctypes.addressof(rbytes), 32, 4, out.data_ptr(),
                                                  curve.affine_stride, stream)
            assert err.code == 0

        t_check = timed(lambda: ctx.check_bases(d_pts, exact=True))
        t_pair = timed(pairwise)
        t_uni = timed(uniform)
    finally:
        ctx.close()
    print("2^20 points: check_bases(exact) %.2f ms; pairwise %.2f ms (ratio %.3f, bound %.3f); uniform k = r %.2f ms (ratio %.3f, bound %.3f); bounds from %s"
          % (t_check * 1e3, t_pair * 1e3, t_pair / t_check, bound_p, t_uni * 1e3, t_uni / t_check, bound_u, source))
    assert t_pair <= bound_p * t_check, (t_pair, t_check, source)
    assert t_uni <= bound_u * t_check, (t_uni, t_check, source)
