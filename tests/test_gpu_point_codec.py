"""GPU: arkworks compressed records on the device -- mi355_msm_decompress_points / _compress_points / _set_bases_compressed /
_point_to_compressed (k_decompress_points, k_compress_points) against the Python model of tests/codec_cases.py and against the host
build of the same templates; the element-wise square roots of libmsm_devtest.so; and a speed guard against check_bases."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import codec_cases as kc
import pymodel as pm
from conftest import ROOT
from test_point_codec_host import sqrt_inputs

pytestmark = pytest.mark.gpu

NL = 14
R392 = 1 << 392
DT_SQRT, DT_SQRT2, DT_LEX_LARGEST = 23, 24, 25


_libc = ctypes.CDLL(None)
_libc.free.argtypes = [ctypes.c_void_p]
_free = _libc.free


def _torch():
    import torch

    return torch


def _cuda(b):
    torch = _torch()
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_decompress_points.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.ht_compress_points.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    lib.ht_devop.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.ht_devop_shape.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return lib


def host_decompress(ht, curve, records, serialized):
    n = len(records) // curve.coord_bytes
    stride = 2 * curve.coord_bytes if serialized else curve.affine_stride
    out = ctypes.create_string_buffer(max(n * stride, 1))
    status = ctypes.create_string_buffer(max(n, 1))
    assert ht.ht_decompress_points(curve.curve_id, int(serialized), records, n, out, stride, status) == 0
    return list(status.raw[:n]), out.raw[:n * stride]


def _bytes(x):
    if hasattr(x, "is_cuda"):
        return x.cpu().numpy().tobytes()
    return x if isinstance(x, bytes) else np.asarray(x).tobytes()


def _summary(statuses, records):
    n = len(statuses)
    first = next((i for i, s in enumerate(statuses) if s), None)
    flagged = sum(1 for s, r in zip(statuses, records) if s == 0 and (r[-1] >> 6) == 1)
    return {"valid": statuses.count(0), "flagged_infinity": flagged, "malformed": statuses.count(1), "no_point": statuses.count(2),
            "off_subgroup": statuses.count(3)}, first


def _expect_decode(res, curve, records, statuses, serialized, want_bytes):
    counts, first = _summary(list(statuses), records)
    assert list(res.status) == list(statuses)
    assert res.counts == counts and res.first_invalid == first and res.ok == (first is None)
    assert _bytes(res.points) == want_bytes


def _fixture(name):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "compressed", name + ".json")))
    return [bytes.fromhex(r) for r in doc["records"]], doc["status"], b"".join(bytes.fromhex(u) for u in doc["uncompressed"])


@pytest.mark.parametrize("serialized", [False, True], ids=["images", "uncompressed"])
@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_corpus_and_fixture_through_the_abi(ea, ht, name, serialized):
    curve = pm.CURVES[name]
    recs, statuses, labels, _ = kc.corpus(name)
    frecs, fstatus, func = _fixture(name)
    ctx = ea.MultiScalarMultContext(name)
    try:
        for rr, st in ((list(recs), list(statuses)), (frecs, fstatus)):
            data = b"".join(rr)
            want_st, want = kc.expected(curve, data, serialized)
            assert want_st == st
            h_st, h_bytes = host_decompress(ht, curve, data, serialized)
            assert h_st == st and h_bytes == want                                   # model == host build ...
            host = ctx.decompress_points(data, uncompressed=serialized)
            _expect_decode(host, curve, rr, st, serialized, want)                   # ... == the engine, host input
            dev = ctx.decompress_points(_cuda(data), uncompressed=serialized)
            assert dev.points.is_cuda
            _expect_decode(dev, curve, rr, st, serialized, want)                    # ... == the engine, device input and output
            # compression of what decoded returns the original bytes (records that failed decoded to zeros: left out; y = 0: bit 7 clear)
            stride = len(want) // len(rr)
            keep = [i for i, s in enumerate(st) if s == 0 and not (rr[i][-1] & 0x40)]
            pts = b"".join(want[i * stride:(i + 1) * stride] for i in keep)
            orig = b"".join(rr[i] if kc.decode(curve, rr[i])[1][1] != (0,) * curve.ext else rr[i][:-1] + bytes([rr[i][-1] & 0x3f]) for i in keep)
            for arg in (pts, _cuda(pts)):
                c = ctx.compress_points(arg, serialized=serialized)
                assert c.ok and list(c.status) == [0] * len(keep) and _bytes(c.points) == orig
        if serialized:
            assert _bytes(ctx.decompress_points(b"".join(frecs), uncompressed=True).points) == func
        # status = NULL, and n = 0
        data = b"".join(recs)
        stride = 2 * curve.coord_bytes if serialized else curve.affine_stride
        out8 = (ctypes.c_uint64 * 8)()
        buf = ctypes.create_string_buffer(len(recs) * stride)
        e = ctx._lib.mi355_msm_decompress_points(ctx.context, data, len(recs), buf, stride, 1 if serialized else 0, None, out8)
        counts, first = _summary(list(statuses), recs)
        assert e.code == 0 and buf.raw == kc.expected(curve, data, serialized)[1]
        assert list(out8)[:6] == [counts["valid"], counts["flagged_infinity"], counts["malformed"], counts["no_point"], 0, first]
        empty = ctx.decompress_points(b"", uncompressed=serialized)
        assert empty.ok and empty.first_invalid is None and len(empty.status) == 0 and not any(empty.counts.values()) and _bytes(empty.points) == b""
        cempty = ctx.compress_points(b"", serialized=serialized)
        assert cempty.ok and len(cempty.status) == 0 and _bytes(cempty.points) == b""
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_placement(ea, ht, name, n):
    """Failing records at index 0, 63, 64, 255, 256 and n - 1; the engine's bytes equal the model's and libmsm_hosttest.so's."""
    curve = pm.CURVES[name]
    recs, statuses = kc.placed(name, n, seed=5)
    data = b"".join(recs)
    ctx = ea.MultiScalarMultContext(name)
    try:
        for serialized in (False, True):
            want_st, want = kc.expected(curve, data, serialized)
            assert want_st == statuses
            # (the host build decodes each distinct record once: its per-record function does not know positions)
            uniq = sorted(set(recs))
            u_st, u_bytes = host_decompress(ht, curve, b"".join(uniq), serialized)
            rb = len(want) // n
            at = {r: i for i, r in enumerate(uniq)}
            assert [u_st[at[r]] for r in recs] == statuses and b"".join(u_bytes[at[r] * rb:(at[r] + 1) * rb] for r in recs) == want
            _expect_decode(ctx.decompress_points(data, uncompressed=serialized), curve, recs, statuses, serialized, want)
            _expect_decode(ctx.decompress_points(_cuda(data), uncompressed=serialized), curve, recs, statuses, serialized, want)
    finally:
        ctx.close()
    assert statuses[0] != 0 and statuses[n - 1] != 0


@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_chunk_seams(ea, name):
    """codec_chunk = 256 with n = 513: three launches, the bytes of the one-chunk run."""
    curve = pm.CURVES[name]
    recs, statuses = kc.placed(name, 513, seed=9)
    data = b"".join(recs)
    ctx = ea.MultiScalarMultContext(name)
    try:
        assert ctx.query("codec_chunk") == 1 << 22
        one = {}
        for form in ("host", "device"):
            arg = data if form == "host" else _cuda(data)
            for serialized in (False, True):
                r = ctx.decompress_points(arg, uncompressed=serialized, validate=True)
                one[form, serialized] = (_bytes(r.points), bytes(r.status), r.counts, r.first_invalid)
                assert one[form, serialized][0] == kc.expected(curve, data, serialized)[1]
        ctx.set_option("codec_chunk", 256)
        assert ctx.query("codec_chunk") == 256
        for form in ("host", "device"):
            arg = data if form == "host" else _cuda(data)
            for serialized in (False, True):
                r = ctx.decompress_points(arg, uncompressed=serialized, validate=True)
                assert (_bytes(r.points), bytes(r.status), r.counts, r.first_invalid) == one[form, serialized]
                good = ctx.decompress_points(arg, uncompressed=serialized)
                c = ctx.compress_points(good.points, serialized=serialized)
                ctx.set_option("codec_chunk", 0)
                c1 = ctx.compress_points(good.points, serialized=serialized)
                ctx.set_option("codec_chunk", 256)
                assert _bytes(c.points) == _bytes(c1.points) and bytes(c.status) == bytes(c1.status)
        with pytest.raises(ea.MsmError):
            ctx.set_option("codec_chunk", -1)
    finally:
        ctx.close()


@pytest.mark.parametrize("exact", [False, True], ids=["endomorphism", "exact"])
@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_validate(ea, name, exact):
    """validate=True: the off-subgroup corpus points get status 3 with either method; a record that failed to decode keeps 1 / 2."""
    curve = pm.CURVES[name]
    recs, statuses, labels, sub = kc.corpus(name)
    want = [3 if (s == 0 and not g) else s for s, g in zip(statuses, sub)]
    assert want.count(3) >= 10 and want.count(1) >= 4 and want.count(2) >= 6
    data = b"".join(recs)
    ctx = ea.MultiScalarMultContext(name)
    try:
        for serialized in (False, True):
            for arg in (data, _cuda(data)):
                r = ctx.decompress_points(arg, uncompressed=serialized, validate=True, exact=exact)
                assert list(r.status) == want, [(l, a, b) for l, a, b in zip(labels, r.status, want) if a != b]
                assert r.counts["off_subgroup"] == want.count(3) and r.counts["valid"] == want.count(0)
                assert r.method == ("exact" if exact else "endomorphism")
                assert _bytes(r.points) == kc.expected(curve, data, serialized)[1]      # validation does not change what is written
    finally:
        ctx.close()


# ---- element-wise: libmsm_devtest.so against the host build ----------------------------------------------------------------------
def _limbs(v):
    return [(v >> (28 * i)) & 0x0fffffff for i in range(NL - 1)] + [v >> (28 * (NL - 1))]


@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_device_square_roots_equal_the_host_build(ht, name):
    curve = pm.CURVES[name]
    p = curve.p
    dev = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_devtest.so"))
    dev.msm_devtest_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    dev.msm_devtest_shape.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    ins = sqrt_inputs(curve)
    rng = random.Random(3)
    recs = [sum((_limbs(c * R392 % p) for c in a), []) for _, a in ins]
    recs += [sum((_limbs(c * R392 % p + p) for c in a), []) for _, a in ins if all((c * R392 % p) * 2 < p for c in a)][:64]   # the upper class-M representative
    ew = NL * curve.ext
    ops = [(DT_SQRT2 if curve.ext == 2 else DT_SQRT, ew), (DT_LEX_LARGEST, ew)]
    if curve.ext == 2:
        ops.append((DT_SQRT, NL))
    for op, words in ops:
        a = np.ascontiguousarray(np.array([r[:words] for r in recs], dtype=np.uint32))
        iw, ow = ctypes.c_int(), ctypes.c_int()
        assert ht.ht_devop_shape(curve.curve_id, op, ctypes.byref(iw), ctypes.byref(ow)) == 0 and iw.value == words
        di, do = ctypes.c_int(), ctypes.c_int()
        assert dev.msm_devtest_shape(curve.curve_id, op, ctypes.byref(di), ctypes.byref(do)) == 0 and (di.value, do.value) == (iw.value, ow.value)
        out_h = np.zeros((len(a), ow.value), dtype=np.uint32)
        out_d = np.full((len(a), ow.value), 0xEEEEEEEE, dtype=np.uint32)
        ht.ht_reset_checks()
        assert ht.ht_devop(curve.curve_id, op, a.ctypes.data, out_h.ctypes.data, len(a)) == 0
        assert ht.ht_check_failures() == 0
        assert dev.msm_devtest_run(curve.curve_id, op, a.ctypes.data, out_d.ctypes.data, len(a)) == 0
        bad = np.nonzero((out_d != out_h).any(axis=1))[0]
        assert bad.size == 0, (name, op, int(bad[0]))          # limb-identical, before any canonicalisation
        if op != DT_LEX_LARGEST:
            # and right: "has a root" where the model says so, and the root squares to the input
            for (label, comp), row in list(zip(ins, out_d))[::7]:
                comp = comp[:words // NL]
                sq = (kc.sqrt_fp(p, comp[0]) is not None) if len(comp) == 1 else (kc.sqrt_fp2(p, curve.nonresidue, *comp) is not None)
                assert bool(row[-1]) == sq, label
                if sq:
                    r = [sum(int(x) << (28 * i) for i, x in enumerate(row[NL * k:NL * k + NL])) * pow(R392, -1, p) % p for k in range(len(comp))]
                    if len(comp) == 1:
                        assert r[0] * r[0] % p == comp[0], label
                    else:
                        X = pm.Fp2(r[0], r[1], p, curve.nonresidue % p)
                        assert ((X * X).c0, (X * X).c1) == tuple(comp), label


# ---- set_bases_compressed ---------------------------------------------------------------------------------------------------------
HDIR = os.path.join(ROOT, "tests", "golden", "harness")


@pytest.mark.parametrize("which,name", [("377_g1_random", "bls12_377_g1"), ("381_g1_random", "bls12_381_g1")])
def test_set_bases_compressed_runs_the_harness_data(ea, which, name):
    f = ea.formats
    data = f.load_harness_dir(os.path.join(HDIR, which), name)
    ctx = ea.MultiScalarMultContext(name)
    try:
        comp = ctx.compress_points(data.records, serialized=True)
        assert comp.ok and len(comp.points) == data.n * f.record_bytes(name, compressed=True)
        results = {}
        for opts in ({"twisted_edwards": 1}, {"twisted_edwards": 0}):
            for k, v in opts.items():
                ctx.set_option(k, v)
            ctx.set_option("scalars_to_montgomery", 1)
            ctx.set_bases_compressed(comp.points)
            assert ctx.npoints == data.n and ctx.query("bases") == data.n
            got = ctx.run(data.scalars, data.n)
            assert [f.point_to_serialized(g, name) for g in got] == data.expected, opts        # == arkworks_results.bin
            f.set_bases_serialized(ctx, data.records)
            assert ctx.run(data.scalars, data.n) == got, opts                                  # == the same context fed uncompressed records
            if name == "bls12_377_g1":
                assert ctx.query("twisted_edwards") == opts["twisted_edwards"]
            results[opts["twisted_edwards"]] = got
            # point_to_compressed of a result decodes to that result
            for g in got:
                rec = f.point_to_serialized(g, name, compressed=True)
                assert len(rec) == 48
                d = ctx.decompress_points(rec, uncompressed=True)
                assert d.ok and d.points == f.point_to_serialized(g, name)
        assert results[0] == results[1]
    finally:
        ctx.close()


def test_set_bases_compressed_refuses_and_keeps_the_previous_bases(ea):
    name = "bls12_377_g1"
    curve = pm.CURVES[name]
    rng = random.Random(21)
    n = 300
    pts = pm.random_points(curve, n, rng, distinct=40)
    scalars = pm.encode_scalars(pm.random_scalars(curve, n, rng))
    good = b"".join(kc.compress(curve, (kc.comps(curve, P[0]), kc.comps(curve, P[1]))) for P in pts)
    recs, statuses, labels, sub = kc.corpus(name)
    ctx = ea.MultiScalarMultContext(name)
    try:
        ctx.set_bases_compressed(good)
        first = ctx.run(scalars)[0]
        ctx.set_bases(curve.encode_affine_array(pts))
        assert ctx.run(scalars)[0] == first                       # compressed upload == image upload
        ctx.set_bases_compressed(good)
        for status in (1, 2):
            bad = bytearray(good)
            bad[48 * 123:48 * 124] = recs[list(statuses).index(status)]
            with pytest.raises(ea.MsmError) as ei:
                ctx.set_bases_compressed(bytes(bad))
            assert ei.value.code == -1 and "record 123 " in ei.value.message and "status %d" % status in ei.value.message
            assert ctx.query("bases") == n and ctx.run(scalars)[0] == first     # the previous bases stay in force
        # validate_bases = 1: an off-subgroup record decodes (status 0) and is then refused by the existing check
        off = bytearray(good)
        off[48 * 7:48 * 8] = recs[sub.index(False)]
        ctx.set_bases_compressed(bytes(off))                      # without the option it uploads, like any other input
        ctx.set_bases_compressed(good)
        ctx.set_option("validate_bases", 1)
        with pytest.raises(ea.MsmError) as ei:
            ctx.set_bases_compressed(bytes(off))
        assert "point 7 " in ei.value.message and "status 3" in ei.value.message
        assert ctx.run(scalars)[0] == first
        ctx.set_bases_compressed(good)
        assert ctx.query("bases_validated") == 1
        ctx.set_bases_compressed(b"")
        assert ctx.query("bases") == 0
        with pytest.raises(TypeError):
            ctx.set_bases_compressed(_cuda(good))
    finally:
        ctx.close()


def test_sharded_context_refuses(ea):
    ctx = ea.MultiScalarMultContext("bls12_377_g1", devices=[0, 0])
    try:
        rec = kc.corpus("bls12_377_g1")[0][0]
        for call in (lambda: ctx.decompress_points(rec), lambda: ctx.compress_points(bytes(104)), lambda: ctx.set_bases_compressed(rec)):
            with pytest.raises(ea.MsmError) as ei:
                call()
            assert ei.value.code == -1 and "sharded" in ei.value.message
    finally:
        ctx.close()


def test_argument_errors(ea):
    ctx = ea.MultiScalarMultContext("bls12_381_g1")
    try:
        rec = kc.corpus("bls12_381_g1")[0][0]
        out8 = (ctypes.c_uint64 * 8)()
        buf = ctypes.create_string_buffer(256)
        st = ctypes.create_string_buffer(8)
        lib = ctx._lib
        for e in (lib.mi355_msm_decompress_points(ctx.context, rec, 1, buf, 96, 0, st, out8),          # stride does not reach the flag
                  lib.mi355_msm_decompress_points(ctx.context, rec, 1, buf, 102, 0, st, out8),         # not a multiple of 4
                  lib.mi355_msm_decompress_points(ctx.context, rec, 1, buf, 104, 8, st, out8),         # unknown flag
                  lib.mi355_msm_decompress_points(ctx.context, None, 1, buf, 104, 0, st, out8),
                  lib.mi355_msm_decompress_points(ctx.context, rec, 1, buf, 104, 0, st, None),
                  lib.mi355_msm_decompress_points(None, rec, 1, buf, 104, 0, st, out8),
                  lib.mi355_msm_compress_points(ctx.context, buf, 1, 104, 2, buf, st, out8),
                  lib.mi355_msm_compress_points(ctx.context, buf, 1, 96, 0, buf, st, out8),
                  lib.mi355_msm_set_bases_compressed(ctx.context, None, 1),
                  lib.mi355_msm_point_to_compressed(1, None, buf),
                  lib.mi355_msm_point_to_compressed(9, buf, buf)):
            assert e.code == -1 and e.message
            _free(e.message)
        with pytest.raises(ValueError):
            ctx.decompress_points(rec + b"\0")
        with pytest.raises(ValueError):
            ctx.compress_points(bytes(100))
    finally:
        ctx.close()


# ---- produce and consume on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_fixed_base_output_round_trips_on_the_device(ea, name):
    torch = _torch()
    curve = pm.CURVES[name]
    n = 1 << 12
    rng = np.random.default_rng(12 + curve.curve_id)
    scalars = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    scalars[3, :] = 0                                                    # one point at infinity among them
    g = curve.encode_affine(curve.generator())
    images = ea.fixed_base_msm(g, torch.from_numpy(scalars).cuda(), curve=name)
    assert images.is_cuda and tuple(images.shape) == (n, curve.affine_stride)
    comp = ea.compress_points(images, curve=name)
    assert comp.points.is_cuda and comp.ok and comp.counts["flagged_infinity"] == 1 and tuple(comp.points.shape) == (n, curve.coord_bytes)
    back = ea.decompress_points(comp.points, curve=name)
    assert back.points.is_cuda and back.ok and back.counts["flagged_infinity"] == 1
    assert torch.equal(back.points, images)
    # a sample against the model
    img = images.cpu().numpy()
    rec = comp.points.cpu().numpy()
    for i in (0, 1, 3, 777, n - 1):
        P = curve.decode_affine(img[i].tobytes())
        want = kc.compress(curve, None if P is None else (kc.comps(curve, P[0]), kc.comps(curve, P[1])))
        assert rec[i].tobytes() == want


# ---- speed guard --------------------------------------------------------------------------------------------------------------------
# Modelled field products per point: decompress = the root (BLS12-381: a^((p+1)/4) by a 2-bit window, about 380 squarings + 145
# products, with the conversions about 540; BLS12-377: a fixed-trip Tonelli-Shanks, 330 + 125 for the exponent, 990 + 135 for the rounds,
# about 1600) against check_bases (endomorphism) = 126 doublings * 9 + additions, about 1250 / 1260.
MODELLED_RATIO = {"bls12_381_g1": 0.4, "bls12_377_g1": 1.3}
GUARD_K = {name: 2 * r for name, r in MODELLED_RATIO.items()}


@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g1"])
def test_decompress_speed_guard(ea, name):
    """At 2^20 device-resident records, decompress takes at most K x what check_bases (endomorphism; the parent commit's kernel, so the
    yardstick is not the code under test) takes on the same points in the same test.  K = 2 x the modelled ratio of field products
    (0.4 for BLS12-381, 1.3 for BLS12-377: K = 0.8 / 2.6), the allowance tests/test_gpu_fixed_base.py gives its own model for gathers
    and tails.  Measured: nothing yet; once profiles/point_codec.txt exists K becomes the measured ratio x 1.5."""
    torch = _torch()
    curve = pm.CURVES[name]
    n = 1 << 20
    images = torch.from_numpy(np.asarray(ea.generate_points(n, distinct=1 << 12, seed=31, curve=name)).reshape(-1)).cuda()
    ctx = ea.MultiScalarMultContext(name)
    try:
        comp = ctx.compress_points(images)
        assert comp.ok
        ctx.decompress_points(comp.points)                       # warm-up (buffers, code)
        ctx.check_bases(images)
        dec = min(ctx.decompress_points(comp.points).device_us for _ in range(3))
        last = ctx.decompress_points(comp.points)
        chk = min(ctx.check_bases(images).device_us for _ in range(3))
        assert last.ok and torch.equal(last.points.reshape(-1), images)
    finally:
        ctx.close()
    ratio = dec / chk
    print(f"{name} 2^20: decompress {dec} us, check_bases (endomorphism) {chk} us, ratio {ratio:.3f}, K {GUARD_K[name]}")
    assert ratio <= GUARD_K[name], (dec, chk, ratio)
