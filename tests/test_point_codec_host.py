"""CPU: the square roots, the y ordering and the compressed-record codec (csrc/sqrt.hpp, csrc/point_codec.hpp) compiled for the
host with the limb-bound checker armed (libmsm_hosttest.so), against the Python model of tests/codec_cases.py, all four curves."""
import ctypes
import json
import os
import random

import pytest

import codec_cases as kc
import pymodel as pm
from conftest import ROOT

R384 = 1 << 384


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    lib.ht_fe_sqrt.argtypes = lib.ht_fe2_sqrt.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    lib.ht_lex_largest.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    lib.ht_decompress_points.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lib.ht_compress_points.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p]
    return lib


def abi(p, comp):
    return b"".join((c * R384 % p).to_bytes(48, "little") for c in comp)


def from_abi(p, raw):
    return tuple(int.from_bytes(raw[i:i + 48], "little") * pow(R384, -1, p) % p for i in range(0, len(raw), 48))


def host_sqrt(ht, curve, comp):
    out = ctypes.create_string_buffer(48 * curve.ext)
    ok = ctypes.c_int(-1)
    fn = ht.ht_fe_sqrt if curve.ext == 1 else ht.ht_fe2_sqrt
    assert fn(curve.curve_id, abi(curve.p, comp), out, ctypes.byref(ok)) == 0
    raw = out.raw
    assert all(int.from_bytes(raw[i:i + 48], "little") < curve.p for i in range(0, len(raw), 48))
    return ok.value, from_abi(curve.p, raw)


def square(curve, comp):
    X = curve.F(comp[0] if curve.ext == 1 else comp)
    return kc.comps(curve, curve.f_mul(X, X))


def sqrt_inputs(curve):
    """(label, components): the inputs the issue lists."""
    p = curve.p
    rng = random.Random(0x5157 + curve.curve_id)
    pad = (0,) * (curve.ext - 1)
    out = [("0", (0,) + pad), ("1", (1,) + pad), ("4", (4,) + pad), ("p - 1", (p - 1,) + pad)]
    if p == pm.BLS12_377_G1.p:
        t = (p - 1) >> 46
        zeta = pow(15, t, p)
        for k in range(46):   # zeta^(2^k): one input per Tonelli-Shanks depth; zeta itself has no root in Fp
            out.append(("zeta^(2^%d)" % k, (pow(zeta, 1 << k, p),) + pad))
        out.append(("zeta^3", (pow(zeta, 3, p),) + pad))
    squares = nons = 0
    while squares < 200 or nons < 200:
        a = tuple(rng.randrange(p) for _ in range(curve.ext))
        sq = kc.el_sqrt(curve, a) is not None
        if sq and squares < 200:
            squares += 1
            out.append(("random square", a))
        elif not sq and nons < 200:
            nons += 1
            out.append(("random non-square", a))
    if curve.ext == 2:
        for _ in range(12):   # c1 == 0 with c0 square / non-square (the latter has its root on the u axis), and c0 == 0
            a = rng.randrange(1, p)
            out.append(("c1 = 0, c0 %s" % ("square" if kc.is_square_fp(p, a) else "non-square"), (a, 0)))
            out.append(("c0 = 0", (0, a)))
        assert {"c1 = 0, c0 square", "c1 = 0, c0 non-square"} <= {l for l, _ in out}
    return out


@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_square_roots(ht, name):
    curve = pm.CURVES[name]
    before = ht.ht_check_failures()
    roots = 0
    for label, a in sqrt_inputs(curve):
        ok, r = host_sqrt(ht, curve, a)
        want = kc.el_sqrt(curve, a) is not None
        assert bool(ok) == want, (label, a)
        if want:   # either root
            assert square(curve, r) == tuple(a), (label, a, r)
            roots += 1
    assert roots >= 200
    if curve.ext == 1 and curve.p == pm.BLS12_377_G1.p:
        p = curve.p
        zeta = pow(15, (p - 1) >> 46, p)
        assert host_sqrt(ht, curve, (zeta,))[0] == 0 and host_sqrt(ht, curve, (pow(zeta, 3, p),))[0] == 0
        assert all(host_sqrt(ht, curve, (pow(zeta, 1 << k, p),))[0] == 1 for k in (1, 45))
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()   # every limb bound held through the squaring chains


@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_lex_largest(ht, name):
    curve = pm.CURVES[name]
    p = curve.p
    h = (p - 1) // 2
    rng = random.Random(7 + curve.curve_id)
    if curve.ext == 1:
        ys = [(h,), (h + 1,), (0,), (1,), (p - 1,)] + [(rng.randrange(p),) for _ in range(50)]
    else:
        ys = [(h, 0), (h + 1, 0), (0, 0), (0, h), (0, h + 1), (h + 1, h), (h, h + 1), (p - 1, 1), (1, p - 1), (h + 1, 1), (h, p - 1)]
        ys += [(rng.randrange(p), rng.randrange(p)) for _ in range(50)] + [(rng.randrange(p), 0) for _ in range(20)]
    for y in ys:
        got = ctypes.c_int(-1)
        assert ht.ht_lex_largest(curve.curve_id, abi(p, y), ctypes.byref(got)) == 0
        assert bool(got.value) == kc.lex_largest(curve, y), y
    assert kc.lex_largest(curve, (h,) + (0,) * (curve.ext - 1)) is False and kc.lex_largest(curve, (h + 1,) + (0,) * (curve.ext - 1)) is True
    assert ht.ht_check_failures() == 0


def decompress(ht, curve, records, serialized, stride=None):
    n = len(records) // curve.coord_bytes
    stride = 2 * curve.coord_bytes if serialized else (stride or curve.affine_stride)
    out = ctypes.create_string_buffer(max(n * stride, 1))
    status = ctypes.create_string_buffer(max(n, 1))
    assert ht.ht_decompress_points(curve.curve_id, int(serialized), records, n, out, stride, status) == 0
    return list(status.raw[:n]), out.raw[:n * stride]


def compress(ht, curve, points, serialized, stride=None):
    stride = 2 * curve.coord_bytes if serialized else (stride or curve.affine_stride)
    n = len(points) // stride
    out = ctypes.create_string_buffer(max(n * curve.coord_bytes, 1))
    status = ctypes.create_string_buffer(max(n, 1))
    assert ht.ht_compress_points(curve.curve_id, int(serialized), points, stride, n, out, status) == 0
    return list(status.raw[:n]), out.raw[:n * curve.coord_bytes]


@pytest.mark.parametrize("serialized", [False, True], ids=["images", "uncompressed"])
@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_corpus_decodes_byte_for_byte(ht, name, serialized):
    curve = pm.CURVES[name]
    recs, statuses, labels, _ = kc.corpus(name)
    data = b"".join(recs)
    want_st, want = kc.expected(curve, data, serialized)
    assert want_st == list(statuses)
    got_st, got = decompress(ht, curve, data, serialized)
    stride = len(want) // len(recs)
    assert got_st == want_st, [(l, a, b) for l, a, b in zip(labels, got_st, want_st) if a != b]
    bad = [labels[i] for i in range(len(recs)) if got[i * stride:(i + 1) * stride] != want[i * stride:(i + 1) * stride]]
    assert not bad, bad
    # compressing what decoded gives the original bytes back (failed records decoded to zeros and are left out)
    keep = [i for i, s in enumerate(want_st) if s == 0 and not (recs[i][-1] & 0x40)]
    pts = b"".join(got[i * stride:(i + 1) * stride] for i in keep)
    cst, crecs = compress(ht, curve, pts, serialized)
    assert cst == [0] * len(keep)
    cb = curve.coord_bytes
    for j, i in enumerate(keep):
        if labels[i].startswith("x = p - 1"):   # y = 0: both flag values name the same point, the encoder writes bit 7 clear
            assert crecs[j * cb:(j + 1) * cb] == recs[i][:-1] + bytes([recs[i][-1] & 0x3f])
        else:
            assert crecs[j * cb:(j + 1) * cb] == recs[i], labels[i]
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_corpus_holds_what_it_should():
    for name in kc.CURVE_NAMES:
        curve = pm.CURVES[name]
        recs, statuses, labels, sub = kc.corpus(name)
        st = dict(zip(labels, statuses))
        assert st["generator, bit 7 set"] == st["generator, bit 7 clear"] == 0
        assert st["x + p stored"] == st["x = p stored"] == 1
        assert st["both flag bits over a valid x"] == st["both flag bits over zero"] == 1
        assert st["infinity over zero"] == st["infinity over garbage"] == st["infinity over all ones"] == 0
        assert st["no point has this x"] == 2
        # the off-subgroup and small-order points decode with status 0 when nobody asks for validation
        off = [s for l, s in zip(labels, statuses) if l.startswith("off subgroup")]
        assert len(off) >= 10 and set(off) == {0} and sub.count(False) >= 10
        if curve.ext == 1:   # (a G2 cofactor need not have a small prime factor: check_cases.small_order_points)
            assert any(l.startswith("off subgroup: T of order") for l in labels)
        # x = 0 without the flag is never the point at infinity
        i = labels.index("x = 0 without the flag")
        s, P = kc.decode(curve, recs[i])
        assert (s == 0 and P is not None and curve.on_curve(kc.cc.to_model(curve, *P))) or (s == 2 and curve.ext == 2)
        if curve.ext == 1:
            assert s == 0
    # BLS12-377 G1, x = p - 1: y = 0, and both flag values give the same point
    curve = pm.BLS12_377_G1
    recs, statuses, labels, _ = kc.corpus("bls12_377_g1")
    a, b = (kc.decode(curve, recs[labels.index("x = p - 1 (y = 0), bit 7 %s" % w)]) for w in ("clear", "set"))
    assert a == b == (0, ((curve.p - 1,), (0,)))


@pytest.mark.parametrize("name", kc.CURVE_NAMES)
def test_golden_fixture(ht, name):
    curve = pm.CURVES[name]
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "compressed", name + ".json")))
    recs = [bytes.fromhex(r) for r in doc["records"]]
    assert len(recs) == 64 and doc["curve"] == name
    assert [kc.decode(curve, r)[0] for r in recs] == doc["status"]          # the fixture is the model's
    st, unc = decompress(ht, curve, b"".join(recs), True)
    assert st == doc["status"]
    assert unc == b"".join(bytes.fromhex(u) for u in doc["uncompressed"])
    st_i, img = decompress(ht, curve, b"".join(recs), False)
    assert st_i == doc["status"] and img == kc.expected(curve, b"".join(recs), False)[1]


def test_compress_refuses_a_non_canonical_coordinate(ht):
    for name in kc.CURVE_NAMES:
        curve = pm.CURVES[name]
        p = curve.p
        G = curve.generator()
        g = kc.comps(curve, G[0]) + kc.comps(curve, G[1])
        for c in range(2 * curve.ext):
            ser = b"".join((v + (p if i == c else 0)).to_bytes(48, "little") for i, v in enumerate(g))
            assert compress(ht, curve, ser, True) == ([1], bytes(curve.coord_bytes))
            img = b"".join((v * R384 % p + (p if i == c else 0)).to_bytes(48, "little") for i, v in enumerate(g)) + bytes(8)
            assert compress(ht, curve, img, False) == ([1], bytes(curve.coord_bytes))
        # a flagged image is infinity whatever its coordinates hold; an uncompressed record carries the flag in bit 6
        inf_rec = bytes(curve.coord_bytes - 1) + b"\x40"
        assert compress(ht, curve, b"\xff" * (2 * curve.coord_bytes) + b"\x01" + bytes(7), False) == ([0], inf_rec)
        assert compress(ht, curve, kc.uncompressed(curve, 0, None), True) == ([0], inf_rec)


def harness_points(which):
    raw = open(os.path.join(ROOT, "tests", "golden", "harness", which, "points.bin"), "rb").read()
    n = int.from_bytes(raw[:8], "little")
    assert n == 1024 and len(raw) == 8 + 96 * n
    return raw[8:]


@pytest.mark.parametrize("which,name", [("377_g1_random", "bls12_377_g1"), ("381_g1_random", "bls12_381_g1")])
def test_harness_points_round_trip(ht, which, name):
    curve = pm.CURVES[name]
    unc = harness_points(which)
    st, recs = compress(ht, curve, unc, True)
    assert st == [0] * 1024
    # the model agrees on a sample, the round trip holds for all 1024
    for i in range(0, 1024, 97):
        x = int.from_bytes(unc[96 * i:96 * i + 48], "little")
        y = int.from_bytes(unc[96 * i + 48:96 * i + 96], "little")
        assert recs[48 * i:48 * i + 48] == kc.compress(curve, ((x,), (y,)))
    st2, back = decompress(ht, curve, recs, True)
    assert st2 == [0] * 1024 and back == unc
    assert ht.ht_check_failures() == 0


def test_rfc9380_points_round_trip(ht):
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "h2c_kat_bls12_381.json")))
    for grp, name in (("g1", "bls12_381_g1"), ("g2", "bls12_381_g2")):
        curve = pm.CURVES[name]
        pts = []
        for v in doc[grp]["vectors"]:
            for k in ("Q0", "Q1", "P"):
                pts.append((tuple(int(c, 16) for c in v[k]["x"].split(",")), tuple(int(c, 16) for c in v[k]["y"].split(","))))
        assert len(pts) >= 9
        unc = b"".join(kc.uncompressed(curve, 0, P) for P in pts)
        st, recs = compress(ht, curve, unc, True)
        assert st == [0] * len(pts) and recs == b"".join(kc.compress(curve, P) for P in pts)
        st2, back = decompress(ht, curve, recs, True)
        assert st2 == [0] * len(pts) and back == unc
        st3, img = decompress(ht, curve, recs, False)
        assert compress(ht, curve, img, False) == ([0] * len(pts), recs)


@pytest.mark.parametrize("n", [0, 1, 255, 257, 1000])
def test_placement(ht, n):
    curve = pm.BLS12_381_G1
    recs, statuses = kc.placed("bls12_381_g1", n)
    got_st, got = decompress(ht, curve, b"".join(recs), True)
    assert got_st == statuses
    assert got == kc.expected(curve, b"".join(recs), True)[1]
    if n:
        assert statuses[0] != 0 and statuses[n - 1] != 0


def test_stride_and_bad_arguments(ht):
    curve = pm.BLS12_377_G1
    recs, _, _, _ = kc.corpus("bls12_377_g1")
    data = b"".join(recs[:8])
    st, img = decompress(ht, curve, data, False, stride=112)      # every pad byte of a wider stride is written as zero
    assert img == kc.expected(curve, data, False, stride=112)[1]
    out = ctypes.create_string_buffer(1024)
    s = ctypes.create_string_buffer(8)
    assert ht.ht_decompress_points(7, 0, data, 1, out, 104, s) == -1
    assert ht.ht_decompress_points(0, 0, data, 1, out, 96, s) == -1        # stride does not reach the flag byte
    assert ht.ht_decompress_points(0, 0, data, 1, out, 102, s) == -1       # not a multiple of 4
    assert ht.ht_compress_points(0, 0, bytes(104), 96, 1, out, s) == -1
    ok = ctypes.c_int()
    assert ht.ht_fe_sqrt(2, bytes(48), out, ctypes.byref(ok)) == -1 and ht.ht_fe2_sqrt(0, bytes(96), out, ctypes.byref(ok)) == -1
