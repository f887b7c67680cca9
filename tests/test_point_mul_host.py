"""CPU: the point-multiplication functions of csrc/point_mul.hpp -- signed digits, non-adjacent form, the per-point table, the windowed
walk, the one-scalar walk -- compiled for the host with the limb-bound checker armed (libmsm_hosttest.so, ht_pm_*), against the
Python model."""
import ctypes
import os
import random

import pytest

import point_mul_cases as pc
import pymodel as pm
from conftest import ROOT


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    cp, sz, ci = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int
    lib.ht_pm_digits.argtypes = [cp, ci, ctypes.POINTER(ctypes.c_int32)]
    lib.ht_pm_top_window.argtypes = [cp, ci]
    lib.ht_pm_naf.argtypes = [cp, sz, ctypes.POINTER(ctypes.c_int8)]
    lib.ht_pm_table.argtypes = [ci, cp, ci, cp, sz]
    lib.ht_pm_mul.argtypes = [ci, cp, sz, sz, cp, ci, ctypes.c_uint, cp, sz]
    lib.ht_pm_mul_uniform.argtypes = [ci, cp, sz, sz, cp, sz, ctypes.c_uint, cp, sz]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def test_signed_recoding(ht):
    """sum d_j 2^(w j) == s with |d_j| <= 2^(w-1) over ceil(257 / w) digits, and no non-zero digit above the window the walk starts at"""
    rng = random.Random(0x9A11)
    scalars = pc.pairwise_edge_scalars(pm.BLS12_377_G1) + pc.pairwise_edge_scalars(pm.BLS12_381_G1)
    scalars += [rng.getrandbits(256) for _ in range(2000)] + [rng.getrandbits(b) for b in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255)]
    scalars += [(1 << b) - 1 for b in range(1, 257)] + [1 << b for b in range(256)]
    out = (ctypes.c_int32 * 257)()
    for w in range(1, 7):
        nd = (257 + w - 1) // w
        for s in scalars:
            raw = s.to_bytes(32, "little")
            assert ht.ht_pm_digits(raw, w, out) == nd
            d = list(out[:nd])
            assert all(abs(x) <= 1 << (w - 1) for x in d), (w, hex(s))
            assert sum(x << (w * j) for j, x in enumerate(d)) == s, (w, hex(s))
            top = ht.ht_pm_top_window(raw, w)
            assert 0 <= top < nd and not any(d[top + 1:]), (w, hex(s))
            if s:
                assert top <= s.bit_length() // w
    assert ht.ht_pm_digits(bytes(32), 0, out) == -1 and ht.ht_pm_digits(bytes(32), 7, out) == -1


def test_naf_recoding(ht):
    rng = random.Random(0x0AF)
    ks = [(0, 4), (1, 4), (3, 4), (0xFFFFFFFF, 4), ((1 << 512) - 1, 64), (1 << 511, 64), (int("aa" * 64, 16), 64), (int("55" * 64, 16), 64)]
    for name in pc.CURVE_NAMES:
        ks += pc.uniform_edge_scalars(pm.CURVES[name])
    ks += [(rng.getrandbits(8 * nb), nb) for nb in range(4, 68, 4) for _ in range(40)]
    out = (ctypes.c_int8 * 544)()
    for k, nb in ks:
        top = ht.ht_pm_naf(k.to_bytes(nb, "little"), nb, out)
        d = list(out)
        assert set(d) <= {-1, 0, 1}
        assert sum(x << i for i, x in enumerate(d)) == k, hex(k)
        assert not any(d[i] and d[i + 1] for i in range(543)), hex(k)
        assert top == max((i for i, x in enumerate(d) if x), default=-1) and top <= 512
    assert ht.ht_pm_naf(bytes(6), 6, out) == -2 and ht.ht_pm_naf(bytes(68), 68, out) == -2 and ht.ht_pm_naf(bytes(4), 0, out) == -2


@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_table(ht, name):
    """1P .. 2^(w-1) P for every base kind: small orders pass through acc == +-P and through infinity"""
    curve = pm.CURVES[name]
    stride = curve.affine_stride
    for label, P, exp in pc.expects(name):
        for w in (1, 2, 4, 6):
            entries = 1 << (w - 1)
            out = ctypes.create_string_buffer(stride * entries)
            assert ht.ht_pm_table(curve.curve_id, pc.fc.base_image(curve, P), w, out, stride) == 0
            assert out.raw == exp.affine(range(1, entries + 1)), (name, label, w)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def pm_mul(lib, curve, points, scalars, w, flags=0, out_stride=None):
    size = curve.projective_bytes if flags & 2 else curve.affine_stride
    out_stride = out_stride or size
    n = len(points)
    out = ctypes.create_string_buffer(b"\xa5" * (out_stride * n), out_stride * n)
    assert lib.ht_pm_mul(curve.curve_id, pc.point_images(curve, points), curve.affine_stride, n, pm.encode_scalars(scalars), w, flags, out, out_stride) == 0
    raw = out.raw
    return b"".join(raw[i * out_stride:i * out_stride + size] for i in range(n)), raw


@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_pairwise_every_base_kind_and_edge_scalar(ht, name):
    curve = pm.CURVES[name]
    edges = pc.pairwise_edge_scalars(curve)
    rnd = pc.fc.random_scalars256(3, 0x9A + curve.curve_id)
    points, scalars, want = [], [], []
    for label, P, exp in pc.expects(name):
        ks = edges + (rnd if label in ("generator", "off the subgroup") else [])
        points += [P] * len(ks)
        scalars += ks
        want += [exp(k) for k in ks]
    before = ht.ht_check_failures()
    for w in (1, 3, 4, 5, 6):
        got, _ = pm_mul(ht, curve, points, scalars, w)
        assert got == pc.want_images(curve, want), (name, w)
    got, _ = pm_mul(ht, curve, points, scalars, 4, flags=2)
    assert got == pc.want_images(curve, want, projective=True)
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_montgomery_scalars_and_stride(ht, name):
    curve = pm.CURVES[name]
    r = curve.r
    g = curve.generator()
    exp = pc.expects(name)[0][2]
    rng = random.Random(6)
    images = [rng.randrange(r) for _ in range(6)] + [0, 1, r - 1, r, r + 1, pc.M256, 1 << 255]
    ks = [a * pow(1 << 256, -1, r) % r for a in images]
    got, _ = pm_mul(ht, curve, [g] * len(ks), images, 4, flags=1)
    assert got == exp.affine(ks)
    stride = curve.affine_stride + 16
    got, raw = pm_mul(ht, curve, [g] * len(ks), ks, 4, out_stride=stride)
    assert got == exp.affine(ks)
    assert all(raw[i * stride + curve.affine_stride:(i + 1) * stride] == b"\xa5" * 16 for i in range(len(ks)))
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("name", pc.CURVE_NAMES)
def test_uniform_every_base_kind_and_edge_scalar(ht, name):
    curve = pm.CURVES[name]
    kinds = pc.expects(name)
    points = [P for _, P, _ in kinds]
    n = len(points)
    size = curve.affine_stride
    before = ht.ht_check_failures()
    for k, nb in pc.uniform_edge_scalars(curve):
        out = ctypes.create_string_buffer(size * n)
        assert ht.ht_pm_mul_uniform(curve.curve_id, pc.point_images(curve, points), size, n, k.to_bytes(nb, "little"), nb, 0, out, size) == 0
        assert out.raw == pc.want_images(curve, [exp(k) for _, _, exp in kinds]), (name, hex(k))
    h = pc.cofactor(curve)
    out = ctypes.create_string_buffer(curve.projective_bytes * n)
    assert ht.ht_pm_mul_uniform(curve.curve_id, pc.point_images(curve, points), size, n, None, 0, 8 | 2, out, curve.projective_bytes) == 0
    assert out.raw == pc.want_images(curve, [exp(h) for _, _, exp in kinds], projective=True)
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


def test_bad_arguments(ht):
    out = ctypes.create_string_buffer(256)
    img = bytes(104)
    assert ht.ht_pm_mul(7, img, 104, 1, bytes(32), 4, 0, out, 104) == -1
    assert ht.ht_pm_mul(0, img, 104, 1, bytes(32), 0, 0, out, 104) == -1
    assert ht.ht_pm_mul(0, img, 104, 1, bytes(32), 7, 0, out, 104) == -1
    assert ht.ht_pm_mul(0, img, 104, 1, bytes(32), 4, 4, out, 104) == -1
    assert ht.ht_pm_mul(0, img, 104, 1, bytes(32), 4, 0, out, 106) == -1
    assert ht.ht_pm_mul_uniform(0, img, 104, 1, bytes(6), 6, 0, out, 104) == -1
    assert ht.ht_pm_mul_uniform(0, img, 104, 1, bytes(4), 4, 1, out, 104) == -1
    assert ht.ht_pm_table(0, img, 7, out, 104) == -1
