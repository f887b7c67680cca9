"""CPU: the fixed-base functions of csrc/fixed_base.hpp -- digit recoding, table levels, windowed_mul, output normalisation --
compiled for the host with the limb-bound checker armed (libmsm_hosttest.so, ht_fb_*), against the Python model."""
import ctypes
import os
import random

import pytest

import fixed_base_cases as fc
import pymodel as pm
from conftest import ROOT


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    lib.ht_fb_digits.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
    lib.ht_fb_table_level.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    lib.ht_fb_mul.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_char_p,
                              ctypes.c_size_t]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def digits(lib, s, w):
    out = (ctypes.c_uint32 * 256)()
    levels = lib.ht_fb_digits(s.to_bytes(32, "little"), w, out)
    assert levels == (256 + w - 1) // w
    return list(out[:levels])


def test_digit_recoding(ht):
    rng = random.Random(0xF1BA5E)
    scalars = [rng.getrandbits(256) for _ in range(10000)] + [0, fc.M256]
    for w in range(1, 21):
        for s in scalars if w in (1, 7, 13, 16, 20) else scalars[::10] + [0, fc.M256]:
            d = digits(ht, s, w)
            assert all(0 <= x < (1 << w) for x in d)
            assert sum(x << (w * j) for j, x in enumerate(d)) == s, (w, hex(s))
        top = 256 - w * ((256 + w - 1) // w - 1)
        assert digits(ht, fc.M256, w) == [(1 << w) - 1] * ((256 + w - 1) // w - 1) + [(1 << top) - 1]
        assert digits(ht, 0, w) == [0] * ((256 + w - 1) // w)
    assert ht.ht_fb_digits(bytes(32), 0, (ctypes.c_uint32 * 256)()) == -1
    assert ht.ht_fb_digits(bytes(32), 21, (ctypes.c_uint32 * 256)()) == -1


def test_digit_recoding_every_scalar_every_window(ht):
    """the full 10^4 x 20 grid (the test above thins it for speed of reading a failure; this one is the requirement)"""
    rng = random.Random(0xD161)
    scalars = [rng.getrandbits(256) for _ in range(10000)]
    out = (ctypes.c_uint32 * 256)()
    for w in range(1, 21):
        for s in scalars:
            levels = ht.ht_fb_digits(s.to_bytes(32, "little"), w, out)
            v = 0
            for j in range(levels - 1, -1, -1):
                v = (v << w) | out[j]
            assert v == s, (w, hex(s))


def table_level(lib, curve, img, w, level):
    stride = curve.affine_stride
    out = ctypes.create_string_buffer(stride << w)
    assert lib.ht_fb_table_level(curve.curve_id, img, w, level, out, stride) == 0
    return out.raw


@pytest.mark.parametrize("w", [3, 8, 13])
@pytest.mark.parametrize("name", fc.CURVE_NAMES)
def test_table_levels(ht, name, w):
    curve = pm.CURVES[name]
    g = curve.generator()
    levels = (256 + w - 1) // w
    rng = random.Random(w)
    before = ht.ht_check_failures()
    for j in (0, 1, levels - 1):
        got = table_level(ht, curve, fc.base_image(curve, g), w, j)
        B = curve.mul(1 << (w * j), g)
        want, acc = [], None
        for d in range(1 << w):
            want.append(curve.encode_affine(acc))           # d * 2^(w j) * g, by d additions of 2^(w j) g ...
            acc = curve.add(acc, B)
        for d in {1, (1 << w) - 1} | {rng.randrange(1 << w) for _ in range(4)}:
            assert want[d] == curve.encode_affine(curve.mul(d << (w * j), g))    # ... which is the model's mul
        assert got == b"".join(want), (name, w, j)
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


@pytest.mark.parametrize("name", fc.CURVE_NAMES)
def test_table_levels_of_small_order_and_infinite_bases(ht, name):
    """entries a base of small order sends to infinity are flagged images, level by level; an infinite base gives nothing else"""
    curve = pm.CURVES[name]
    w = 3
    for label, P in fc.bases(name):
        if not (label.startswith("order") or P is None):
            continue
        for j in (0, 1, 85):
            got = table_level(ht, curve, fc.base_image(curve, P), w, j)
            want = b"".join(curve.encode_affine(None if P is None else curve.mul(d << (w * j), P)) for d in range(1 << w))
            assert got == want, (name, label, j)
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def fb_mul(lib, curve, img, w, scalars, flags=0, stride=None):
    size = curve.projective_bytes if flags & 2 else curve.affine_stride
    stride = stride or size
    n = len(scalars)
    out = ctypes.create_string_buffer(b"\xa5" * (stride * n), stride * n)
    assert lib.ht_fb_mul(curve.curve_id, img, w, pm.encode_scalars(scalars), n, flags, out, stride) == 0
    raw = out.raw
    return b"".join(raw[i * stride:i * stride + size] for i in range(n)), raw


@pytest.mark.parametrize("name", fc.CURVE_NAMES)
def test_windowed_mul_and_normalise(ht, name):
    curve = pm.CURVES[name]
    rnd = fc.random_scalars256(20, 0xFB + curve.curve_id)
    before = ht.ht_check_failures()
    for label, P in fc.bases(name):
        exp = fc.Expect(curve, P)
        img = fc.base_image(curve, P)
        for w in (3, 8, 13):
            if w == 13 and label not in ("generator", "order 2 (p - 1, 0)"):
                continue                                    # (the 164 K-entry table: once per curve, and for the order-2 base)
            ks = list(dict.fromkeys(fc.edge_scalars(curve, w))) + rnd
            got, _ = fb_mul(ht, curve, img, w, ks)
            assert got == exp.affine(ks), (name, label, w)
            got, _ = fb_mul(ht, curve, img, w, ks, flags=2)
            assert got == exp.projective(ks), (name, label, w)
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g2"])
def test_montgomery_scalars_and_stride(ht, name):
    curve = pm.CURVES[name]
    r = curve.r
    g = curve.generator()
    exp = fc.Expect(curve, g)
    rng = random.Random(5)
    # canonical Fr images, and 256-bit "images" at and above r: fr_from_montgomery is a * 2^-256 mod r for any 256-bit a
    images = [rng.randrange(r) for _ in range(70)] + [0, 1, r - 1, r, r + 1, fc.M256, 1 << 255]
    ks = [a * pow(1 << 256, -1, r) % r for a in images]
    got, _ = fb_mul(ht, curve, fc.base_image(curve, g), 8, images, flags=1)
    assert got == exp.affine(ks)
    # a wider stride moves the images and leaves the bytes between them alone
    stride = curve.affine_stride + 16
    got, raw = fb_mul(ht, curve, fc.base_image(curve, g), 8, ks, stride=stride)
    assert got == exp.affine(ks)
    assert all(raw[i * stride + curve.affine_stride:(i + 1) * stride] == b"\xa5" * 16 for i in range(len(ks)))
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


def test_bad_arguments(ht):
    out = ctypes.create_string_buffer(256)
    img = bytes(104)
    assert ht.ht_fb_mul(7, img, 8, bytes(32), 1, 0, out, 104) == -1
    assert ht.ht_fb_mul(0, img, 0, bytes(32), 1, 0, out, 104) == -1
    assert ht.ht_fb_mul(0, img, 21, bytes(32), 1, 0, out, 104) == -1
    assert ht.ht_fb_mul(0, img, 8, bytes(32), 1, 4, out, 104) == -1
    assert ht.ht_fb_mul(0, img, 8, bytes(32), 1, 0, out, 106) == -1
    assert ht.ht_fb_table_level(0, img, 8, 32, out, 104) == -1
