"""CPU: the per-element functions of csrc/group_fft.hpp -- the index maps, the twiddle exponent, the twiddle as canonical words, the
table of a butterfly's B, the walk and the butterfly -- compiled for the host with the limb-bound checker armed
(libmsm_hosttest.so, ht_gf_*), in the order the engine launches them, against the Python model's group arithmetic and the
big-integer transforms of ntt_cases.py."""
import ctypes
import os
import random

import pytest

import gfft_cases as gc
import ntt_cases as nc
import pymodel as pm
from conftest import ROOT


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    cp, sz, ci, cu = ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    lib.ht_gf_index.argtypes = [cu, cu, cu, ctypes.POINTER(ctypes.c_uint32)]
    lib.ht_gf_twiddle_words.argtypes = [ci, cu, ci, ctypes.POINTER(ctypes.c_uint32), sz, cp]
    lib.ht_gf_transform.argtypes = [ci, cu, cu, cp, cp, sz, cu, ci, cu, cp, sz]
    lib.ht_check_failures.restype = ctypes.c_long
    lib.ht_first_failure.restype = ctypes.c_char_p
    return lib


def host_transform(ht, name, n, kind, images, in_len=None, offset=None, w=4, projective=False, stride=None, out_stride=None):
    curve = pm.CURVES[name]
    size = curve.projective_bytes if projective else curve.affine_stride
    stride = stride or curve.affine_stride
    out_stride = out_stride or size
    in_len = len(images) // stride if in_len is None else in_len
    out = ctypes.create_string_buffer(b"\xa5" * (out_stride * n), out_stride * n)
    off = None if offset is None else ((offset << 256) % curve.r).to_bytes(32, "little")
    rc = ht.ht_gf_transform(curve.curve_id, gc.log2(n), kind, off, images or None, stride, in_len, w, 2 if projective else 0, out, out_stride)
    assert rc == 0, (name, n, kind)
    raw = out.raw
    return b"".join(raw[i * out_stride:i * out_stride + size] for i in range(n)), raw


def test_index_maps_and_twiddle_exponents(ht):
    """The stages compute the transform: run on integers through the index maps and exponents the kernels use, they give the DFT; every
    stage reads each element once and stage 0 has exponent 0 throughout."""
    field = "bls12_381"
    r = nc.modulus(field)
    out = (ctypes.c_uint32 * 3)()
    for k in range(1, 8):
        n = 1 << k
        omega = nc.root_of_unity(field, k)
        x = nc.random_values(field, n, 0x1D + k)
        want = nc.dft_direct(x, omega, r)
        for s in range(k):
            y = [None] * n
            seen = set()
            for b in range(n // 2):
                assert ht.ht_gf_index(k, s, b, out) == 0
                ia, ib, e = out[0], out[1], out[2]
                assert ib == ia + (1 << (k - s - 1)) and e < n // 2 and (s or e == 0)
                assert not {ia, ib} & seen
                seen |= {ia, ib}
                t = x[ib] * pow(omega, e, r) % r
                y[b], y[b + n // 2] = (x[ia] + t) % r, (x[ia] - t) % r
            assert len(seen) == n
            x = y
        assert x == want, k
    assert ht.ht_gf_index(3, 3, 0, out) == -1 and ht.ht_gf_index(3, 0, 4, out) == -1 and ht.ht_gf_index(0, 0, 0, out) == -1


@pytest.mark.parametrize("field", ["bls12_377", "bls12_381"])
def test_twiddle_words_of_a_domain_with_two_table_levels(ht, field):
    """k = 15: LO has 2^14 entries and HI two.  The words are the canonical integer of omega^e (omega^-e), for 4096 exponents"""
    k = 15
    n = 1 << k
    r = nc.modulus(field)
    rng = random.Random(0x7D)
    exps = [0, 1, (1 << 14) - 1, 1 << 14, n // 2 - 1, (1 << 14) + 1, n - 1]
    exps += [rng.randrange(n) for _ in range(4096 - len(exps))]
    arr = (ctypes.c_uint32 * len(exps))(*exps)
    before = ht.ht_check_failures()
    for inverse in (0, 1):
        out = ctypes.create_string_buffer(32 * len(exps))
        assert ht.ht_gf_twiddle_words(nc.FIELD_IDS[field], k, inverse, arr, len(exps), out) == 0
        omega = nc.root_of_unity(field, k)
        if inverse:
            omega = pow(omega, -1, r)
        got = [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(len(exps))]
        assert got == [pow(omega, e, r) for e in exps], (field, inverse)
    bad = (ctypes.c_uint32 * 1)(n)
    assert ht.ht_gf_twiddle_words(nc.FIELD_IDS[field], k, 0, bad, 1, ctypes.create_string_buffer(32)) == -1
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


@pytest.mark.parametrize("name", gc.CURVE_NAMES)
def test_transforms_against_the_model(ht, name):
    """n = 1 .. 64 (G2: .. 16), the four kinds, random logs: byte-equal to (the transform of the logs) * G"""
    curve = pm.CURVES[name]
    sizes = (1, 2, 4, 8, 16) if curve.ext == 2 else (1, 2, 4, 8, 16, 64)
    before = ht.ht_check_failures()
    for n in sizes:
        logs = gc.random_logs(name, n, 0x6F + n)
        images = gc.model_images(name, logs)
        for kind in gc.KINDS:
            offset = gc.OTHER_OFFSET if (kind & 2 and n in (4, 16)) else None
            want = gc.model_images(name, gc.transform_logs(name, n, kind, logs, offset))
            got, _ = host_transform(ht, name, n, kind, images, offset=offset)
            assert got == want, (name, n, kind)
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_window_projective_stride_and_in_len(ht, name):
    curve = pm.CURVES[name]
    n = 8
    logs = gc.random_logs(name, n, 0x51)
    images = gc.model_images(name, logs)
    want_logs = gc.transform_logs(name, n, nc.COSET_INVERSE, logs)
    want = gc.model_images(name, want_logs)
    for w in (1, 3, 5, 6):
        got, _ = host_transform(ht, name, n, nc.COSET_INVERSE, images, w=w)
        assert got == want, (name, w)
    got, _ = host_transform(ht, name, n, nc.COSET_INVERSE, images, projective=True)
    assert got == gc.model_images(name, want_logs, projective=True)
    # strides on both sides: the bytes between two output images stay as they were; the input's bytes past in_len are never read
    st = curve.affine_stride + 8
    spread = b"".join(images[i * curve.affine_stride:(i + 1) * curve.affine_stride] + b"\xff" * 8 for i in range(5)) + b"\xff" * (3 * st)
    want5 = gc.model_images(name, gc.transform_logs(name, n, nc.FORWARD, logs[:5]))
    got, raw = host_transform(ht, name, n, nc.FORWARD, spread, in_len=5, stride=st, out_stride=st + 4)
    assert got == want5
    assert all(raw[i * (st + 4) + curve.affine_stride:(i + 1) * (st + 4)] == b"\xa5" * 12 for i in range(n))
    got, _ = host_transform(ht, name, n, nc.COSET_FORWARD, spread, in_len=5, stride=st)
    assert got == gc.model_images(name, gc.transform_logs(name, n, nc.COSET_FORWARD, logs[:5]))
    got, _ = host_transform(ht, name, n, nc.INVERSE, b"", in_len=0)
    assert got == gc.infinity_image(curve) * n
    assert ht.ht_check_failures() == 0, ht.ht_first_failure()


@pytest.mark.parametrize("name", gc.CURVE_NAMES)
def test_doubling_cancellation_and_infinities(ht, name):
    """all points equal (every butterfly of stage 0 doubles and cancels), B = -A, every second point at infinity, infinities flagged
    over junk coordinates"""
    curve = pm.CURVES[name]
    r = curve.r
    n = 8
    h = gc.random_logs(name, 1, 0xE0)[0]
    half = gc.random_logs(name, n // 2, 0xE1)
    cases = {
        "all equal": [h] * n,
        "B = -A": half + [r - v for v in half],
        "B = A": half + half,
        "every second point at infinity": [v if i % 2 == 0 else 0 for i, v in enumerate(gc.random_logs(name, n, 0xE2))],
        "all infinity": [0] * n,
    }
    before = ht.ht_check_failures()
    for label, logs in cases.items():
        # a log of 0 is the point at infinity: flag byte 1 over the generator's coordinates
        inf = gc.fc.base_image(curve, None)
        st = curve.affine_stride
        model = gc.model_images(name, logs)
        images = b"".join(inf if v % r == 0 else model[i * st:(i + 1) * st] for i, v in enumerate(logs))
        for kind in gc.KINDS:
            want = gc.model_images(name, gc.transform_logs(name, n, kind, logs))
            got, _ = host_transform(ht, name, n, kind, images)
            assert got == want, (name, label, kind)
    got, _ = host_transform(ht, name, n, nc.FORWARD, gc.model_images(name, [h] * n))
    assert got == gc.model_images(name, [n * h]) + gc.infinity_image(curve) * (n - 1)
    assert ht.ht_check_failures() == before == 0, ht.ht_first_failure()


def test_bad_arguments(ht):
    out = ctypes.create_string_buffer(4096)
    img = (bytes(96) + b"\x01" + bytes(7)) * 4   # four flagged infinities
    assert ht.ht_gf_transform(0, 2, 0, None, img, 104, 4, 4, 0, out, 104) == 0
    assert ht.ht_gf_transform(7, 2, 0, None, img, 104, 4, 4, 0, out, 104) == -1
    assert ht.ht_gf_transform(0, 2, 4, None, img, 104, 4, 4, 0, out, 104) == -1
    assert ht.ht_gf_transform(0, 2, 0, None, img, 104, 5, 4, 0, out, 104) == -1       # in_len > n
    assert ht.ht_gf_transform(0, 2, 0, None, img, 104, 4, 7, 0, out, 104) == -1       # window
    assert ht.ht_gf_transform(0, 2, 0, None, img, 104, 4, 4, 1, out, 104) == -1       # flag bit 0 does not exist
    assert ht.ht_gf_transform(0, 2, 0, bytes(32), img, 104, 4, 4, 0, out, 104) == -1  # an offset on a plain transform
    assert ht.ht_gf_transform(0, 2, 0, None, img, 106, 4, 4, 0, out, 104) == -1
