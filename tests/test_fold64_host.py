"""CPU: the 64-bit host tail of an MSM (csrc/host_fold64.hpp: window fold, chunk sums, normalisation on 6 x u64 Montgomery
limbs) against (i) the generic radix-2^28 arithmetic it replaces and (ii) the big-int model -- field operations, the
short-Weierstrass fold for both G1 curves, and the twisted-Edwards fold with the map back (BLS12-377).

The fold of a WIDE anchored window (`wide_a` of fold_windows64 / fold_windows_te64) is compared with the model's curve arithmetic on the
identity of the header comment,  sum_(w<a) 2^(c w) S_w + 2^(c a) (S_a + S_(a+1) + 2^(c-1) R),  as affine points."""
import ctypes
import os
import random

import pytest

import pymodel as m
from conftest import ROOT

R384 = 1 << 384


@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    lib.ht_f64_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.ht_fold_both.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p]
    lib.ht_fold_wide.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    return lib


def mont(v, p):
    return ((v * R384) % p).to_bytes(48, "little")


@pytest.mark.parametrize("cid,curve", [(0, m.BLS12_377_G1), (1, m.BLS12_381_G1)])
def test_f64_field_ops(ht, cid, curve):
    p = curve.p
    rng = random.Random(5 + cid)
    vals = [0, 1, p - 1, p - 2, 2, (p + 1) // 2] + [rng.randrange(p) for _ in range(40)]
    out = ctypes.create_string_buffer(48)
    for a in vals:
        for b in (vals[0], vals[2], rng.choice(vals), rng.randrange(p)):
            # op 0 = Fp64::mul (mulx / adcx / adox assembly where the CPU has them), op 4 = the portable no-carry CIOS loop
            for op, fn in ((0, lambda x, y: x * y), (4, lambda x, y: x * y), (1, lambda x, y: x + y), (2, lambda x, y: x - y)):
                assert ht.ht_f64_op(cid, op, mont(a, p), mont(b, p), out) == 0
                assert out.raw == mont(fn(a, b) % p, p), (op, a, b)
        if a:
            assert ht.ht_f64_op(cid, 3, mont(a, p), mont(0, p), out) == 0
            assert out.raw == mont(pow(a, p - 2, p), p)


@pytest.mark.parametrize("cid,curve,te", [(0, m.BLS12_377_G1, 0), (1, m.BLS12_381_G1, 0), (0, m.BLS12_377_G1, 1), (2, m.BLS12_377_G2, 0), (3, m.BLS12_381_G2, 0)])
def test_fold64_matches_generic_and_model(ht, cid, curve, te):
    rng = random.Random(31 + 2 * cid + te)
    pb = 288 if cid >= 2 else 144                      # G2 (Fp2_64 over Fp64): coordinates are c0 | c1
    for windows, c in ((1, 5), (3, 7), (13, 20), (37, 7), (11, 24)) if cid < 2 else ((1, 5), (3, 7), (13, 9)):
        pts = m.random_points(curve, windows, rng)
        mult = [rng.randrange(1, 1 << 40) for _ in range(windows)]
        if windows >= 3:
            mult[1] = 0                      # an empty window
            if not te:
                pts[2] = None                # a window sum at infinity
            pts[-1] = pts[0]                 # equal points: the add-becomes-doubling branch
            mult[-1] = mult[0]
        arr = (ctypes.c_uint64 * windows)(*mult)
        og, oh = ctypes.create_string_buffer(pb), ctypes.create_string_buffer(pb)
        rc = ht.ht_fold_both(cid, curve.encode_affine_array(pts), 200 if cid >= 2 else 104, arr, windows, c, te, og, oh)
        assert rc == 0, rc
        acc = None
        for w in range(windows - 1, -1, -1):
            for _ in range(c):
                acc = curve.add(acc, acc)
            acc = curve.add(acc, curve.mul(mult[w], pts[w]) if pts[w] is not None else None)
        assert og.raw == oh.raw == curve.encode_projective_normalized(acc), (windows, c)


def test_fold64_cancellation_to_infinity(ht):
    curve = m.BLS12_377_G1
    P = m.random_points(curve, 1, random.Random(9))[0]
    pts = [P, curve.neg(P)]
    # 2^4 * (1 * -P) + 16 * P = O
    arr = (ctypes.c_uint64 * 2)(16, 1)
    for te in (0, 1):
        og, oh = ctypes.create_string_buffer(144), ctypes.create_string_buffer(144)
        assert ht.ht_fold_both(0, curve.encode_affine_array(pts), 104, arr, 2, 4, te, og, oh) == 0
        assert og.raw == oh.raw == curve.encode_projective_normalized(None)


def _wide_rows(curve, c, rng):
    """name -> rows 0 .. windows of window sums as (multiplier of the generator, point), None = infinity; row `windows` is R"""
    a = 252 // c - 1
    windows = a + 2
    assert windows == (257 + c - 1) // c
    r, g = curve.r, curve.generator()
    k0, step = rng.randrange(1, r), rng.randrange(1, r)
    base, acc, inc = [], curve.mul(k0, g), curve.mul(step, g)
    for i in range(windows + 1):                         # (an arithmetic progression: one addition per row)
        base.append(((k0 + i * step) % r, acc))
        acc = curve.add(acc, inc)

    def total(rows):
        k = [0 if row is None else row[0] for row in rows]
        return sum(k[w] << (c * w) for w in range(a)) + ((k[a] + k[a + 1] + (k[windows] << (c - 1))) << (c * a))

    cases = {"random": list(base)}
    for name, at in (("R_at_infinity", (windows,)), ("lower_set_at_infinity", (a,)), ("upper_set_at_infinity", (a + 1,)),
                     ("window_empty", (a, a + 1, windows))):
        cases[name] = [None if w in at else row for w, row in enumerate(base)]
    rows = list(base)
    rows[a] = (r - rows[a + 1][0], curve.neg(rows[a + 1][1]))           # S_a = -S_(a+1): the anchored window is 2^(c-1) R alone
    cases["sets_cancel"] = rows
    rows = list(base)
    rows[windows] = None
    k_r = (-total(rows) * pow(1 << (c * a + c - 1), -1, r)) % r         # R such that everything cancels
    rows[windows] = (k_r, curve.mul(k_r, g))
    assert k_r and total(rows) % r == 0
    cases["all_cancel"] = rows
    return a, windows, cases, total


@pytest.mark.parametrize("c", [6, 12, 21])
@pytest.mark.parametrize("cid,curve,te", [(0, m.BLS12_377_G1, 1), (2, m.BLS12_377_G2, 0)], ids=["g1_both_laws", "g2"])
def test_fold64_of_a_wide_anchored_window(ht, cid, curve, te, c):
    rng = random.Random(1000 * cid + c)
    pb, stride = (288, 200) if cid >= 2 else (144, 104)
    a, windows, cases, total = _wide_rows(curve, c, rng)
    g = curve.generator()
    ok = (ctypes.c_int * 2)()
    for name, rows in cases.items():
        pts = [None if row is None else row[1] for row in rows]
        img = curve.encode_affine_array(pts)
        o_sw, o_te = ctypes.create_string_buffer(pb), ctypes.create_string_buffer(pb)
        assert ht.ht_fold_wide(cid, img, stride, windows, c, a, te, o_sw, o_te, ok) == 0
        # the identity, in the model's curve arithmetic (the multipliers are only how the rows were made)
        inner = curve.add(curve.add(pts[a], pts[a + 1]), curve.mul(1 << (c - 1), pts[windows]))
        acc = inner
        for w in range(a - 1, -1, -1):
            acc = curve.add(curve.mul(1 << c, acc), pts[w])
        exp = curve.encode_projective_normalized(acc)
        if name in ("random", "window_empty"):
            assert exp == curve.encode_projective_normalized(curve.mul(total(rows) % curve.r, g)), name
        if name == "all_cancel":
            assert acc is None
        assert ok[0] == 1 and o_sw.raw == exp, (name, c, "short Weierstrass")
        if te:
            assert ok[1] == 1 and o_te.raw == exp, (name, c, "twisted Edwards")
        # wide_a = -1: the plain fold of the same rows (row `windows` is not read)
        p_sw, p_te = ctypes.create_string_buffer(pb), ctypes.create_string_buffer(pb)
        assert ht.ht_fold_wide(cid, img, stride, windows, c, -1, te, p_sw, p_te, ok) == 0
        plain = None
        for w in range(windows - 1, -1, -1):
            plain = curve.add(curve.mul(1 << c, plain), pts[w])
        assert ok[0] == 1 and p_sw.raw == curve.encode_projective_normalized(plain), (name, c)
        if te:
            assert ok[1] == 1 and p_te.raw == p_sw.raw, (name, c)
        og, oh = ctypes.create_string_buffer(pb), ctypes.create_string_buffer(pb)
        if all(p is not None for p in pts[:windows]):      # (ht_fold_both's Edwards rows take no point at infinity)
            one = (ctypes.c_uint64 * windows)(*([1] * windows))
            assert ht.ht_fold_both(cid, img, stride, one, windows, c, te, og, oh) == 0 and oh.raw == p_sw.raw, (name, c)
