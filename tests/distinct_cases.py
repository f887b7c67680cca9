"""MSMs at size on ALL-DISTINCT bases, and an exact reference that scales to them.

Discrete-log oracle.  When bases[i] = h_i * G for known h_i (G the generator of the order-r subgroup),

    sum_i s_i * bases[i] = ((sum_i s_i h_i) mod r) * G

for any 256-bit s_i and h_i: one integer dot product on the CPU (weighted_sum256) and ONE one-pair multiplication by the CPU oracle,
for any n.  Unlike the fold-by-tile reference of skew_cases.py -- which folds the scalars modulo the tile length D and therefore gives
the same point when entry i meets base j with j = i (mod D) -- every entry has a base of its own here, so any scalar that meets the
wrong base moves the sum (test_distinct_reference.py states both halves as tests).

The bases are made on the GPU by the fixed-base entry (device_bases): FixedBase shares no code with the MSM but the field
arithmetic, and its output is pinned to the oracle and the Python model by test_gpu_fixed_base.py.

Here: the dot product, the logs h_i (uniform, with planted rows: infinities, equal and opposite bases at the distances of the tile
lengths the other at-size tests use), the scalar generators, the expected point.  Nothing here needs a GPU to import."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import pymodel as pm

NAMES = {0: "bls12_377_g1", 1: "bls12_381_g1", 2: "bls12_377_g2", 3: "bls12_381_g2"}
BLOCK = 1 << 20          # rows per float64 product: BLOCK * (2^16 - 1)^2 < 2^52, so every partial sum is an exact integer below 2^53


def r_of(cid):
    return pm.CURVES[NAMES[cid]].r


def int_row(v):
    """v < 2^256 as 4 little-endian uint64 words"""
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64)


def row_int(row):
    return int.from_bytes(np.ascontiguousarray(row).tobytes(), "little")


def as_bytes(words):
    """(n, 4) uint64 -> uint8[n, 32], the scalar image the engine reads (a view)"""
    return np.ascontiguousarray(words).view(np.uint8).reshape(len(words), 32)


# ---------------------------------------------------------------------------------------------------------------------- dot product

def weighted_sum256(h_words, s_words):
    """sum_i h_i * s_i, exactly, for two (n, 4) uint64 little-endian arrays: 16-bit pieces, float64 products h16.T @ s16 over blocks of
    at most 2^20 rows (every entry of a block product is an integer below 2^20 * (2^16 - 1)^2 < 2^52, and so is every partial sum on
    the way: float64 holds them exactly in any summation order), the 16 x 16 block results added into a Python integer."""
    h_words, s_words = np.ascontiguousarray(h_words), np.ascontiguousarray(s_words)
    assert h_words.dtype == np.uint64 and s_words.dtype == np.uint64 and h_words.shape == s_words.shape and h_words.shape[1:] == (4,)
    total = 0
    for lo in range(0, len(h_words), BLOCK):
        h16 = h_words[lo:lo + BLOCK].view(np.uint16).reshape(-1, 16).astype(np.float64)
        s16 = s_words[lo:lo + BLOCK].view(np.uint16).reshape(-1, 16).astype(np.float64)
        m = h16.T @ s16
        assert m.max() < 2.0 ** 53
        for a in range(16):
            for b in range(16):
                total += int(m[a, b]) << (16 * (a + b))
    return total


# ---------------------------------------------------------------------------------------------------------------------- inputs

def _uniform(cid, n, rng):
    """uniform below r (top word below r's top word) as (n, 4) uint64"""
    w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    w[:, 3] %= np.uint64(r_of(cid) >> 192)
    return w


def planted_rows(n):
    """{label: row or (row i, row j)} of the rows make_logs plants in n logs: fixed fractions of min(n, 2^18), far apart, so that every
    prefix of 2^18 rows and more holds all of them but the far ends of the n // 2 pairs.  A pair is left out where its distance does not
    fit (n = 512 keeps the infinities, h = 1 and the n // 2 pairs)."""
    m = min(n, 1 << 18)
    rows = {"zero": m // 5, "r": 2 * m // 5, "one": 3 * m // 5 + 1}
    for k, (label, d) in enumerate((("2^12", 1 << 12), ("2^15", 1 << 15), ("half", n // 2))):
        for t, sign in enumerate(("equal", "opposite")):
            i = (2 * k + t + 1) * m // 13 + k
            if d and i + d < n:
                rows["%s %s" % (sign, label)] = (i, i + d)
    flat = [x for v in rows.values() for x in (v if isinstance(v, tuple) else (v,))]
    assert len(set(flat)) == len(flat) and max(flat) < n, rows
    return rows


def make_logs(cid, n, seed):
    """(h, planted): h_i as (n, 4) uint64, uniform below r, with the rows of planted_rows(n) set to 0 and r (infinity records), 1 (the
    generator itself) and to pairs h_j = h_i / h_j = r - h_i at distance exactly 2^12, 2^15 and n // 2 (equal and opposite bases: an
    addition of the two is a doubling or a cancellation)."""
    r = r_of(cid)
    h = _uniform(cid, n, np.random.default_rng([seed, cid, 0x109]))
    planted = planted_rows(n)
    for label, where in planted.items():
        if label == "zero":
            h[where] = 0
        elif label == "r":
            h[where] = int_row(r)
        elif label == "one":
            h[where] = int_row(1)
        else:
            i, j = where
            hi = row_int(h[i])
            assert 0 < hi < r
            h[j] = int_row(hi if label.startswith("equal") else r - hi)
    return h, planted


def planted_infinities(planted):
    return sum(1 for label in planted if label in ("zero", "r"))


KINDS = ("uniform", "any256", "hot")


def make_scalars(cid, n, seed, kind):
    """(n, 4) uint64.  "uniform": below r.  "any256": all 256 bits random.  "hot": uniform, but half the rows share one value -- a bucket
    of about n / 2 entries in every window, on distinct bases."""
    rng = np.random.default_rng([seed, cid, KINDS.index(kind)])
    if kind == "any256":
        return rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    s = _uniform(cid, n, rng)
    if kind == "hot":
        s[rng.random(n) < 0.5] = _uniform(cid, 1, rng)[0]
    return s


# ---------------------------------------------------------------------------------------------------------------------- reference

def oracle_mul(oracle, curve, img, ks):
    """[k * (the point of Affine image img) as a normalised Projective image] by one-pair oracle MSMs, k below 2^scalar_bits"""
    def one(k):
        assert 0 <= k < 1 << curve.scalar_bits
        out = ctypes.create_string_buffer(curve.projective_bytes)
        b = ctypes.create_string_buffer(img, len(img))
        s = ctypes.create_string_buffer(int(k).to_bytes(32, "little"), 32)
        assert oracle.oracle_msm(curve.curve_id, b, curve.affine_stride, s, 1, out, 1) == 0
        return out.raw
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(one, ks))


def generator_image(curve):
    return curve.encode_affine(curve.generator())


def expected(oracle, curve, logs, scalars):
    """sum_i scalars[i] * (logs[i] * G) as the normalised Projective image the engine returns: ((sum s_i h_i) mod r) * G by the oracle"""
    k = weighted_sum256(logs, scalars) % curve.r
    return oracle_mul(oracle, curve, generator_image(curve), [k])[0]


def affine_of_projective(curve, img):
    """normalised Projective image -> Affine image: the same coordinate bytes; (1, 1, 0) -> zeros with the flag set"""
    cb = curve.coord_bytes
    if img[2 * cb:] == bytes(cb):
        return bytes(2 * cb) + b"\x01" + bytes(7)
    return img[:2 * cb] + bytes(8)


def device_bases(ea, name, logs):
    """logs[i] * G as Affine images in a GPU tensor of shape (n, stride), made on the device by the fixed-base entry"""
    import torch

    curve = pm.CURVES[name]
    d = torch.from_numpy(as_bytes(logs).reshape(-1)).cuda()
    with ea.FixedBase.get_window_table(generator_image(curve), curve=name, expected_scalars=len(logs)) as table:
        out = table.msm(d)
    assert out.is_cuda and tuple(out.shape) == (len(logs), curve.affine_stride)
    return out
