"""Skewed and degenerate MSM inputs at production sizes, and an exact reference that scales to them.

Fold by tile.  When the bases are a tile of D points repeated T = n / D times (base i = Q_{i mod D}) and every tile point lies in the
order-r subgroup (or is the point at infinity),

    sum_i k_i P_i = sum_j s_j Q_j,    s_j = (sum_t k_{tD + j}) mod r,

for any 256-bit k_i.  The s_j are exact: the scalars are viewed as (T, D, 8) uint32 limbs, summed over T in uint64 (exact while
T < 2^32), and the eight column sums of each j are combined as Python integers.  The reference is then the CPU oracle over the D tile
points: O(n) NumPy and one small oracle call, for any n.

Also here: the scalar generators (seeded, uint8[n, 32]), the base tiles (random, one base, Q / -Q pairs) and a NumPy model of the engine's
signed digits (csrc/partition.hpp next_digit) that tells a test how long the hottest bucket and the longest level-1 segment of a run are,
so that coverage is asserted rather than assumed."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {0: "bls12_377_g1", 1: "bls12_381_g1", 2: "bls12_377_g2", 3: "bls12_381_g2"}
R = {0: 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001,
     1: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
P = {0: 0x1ae3a4617c510eac63b05c06ca1493b1a22d9f300f5138f1ef3622fba094800170b5d44300000008508c00000000001,
     1: 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab}
STRIDE = {0: 104, 1: 104, 2: 200, 3: 200}
PROJ = {0: 144, 1: 144, 2: 288, 3: 288}
COORD = {0: 48, 1: 48, 2: 96, 3: 96}


def r_of(cid):
    return R[cid & 1]


def scalar_bits(cid):
    return r_of(cid).bit_length()


def part_subjob():
    """PART_SUBJOB of csrc/partition_plan.hpp: entries per sub-job of a generic grouping pass (a longer segment is cut into sub-jobs)."""
    with open(os.path.join(ROOT, "2022-entries_amd", "csrc", "partition_plan.hpp")) as f:
        m = re.search(r"constexpr\s+uint32_t\s+PART_SUBJOB\s*=\s*(\d+)u?\s*<<\s*(\d+)\s*;", f.read())
    assert m, "PART_SUBJOB not found in partition_plan.hpp"
    return int(m.group(1)) << int(m.group(2))


# ---------------------------------------------------------------------------------------------------------------------- scalars

def _int_row(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)


def _uniform(cid, n, rng):
    """uniform below r (top limb below r's top limb), 4 x u64 LE as uint8[n, 32]"""
    limbs = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] %= np.uint64(r_of(cid) >> 192)
    return limbs.view(np.uint8).reshape(n, 32)


def all_equal(cid, n, seed):
    k = int.from_bytes(_uniform(cid, 1, np.random.default_rng(seed)).tobytes(), "little")
    return np.tile(_int_row(k), (n, 1))


def all_one(cid, n, seed):
    return np.tile(_int_row(1), (n, 1))


def all_zero(cid, n, seed):
    return np.zeros((n, 32), dtype=np.uint8)


def zeros_90(cid, n, seed):
    rng = np.random.default_rng(seed)
    sc = _uniform(cid, n, rng)
    sc[rng.random(n) < 0.9] = 0
    return sc


def witness(cid, n, seed):
    """0/1 values, 5 % uniform full-width: the shape of a prover's witness vector"""
    rng = np.random.default_rng(seed)
    sc = np.zeros((n, 32), dtype=np.uint8)
    sc[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint8)
    full = np.flatnonzero(rng.random(n) < 0.05)
    sc[full] = _uniform(cid, len(full), rng)
    return sc


def short64(cid, n, seed):
    sc = np.zeros((n, 32), dtype=np.uint8)
    sc[:, :8] = np.random.default_rng(seed).integers(0, 256, size=(n, 8), dtype=np.uint8)
    return sc


def top_only(cid, n, seed):
    """only the top 8 significant bits may be set (values stay below r)"""
    sh = scalar_bits(cid) - 8
    t = np.random.default_rng(seed).integers(0, r_of(cid) >> sh, size=n, dtype=np.uint64)
    limbs = np.zeros((n, 4), dtype=np.uint64)
    limbs[:, sh // 64] = t << np.uint64(sh % 64)
    if sh % 64 > 56:   # (the byte straddles two limbs)
        limbs[:, sh // 64 + 1] = t >> np.uint64(64 - sh % 64)
    return limbs.view(np.uint8).reshape(n, 32)


def two_values(cid, n, seed):
    rng = np.random.default_rng(seed)
    ab = _uniform(cid, 2, rng)
    return np.ascontiguousarray(ab[rng.integers(0, 2, size=n)])


def r_minus_1(cid, n, seed):
    return np.tile(_int_row(r_of(cid) - 1), (n, 1))


def window_periodic(cid, n, seed, c):
    """the same positive digit d < 2^(c-1) in every window of size c below bit scalar_bits - 1 (so the value stays below r): one hot
    bucket in every window, and with shared table levels one bucket for them all"""
    d = int(np.random.default_rng(seed).integers(1, 1 << (c - 1)))
    k = sum(d << (c * w) for w in range((scalar_bits(cid) - 1) // c))
    return np.tile(_int_row(k), (n, 1))


GENERATORS = {f.__name__: f for f in (all_equal, all_one, all_zero, zeros_90, witness, short64, top_only, two_values, r_minus_1)}


def make_scalars(name, cid, n, seed, c=None):
    """generator `name` ("window_periodic" needs the window size c)"""
    sc = window_periodic(cid, n, seed, c) if name == "window_periodic" else GENERATORS[name](cid, n, seed)
    assert sc.shape == (n, 32) and sc.dtype == np.uint8
    return np.ascontiguousarray(sc)


# ---------------------------------------------------------------------------------------------------------------------- bases

def negate(cid, pts):
    """-Q of affine byte images (uint8[D, stride]): y -> p - y per Fp component (Montgomery form is linear); infinity stays"""
    out = np.array(pts, copy=True)
    cb, p = COORD[cid], P[cid & 1]
    for i in range(len(out)):
        if out[i, 2 * cb]:
            continue
        for off in range(cb, 2 * cb, 48):
            y = int.from_bytes(out[i, off:off + 48].tobytes(), "little")
            out[i, off:off + 48] = np.frombuffer(((p - y) % p).to_bytes(48, "little"), dtype=np.uint8)
    return out


def random_tile(ea, cid, D, seed, infinity_at=None):
    tile = ea.generate_points(D, distinct=D, seed=seed, curve=NAMES[cid])
    if infinity_at is not None:
        tile[infinity_at, :] = 0
        tile[infinity_at, 2 * COORD[cid]] = 1
    return tile


def same_base_tile(ea, cid, seed):
    return random_tile(ea, cid, 1, seed)


def cancel_tile(ea, cid, seed, pairs=1):
    """[Q_0, -Q_0, Q_1, -Q_1, ...]: with scalars equal within each pair (cancel_scalars) the MSM is the point at infinity"""
    q = random_tile(ea, cid, pairs, seed)
    t = np.empty((2 * pairs, STRIDE[cid]), dtype=np.uint8)
    t[0::2], t[1::2] = q, negate(cid, q)
    return t


def cancel_scalars(sc):
    """make the scalars equal within each (2m, 2m + 1) pair"""
    sc = np.array(sc, copy=True)
    sc[1::2] = sc[0::2][: len(sc[1::2])]
    return sc


def expand(tile, n):
    """base i = tile[i mod D] on the host (small n only: the GPU tests repeat the tile on the device)"""
    return np.ascontiguousarray(np.tile(tile, (n // len(tile), 1)))


# ---------------------------------------------------------------------------------------------------------------------- reference

def fold_scalars(cid, scalars, D):
    """s_j = (sum_t k_{tD + j}) mod r as uint8[D, 32], exact for any 256-bit k"""
    n = len(scalars)
    assert n % D == 0 and n // D < (1 << 32)
    cols = np.ascontiguousarray(scalars).view(np.uint32).reshape(n // D, D, 8).sum(axis=0, dtype=np.uint64)
    r = r_of(cid)
    out = np.zeros((D, 32), dtype=np.uint8)
    for j in range(D):
        s = sum(int(cols[j, l]) << (32 * l) for l in range(8)) % r
        out[j] = _int_row(s)
    return out


def oracle_msm(oracle, cid, bases, scalars, threads=0):
    bases, scalars = np.ascontiguousarray(bases), np.ascontiguousarray(scalars)
    assert len(bases) == len(scalars)
    out = ctypes.create_string_buffer(PROJ[cid])
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert oracle.oracle_msm(cid, vp(bases.ctypes.data), sz(STRIDE[cid]), vp(scalars.ctypes.data), sz(len(scalars)), out, threads) == 0
    return out.raw


def fold_reference(oracle, cid, tile, scalars):
    """sum_i k_i tile[i mod D], computed as the oracle's MSM of the D tile points by their folded scalars"""
    return oracle_msm(oracle, cid, tile, fold_scalars(cid, scalars, len(tile)))


# ---------------------------------------------------------------------------------------------------------------------- coverage

def anchor_window(c, bits):
    """the engine's anchored window for window size c (msm_engine.hip anchor_window, option anchor = 1); None: plain digits only"""
    full, rem = bits // c, bits % c
    if full < 1:
        return None
    q = 0.857 if bits == 253 else 0.552
    top_clear = 1.0 if rem == 0 else min(1.0, q * 2.0 ** (1 - rem))
    plain = full + (1.0 - q if rem == 0 else 1.0 - 0.5 * top_clear)
    anchored = full + (1.0 - top_clear)
    return full - 1 if plain - anchored >= 0.01 * plain else None


def digits(scalars, c, anchor=None):
    """magnitudes of the engine's signed digits (partition.hpp next_digit, plain form; `anchor`: the window taken relative to 2^(c-1),
    which ends the carry chain) as uint32[windows, n]"""
    n = len(scalars)
    windows = (257 + c - 1) // c
    limbs = np.zeros((n, 5), dtype=np.uint64)   # one zero limb above, for the windows that cross bit 256
    limbs[:, :4] = np.ascontiguousarray(scalars).view(np.uint64).reshape(n, 4)
    half, full = 1 << (c - 1), 1 << c
    mag = np.empty((windows, n), dtype=np.uint32)
    carry = np.zeros(n, dtype=np.int32)
    for w in range(windows):
        o = w * c
        l, sh = o // 64, o % 64
        u = limbs[:, l] >> np.uint64(sh)
        if sh + c > 64:
            u |= limbs[:, l + 1] << np.uint64(64 - sh)
        v = (u & np.uint64(full - 1)).astype(np.int32) + carry
        if w == anchor:
            m = np.abs(v - half)
            carry = np.zeros(n, dtype=np.int32)
        else:
            neg = v > half
            m = np.where(neg, full - v, v)
            carry = neg.astype(np.int32)
        mag[w] = m
    return mag


def hot_spots(scalars, c, bucket_sets, l1_bits, anchor=None):
    """(entries of the hottest bucket, entries of the longest level-1 segment, all entries) of one chunk: window w feeds bucket set
    w mod bucket_sets (precomputed table levels share sets), bucket = magnitude - 1, a level-1 segment = the buckets that share their
    top l1_bits bits (csrc/partition_plan.hpp).  A bucket lies inside one segment of every grouping level, so its entries are a lower bound of the
    longest segment of every pass."""
    mag = digits(scalars, c, anchor)
    half, lb = 1 << (c - 1), (c - 1) - l1_bits
    counts = np.zeros((bucket_sets, half + 1), dtype=np.int64)
    for w in range(mag.shape[0]):
        counts[w % bucket_sets] += np.bincount(mag[w], minlength=half + 1)   # (magnitudes are <= 2^(c-1))
    entries = int(counts[:, 1:].sum())
    counts = counts[:, 1:]   # bucket = magnitude - 1; magnitude 0 is no entry
    segs = counts.reshape(bucket_sets, half >> lb, 1 << lb).sum(axis=2)
    return int(counts.max()), int(segs.max()), entries
