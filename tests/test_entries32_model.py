"""CPU: the Entries32 format of the sorted entry stream (csrc/msm_types.hpp), a Python model of its writer and reader against the
format's own helpers compiled for the host (libmsm_hosttest.so, ht_e32_encode / ht_e32_decode).

An entry is one 32-bit word: bits 25..0 the base index, 30..26 the key's step from the entry before (0 same key, 1..30 that many
buckets on, 31 = the key stands in run_keys[position]), bit 31 the sign.  run_keys is sparse: escapes (the first run of a grouping
segment, a gap above 30 buckets, every run start of a segment cut into sub-jobs) and every multiple of the lane length K."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import ROOT

UNWRITTEN = 0xFFFFFFFF
IDX_BITS, ESCAPE, MAX_STEP = 26, 31, 30


# ---- the model ------------------------------------------------------------------------------------------------------------------
def encode(keys, values, K, seg_keys, seg_subjobs=None):
    """keys sorted; segment s holds the keys [seg_keys[s], seg_keys[s + 1]).  Returns (words, {position: key})."""
    words, run_keys = [], {}
    prev_seg = None
    for i, (k, v) in enumerate(zip(keys, values)):
        seg = max(s for s in range(len(seg_keys)) if seg_keys[s] <= k)
        step = 0
        if i == 0 or k != keys[i - 1]:
            gap = k - keys[i - 1] if i else None
            if seg != prev_seg or gap > MAX_STEP or (seg_subjobs and seg_subjobs[seg]):
                step = ESCAPE
                run_keys[i] = k
            else:
                step = gap
            prev_seg = seg
        assert v & 0x7FFFFFFF < 1 << IDX_BITS
        words.append((v & 0x80000000) | (v & ((1 << IDX_BITS) - 1)) | (step << IDX_BITS))
    for q in range(0, len(keys), K):
        run_keys[q] = keys[q]
    return words, run_keys


def decode(words, run_keys, K):
    """The accumulation's walk: lane t starts from run_keys[t K].  Returns (keys, values, continued per lane)."""
    keys, values, cont = [], [], []
    for beg in range(0, len(words), K):
        cur = run_keys[beg]
        cont.append((words[beg] >> IDX_BITS) & 31 == 0)
        for i in range(beg, min(beg + K, len(words))):
            step = (words[i] >> IDX_BITS) & 31
            if i > beg:
                cur = run_keys[i] if step == ESCAPE else cur + step
            keys.append(cur)
            values.append(words[i] & (0x80000000 | ((1 << IDX_BITS) - 1)))
    return keys, values, cont


# ---- the compiled helpers --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ht(built):
    lib = ctypes.CDLL(os.path.join(ROOT, "2022-entries_amd", "libmsm_hosttest.so"))
    lib.ht_e32_encode.restype = ctypes.c_long
    lib.ht_e32_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                  ctypes.c_void_p, ctypes.c_void_p]
    lib.ht_e32_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ht_e32_run_keys_offset.restype = ctypes.c_uint32
    lib.ht_e32_run_keys_offset.argtypes = [ctypes.c_uint64]
    lib.ht_e32_applies.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    return lib


def native(ht, keys, values, K, seg_keys, seg_subjobs=None):
    n = len(keys)
    k = np.array(keys, dtype=np.uint32)
    v = np.array(values, dtype=np.uint32)
    sk = np.array(seg_keys, dtype=np.uint32)
    sj = np.array(seg_subjobs if seg_subjobs else [0] * len(seg_keys), dtype=np.uint8)
    words = np.zeros(max(n, 1), dtype=np.uint32)
    rk = np.full(max(n, 1), UNWRITTEN, dtype=np.uint32)
    esc = ht.ht_e32_encode(k.ctypes.data, v.ctypes.data, n, K, sk.ctypes.data, sj.ctypes.data, len(seg_keys), words.ctypes.data, rk.ctypes.data)
    assert esc >= 0
    ko = np.zeros(max(n, 1), dtype=np.uint32)
    vo = np.zeros(max(n, 1), dtype=np.uint32)
    cont = np.zeros(n // K + 1, dtype=np.uint8)
    assert ht.ht_e32_decode(words.ctypes.data, rk.ctypes.data, n, K, ko.ctypes.data, vo.ctypes.data, cont.ctypes.data) == 0
    lanes = (n + K - 1) // K
    return (esc, [int(x) for x in words[:n]], {i: int(rk[i]) for i in range(n) if rk[i] != UNWRITTEN}, [int(x) for x in ko[:n]], [int(x) for x in vo[:n]],
            [bool(x) for x in cont[:lanes]])


def check(ht, keys, K, seg_keys, seg_subjobs=None, seed=0):
    rng = random.Random(seed)
    values = [rng.randrange(1 << IDX_BITS) | (rng.randrange(2) << 31) for _ in keys]
    words, run_keys = encode(keys, values, K, seg_keys, seg_subjobs)
    dk, dv, cont = decode(words, run_keys, K)
    assert dk == list(keys) and dv == values
    # "continues the previous lane's bucket" is what the 64-bit format finds by comparing with the entry before the lane
    assert cont == [t > 0 and keys[t * K] == keys[t * K - 1] for t in range(len(cont))]
    esc, n_words, n_rk, n_keys, n_vals, n_cont = native(ht, keys, values, K, seg_keys, seg_subjobs)
    assert n_words == words and n_rk == run_keys and n_keys == dk and n_vals == dv and n_cont == cont
    assert esc == sum(1 for w in words if (w >> IDX_BITS) & 31 == ESCAPE)
    return words, run_keys


def steps(words):
    return [(w >> IDX_BITS) & 31 for w in words]


# ---- the edges ------------------------------------------------------------------------------------------------------------------
def test_gaps_of_1_29_30_31_32_buckets(ht):
    keys, k = [], 5
    for gap in (1, 29, 30, 31, 32):
        keys += [k, k]
        k += gap
    keys += [k]
    words, run_keys = check(ht, keys, 1 << 20, [0])
    assert steps(words) == [31, 0, 1, 0, 29, 0, 30, 0, 31, 0, 31]     # the segment's first run, then the gaps; above 30 the key is stored
    assert run_keys == {0: 5, 8: 5 + 1 + 29 + 30 + 31, 10: 5 + 1 + 29 + 30 + 31 + 32}


def test_a_run_that_starts_exactly_on_a_lane_start(ht):
    keys = [3] * 4 + [4] * 4 + [9] * 3
    words, run_keys = check(ht, keys, 4, [0])
    assert steps(words)[4] == 1 and run_keys[4] == 4 and run_keys[8] == 9     # the step stays, the key is stored as well
    assert set(run_keys) == {0, 4, 8}


def test_a_run_that_spans_three_lanes(ht):
    keys = [7] * 2 + [8] * 11 + [40]
    words, run_keys = check(ht, keys, 4, [0])
    assert run_keys[4] == run_keys[8] == 8 and steps(words)[4] == steps(words)[8] == 0      # lanes 1 and 2 continue bucket 8
    assert run_keys[12] == 8 and run_keys[13] == 40                                        # ... lane 3 too; then a gap of 32


def test_a_segment_whose_first_bin_is_empty(ht):
    # segments of 16 keys; the second one starts at key 16 but its first entry is key 19 -- one bucket after the previous segment's last
    keys = [14, 15, 15, 19, 20, 20, 33]
    words, run_keys = check(ht, keys, 1 << 20, [0, 16, 32])
    assert steps(words) == [31, 1, 0, 31, 1, 0, 31]
    assert run_keys == {0: 14, 3: 19, 6: 33}


def test_a_segment_cut_into_sub_jobs_escapes_every_run_start(ht):
    keys = [0, 0, 1, 2, 2, 16, 17]
    words, run_keys = check(ht, keys, 1 << 20, [0, 16], [1, 0])
    assert steps(words) == [31, 0, 31, 31, 0, 31, 1]
    assert run_keys == {0: 0, 2: 1, 3: 2, 5: 16}


def test_a_single_entry_and_none(ht):
    words, run_keys = check(ht, [123456], 8, [0])
    assert steps(words) == [31] and run_keys == {0: 123456}
    words, run_keys = check(ht, [], 8, [0])
    assert words == [] and run_keys == {}


@pytest.mark.parametrize("K", [4, 8, 24, 512])
def test_random_streams(ht, K):
    rng = random.Random(K)
    for trial in range(20):
        nseg = rng.randrange(1, 6)
        seg_keys = [64 * s for s in range(nseg)]
        n = rng.randrange(0, 6 * K + 3)
        density = rng.choice([2, 40, 400])
        keys = sorted(rng.randrange(64 * nseg) // rng.choice([1, density]) for _ in range(n))
        subjobs = [rng.randrange(4) == 0 for _ in range(nseg)]
        check(ht, keys, K, seg_keys, subjobs, seed=trial)


def test_geometry_helpers(ht):
    for cap in (0, 1, 15, 16, 17, 1 << 14, 13 * (1 << 26), 12 * (1 << 26) + 5):
        off = ht.ht_e32_run_keys_offset(cap)
        assert off % 16 == 0 and off >= cap + 16          # behind the words and 64 bytes of slack
        assert 4 * (off + cap) <= 8 * cap + 128           # ... and run_keys still ends inside a buffer of `cap` 64-bit entries + 128 bytes
    assert ht.ht_e32_applies(0, 1 << 26, 1) == 1 and ht.ht_e32_applies(0, 1 << 26, 0) == 1
    assert ht.ht_e32_applies(1, 1 << 26, 1) == 0 and ht.ht_e32_applies(0, (1 << 26) + 1, 1) == 0
    assert ht.ht_e32_applies((1 << 26) - 5, 5, 1) == 1 and ht.ht_e32_applies(0, 1024, 2) == 0
