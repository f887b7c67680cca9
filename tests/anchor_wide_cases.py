"""Host model of the signed-digit recoding with an anchored window (csrc/partition.hpp next_digit, csrc/partition_plan.hpp part_plan),
in plain Python integers, for tests/test_anchor_wide_model.py (CPU), tests/test_gpu_anchor_wide.py and tests/test_gpu_anchor_wide_paths.py
(GPU; the scalar lists of the latter are built at the end of this file).

recode(k, c, bits, wide) returns what the level-1 kernels emit for the 256-bit scalar k and what the host adds for it:

    entries   a list of (bucket set g, bucket index j in [1, 2^(c-1)], sign), at most one per digit window
    constant  the multiple of the base that the host adds for EVERY scalar (the anchored window's offset)

or None when the wide window refuses the scalar (a bit at or above `bits` is set: the engine repeats the chunk with wide off).
value(entries, constant, c, bits, wide) folds them the way the bucket reduction and HostTail::fold do: bucket (g, j) weighs j 2^(c g),
except the upper bucket set of a wide window, which shares the weight of the window below it and whose buckets weigh 2^(c-1) more."""

import random

R377 = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001
R381 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def windows_of(c):
    return (257 + c - 1) // c


def anchor_of(c, bits):
    """the last full window (the engine anchors it under option anchor = 2 whatever the gain)"""
    return bits // c - 1


def wide_fits(c, bits):
    a = anchor_of(c, bits)
    return a >= 0 and bits - (a + 1) * c == 1 and windows_of(c) == a + 2


def recode(k, c, bits=253, wide=True):
    assert 0 <= k < 1 << 256
    half, full = 1 << (c - 1), 1 << c
    a = anchor_of(c, bits)
    wide = wide and wide_fits(c, bits)
    if wide and k >> bits:
        return None
    entries, carry = [], 0
    for w in range(windows_of(c)):
        if wide and w == a:
            v = ((k >> (c * a)) & (2 * full - 1)) + carry          # c + 1 raw bits and the carry: [0, 2^(c+1)]
            s = v - full
            m = abs(s)
            assert m <= full
            if m:
                entries.append((a, m, s < 0) if m <= half else (a + 1, m - half, s < 0))
            carry = 0
            break                                                  # step a + 1 reads the same bits; nothing lies above
        v = ((k >> (c * w)) & (full - 1)) + carry
        if w == a:                                                 # the anchored window of round 6: relative to 2^(c-1), the chain ends
            s = v - half
            carry = 0
        else:
            s = v - full if v > half else v
            carry = 1 if v > half else 0
        if s:
            entries.append((w, abs(s), s < 0))
    assert carry == 0
    constant = (full if wide else half) << (c * a)
    return entries, constant


def value(entries, constant, c, bits=253, wide=True):
    a = anchor_of(c, bits)
    wide = wide and wide_fits(c, bits)
    half = 1 << (c - 1)
    total = constant
    for g, j, neg in entries:
        assert 1 <= j <= half and 0 <= g < windows_of(c)
        weight = (j + half) << (c * a) if (wide and g == a + 1) else j << (c * g)
        total += -weight if neg else weight
    return total


def edge_scalars(c, bits=253, r=R377):
    """the values of the issue, and the wide window's value on 0, 2^c, 2^(c+1) and its magnitude on 2^(c-1), 2^(c-1) + 1"""
    a = anchor_of(c, bits)
    full, half = 1 << c, 1 << (c - 1)
    top = 1 << bits
    vals = [0, 1, r - 1, r, (top >> 1) - 1, top >> 1, (top >> 1) + 1, top - 1]
    low = (1 << (c * a)) - 1
    for v in (0, full, 2 * full - 1, full - half, full + half, full - half - 1, full + half + 1, full - 1, full + 1):
        vals.append(v << (c * a))
        vals.append((v << (c * a)) | low)           # ... with a carry arriving: v + 1 (2^(c+1) for v = 2^(c+1) - 1)
        vals.append((v << (c * a)) | (low >> 1))    # ... and without one
    return [v for v in vals if v < top]


# ---- scalar lists for tests/test_gpu_anchor_wide_paths.py -----------------------------------------------------------------------------
def uniform_scalars(n, seed, r=R377):
    rng = random.Random(seed)
    return [rng.randrange(r) for _ in range(n)]


def planted_edges(c, n, seed, bits=253, r=R377):
    """edge_scalars(c) planted among n uniform canonical scalars (every fifth index from 3 on)"""
    vals = uniform_scalars(n, seed, r)
    planted = edge_scalars(c, bits, r)
    assert 3 + 5 * len(planted) < n
    for i, v in enumerate(planted):
        vals[3 + 5 * i] = v
    return vals


def equal_values(c, bits=253):
    """name -> the value every scalar of an all-equal list takes: the wide window's digit at its ends, on both sides of the two bucket sets"""
    a = anchor_of(c, bits)
    full, half = 1 << c, 1 << (c - 1)
    return {
        "zero": 0,                                             # every digit -2^c: the last bucket of the upper set holds -(sum of the bases)
        "upper_first": (full + half + 1) << (c * a),           # bucket 1 of the upper set, the lower set empty
        "lower_last": (full + half) << (c * a),                # the last bucket of the lower set, the upper set and R empty
        "no_entry": full << (c * a),                           # s = 0: no entry at all in the window
        "all_ones": (1 << bits) - 1,
    }


def bad_scalar(seed, bits=253):
    """a scalar with bit `bits` set: the wide window refuses it"""
    return (1 << bits) | random.Random(seed).randrange(1 << bits)


def entry_count(vals, c, wide, skip=(), bits=253):
    """non-zero digits the device groups for these scalars (bases at the indices `skip` are at infinity: no entries)"""
    memo = {}
    total = 0
    for i, v in enumerate(vals):
        if i in skip:
            continue
        if v not in memo:
            memo[v] = len(recode(v, c, bits, wide)[0])
        total += memo[v]
    return total


def montgomery_images(vals, r=R377, bit=253):
    """v 2^256 mod r for canonical v, every other one moved up by r or 2 r so that bit `bit` of the IMAGE is set (the value is the same)"""
    out = []
    for i, v in enumerate(vals):
        assert 0 <= v < r
        img = (v << 256) % r
        if i % 2 == 0:
            img += r if (img + r) >> bit & 1 else 2 * r
            assert img >> bit & 1 and img < 1 << 256
        out.append(img)
    return out
