"""Integer models and case generators for the tests of csrc/lookup.hpp (resident lookup tables over Fr, plookup's sorted vector and the
logUp running sum), next to the helpers of ntt_cases.py.  Nothing here comes from the code under test and nothing needs a GPU to
import.  The contract is stated on integers: two 256-bit patterns match when they are equal modulo r, so the model is a dict from
residue to first index, a list of counts, s by list expansion, and logUp in Python integers."""
import functools
import random

import ntt_cases as nc

NONE = 0xFFFFFFFF


def rows(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def raw_bytes(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def model_count(field, table_raw, values_raw):
    """(index, counts, missing, first_missing) of the raw patterns, whatever form they are read in"""
    r = nc.modulus(field)
    first = {}
    for i, t in enumerate(rows(table_raw)):
        first.setdefault(t % r, i)
    index = [first.get(v % r, NONE) for v in rows(values_raw)]
    counts = [0] * (len(table_raw) // 32)
    for i in index:
        if i != NONE:
            counts[i] += 1
    gone = [j for j, i in enumerate(index) if i == NONE]
    return index, counts, len(gone), gone[0] if gone else len(index)


def model_mult(field, counts, normal):
    return nc.encode(field, counts, normal)


def model_sorted(field, table_raw, counts):
    r = nc.modulus(field)
    out = []
    for t, c in zip(rows(table_raw), counts):
        out += [t % r] * (1 + c)
    return raw_bytes(out)


def model_logup(field, table_raw, mult_raw, values_raw, m, stride, n, beta_raw, normal):
    """(out, total, helpers) as bytes: values_raw holds m columns stride elements apart"""
    r = nc.modulus(field)
    inv = lambda x: pow(x, r - 2, r)   # (0 stays 0)
    t, mu, v = nc.decode(field, table_raw, normal), nc.decode(field, mult_raw, normal), nc.decode(field, values_raw, normal)
    beta = nc.decode(field, beta_raw, normal)[0]
    cols = [[inv((beta + v[c * stride + j]) % r) for j in range(n)] for c in range(m)]
    cols.append([mu[j] * inv((beta + t[j]) % r) % r for j in range(n)])
    out, acc = [], 0
    for j in range(n):
        out.append(acc)
        acc = (acc + sum(cols[c][j] for c in range(m)) - cols[m][j]) % r
    return nc.encode(field, out, normal), nc.encode(field, [acc], normal), nc.encode(field, [x for col in cols for x in col], normal)


class Case:
    def __init__(self, name, field, normal, table, values):
        self.name, self.field, self.normal = name, field, normal
        self.table_raw = table if isinstance(table, bytes) else raw_bytes(table)
        self.values_raw = values if isinstance(values, bytes) else raw_bytes(values)
        self.n_t, self.n_f = len(self.table_raw) // 32, len(self.values_raw) // 32

    @functools.cached_property
    def expected(self):
        index, counts, missing, first = model_count(self.field, self.table_raw, self.values_raw)
        return {"index": index, "counts": counts, "missing": missing, "first": first, "mult": model_mult(self.field, counts, self.normal),
                "sorted": model_sorted(self.field, self.table_raw, counts) if missing == 0 else None}


def distinct_table(field, n, rng):
    """n raw patterns with distinct residues, a few of them above r"""
    r = nc.modulus(field)
    res = set()
    while len(res) < n:
        res.add(rng.randrange(r))
    out = []
    for v in res:
        k = rng.randrange(4)
        out.append(v + r if k == 0 and v + r < (1 << 256) else v)
    rng.shuffle(out)
    return out


def distinct_small(n, bits, rng):
    """n distinct non-zero integers below 2^bits, in a random order"""
    seen = {}
    while len(seen) < n:
        seen.setdefault(1 + rng.getrandbits(bits) % ((1 << bits) - 1), None)
    return list(seen)


def draw(table, n, rng):
    return [table[rng.randrange(len(table))] for _ in range(n)]


@functools.lru_cache(maxsize=None)
def cases(field, normal):
    """every small case of the issue's list, by name; built once per (field, form)"""
    rng = random.Random("lookup %s %d" % (field, normal))
    r = nc.modulus(field)
    out = []

    def add(name, table, values):
        out.append(Case(name, field, normal, table, values))

    one = distinct_table(field, 1, rng)
    for n_f in (0, 1, 65):
        add("nt1_nf%d" % n_f, one, one * n_f)
    for n_t in (32, 33):   # slots 64 and 128
        t = distinct_table(field, n_t, rng)
        add("nt%d" % n_t, t, draw(t, 100, rng))
    t = distinct_table(field, (1 << 16) + 1, rng)
    add("block_edges", t, draw(t, (1 << 16) + 3, rng))
    # duplicates
    base = distinct_table(field, 40, rng)
    t = base + [base[3], base[17], base[3], base[39], base[0]]
    rng.shuffle(t)
    add("dup_scattered", t, draw(t, 300, rng))
    add("dup_1000_equal", [base[5]] * 1000, [base[5]] * 77)
    # residues: v against v + r (and v + 2r where it fits)
    small = [rng.getrandbits(200) for _ in range(24)]
    add("table_v_values_v_plus_r", small, [v + r for v in draw(small, 90, rng)])
    add("table_v_plus_r_values_v", [v + r for v in small], draw(small, 90, rng))
    if field == "bls12_381":
        add("values_v_plus_2r", small, [v + 2 * r for v in draw(small, 90, rng)])
        add("table_v_plus_2r", [v + 2 * r if i % 2 else v + r for i, v in enumerate(small)], draw(small, 90, rng))
    # every multiple that fits 256 bits: up to 2r for BLS12-381, up to 13r for BLS12-377 (r has 253 bits)
    kmax = ((1 << 256) - (1 << 200)) // r
    for k in sorted({2, 8, kmax} & set(range(1, kmax + 1))):
        add("values_v_plus_%dr" % k if k != 2 or field != "bls12_381" else "values_v_plus_2r_again", small, [v + k * r for v in draw(small, 90, rng)])
        add("table_v_plus_%dr_values_v" % k, [v + k * r for v in small], draw(small, 90, rng))
    add("table_and_values_every_multiple", [v + (i % (kmax + 1)) * r for i, v in enumerate(small)],
        [v + rng.randrange(kmax + 1) * r for v in draw(small, 300, rng)])
    wild = [rng.getrandbits(256) for _ in range(200)] + [(1 << 256) - 1, (1 << 256) - 1 - r, kmax * r, kmax * r - 1, (kmax + 1) * r - 1 if (kmax + 1) * r - 1 < (1 << 256) else r - 1]
    add("any_256_bit_pattern_against_its_residue", wild, [v % r for v in draw(wild, 400, rng)])
    add("residues_against_any_256_bit_pattern", [v % r for v in wild], draw(wild, 400, rng))
    add("one_residue_every_multiple", [small[0] + k * r for k in range(kmax + 1)], [small[0] + k * r for k in range(kmax, -1, -1)] * 3)
    # missing values
    t = distinct_table(field, 200, rng)
    inside, outside = t[:150], t[150:]
    v = draw(inside, 500, rng)
    add("missing_none", inside, v)
    add("missing_first", inside, [outside[0]] + v[1:])
    add("missing_last", inside, v[:-1] + [outside[1]])
    many = list(v)
    for j in rng.sample(range(7, 500), 120):
        many[j] = outside[rng.randrange(len(outside))]
    add("missing_many", inside, many)
    # skew
    t = distinct_table(field, 1 << 10, rng)
    for name, at in (("first", 0), ("last", len(t) - 1), ("middle", 517)):
        add("skew_all_on_%s" % name, t, [t[at]] * (1 << 16))
    half = [t[9] if rng.randrange(2) else t[rng.randrange(len(t))] for _ in range(1 << 16)]
    add("skew_half_padding", t, half)
    add("range_table", nc.encode(field, range(1 << 12), normal), nc.encode(field, [rng.randrange(1 << 12) for _ in range(1 << 14)], normal))
    return {c.name: c for c in out}


def medium_case(field, normal, seed=5):
    """2^20 uniform values into 2^16 distinct entries as NumPy arrays of canonical rows (top word below 2^28, so below r)"""
    import numpy as np
    g = np.random.default_rng(seed + nc.FIELD_IDS[field])
    table = g.integers(0, 1 << 32, size=(1 << 16, 8), dtype=np.uint64).astype(np.uint32)
    table[:, 7] &= (1 << 28) - 1
    table[:, 0] = np.arange(1 << 16, dtype=np.uint32)   # distinct
    table = table[g.permutation(1 << 16)]
    pick = g.integers(0, 1 << 16, size=1 << 20)
    return table, table[pick], pick


def logup_case(field, normal, n, m, stride, seed, zero_den=False):
    """a table of n rows, m columns of n values drawn from it (stride elements apart, the gaps filled with noise), the multiplicities of
    the model and a beta; with zero_den, beta = -table[3]"""
    rng = random.Random("logup %s %d %d %d %d %d" % (field, normal, n, m, stride, seed))
    r = nc.modulus(field)
    t = distinct_small(n, 64, rng)
    cols = [[t[rng.randrange(n)] for _ in range(n)] + [rng.getrandbits(250) for _ in range(stride - n)] for _ in range(m)]
    counts = [0] * n
    pos = {v: i for i, v in enumerate(t)}
    for col in cols:
        for v in col[:n]:
            counts[pos[v]] += 1
    beta = (r - t[3]) % r if zero_den and n > 3 else rng.randrange(r)
    flat = [x for col in cols for x in col][:(m - 1) * stride + n]
    return {"table": nc.encode(field, t, normal), "mult": nc.encode(field, counts, normal), "values": nc.encode(field, flat, normal),
            "beta": nc.encode(field, [beta], normal), "counts": counts}
