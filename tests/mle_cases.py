"""Big-integer models and case lists for the tests of csrc/mle.hpp (dense multilinear extensions and sumcheck prover rounds over Fr),
next to the helpers of ntt_cases.py.  Nothing here comes from the code under test and nothing needs a GPU to import.

Index b of a table of 2^nv values is the point (b_0, .., b_{nv-1}) with b_0 the lowest bit; variables are fixed from x_1 (the lowest
bit) upward, out[b] = in[2b] + r (in[2b+1] - in[2b]) -- ark-poly's DenseMultilinearExtension::fix_variables.  A term list is a list of
(coefficient, [table indices]); g = sum_j c_j prod_{k in S_j} f_k, the ListOfProductsOfPolynomials of ark-linear-sumcheck."""
import hashlib
import random

import ntt_cases as nc

MAX_TABLES, MAX_TERMS, MAX_FACTORS = 12, 8, 5


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def fix_variables(r, table, point):
    t = [v % r for v in table]
    for p in point:
        t = [(t[2 * b] + p * (t[2 * b + 1] - t[2 * b])) % r for b in range(len(t) // 2)]
    return t


def evaluate(r, table, point):
    assert len(table) == 1 << len(point)
    return fix_variables(r, table, point)[0]


def eq_table(r, point):
    out = []
    for b in range(1 << len(point)):
        v = 1
        for i, p in enumerate(point):
            v = v * (p if (b >> i) & 1 else 1 - p) % r
        out.append(v)
    return out


def degree(terms):
    return max(len(f) for _, f in terms)


def round_evals(r, tables, terms):
    """P(t) = sum_b sum_j c_j prod_k (f_k[2b] + t (f_k[2b+1] - f_k[2b])) for t = 0 .. d"""
    out = []
    for t in range(degree(terms) + 1):
        s = 0
        for b in range(len(tables[0]) // 2):
            for c, fs in terms:
                v = c
                for k in fs:
                    v = v * (tables[k][2 * b] + t * (tables[k][2 * b + 1] - tables[k][2 * b])) % r
                s += v
        out.append(s % r)
    return out


def hypercube_sum(r, tables, terms):
    s = 0
    for b in range(len(tables[0])):
        for c, fs in terms:
            v = c
            for k in fs:
                v = v * tables[k][b] % r
            s += v
    return s % r


def g_at(r, terms, values):
    """sum_j c_j prod_k values[k]"""
    s = 0
    for c, fs in terms:
        v = c
        for k in fs:
            v = v * values[k] % r
        s += v
    return s % r


def interpolate(r, evals, x):
    """the polynomial of degree len(evals) - 1 through (t, evals[t]), at x"""
    s = 0
    for i, yi in enumerate(evals):
        num, den = 1, 1
        for j in range(len(evals)):
            if j != i:
                num = num * (x - j) % r
                den = den * (i - j) % r
        s += yi * num * pow(den, -1, r)
    return s % r


def verify(r, claim, rounds, point, finals, terms):
    """the verifier of the sumcheck protocol: the list of failed checks (empty = accept)"""
    bad = []
    expect = claim % r
    for i, (ev, x) in enumerate(zip(rounds, point)):
        if (ev[0] + ev[1]) % r != expect:
            bad.append("round %d: P(0) + P(1) differs from the claim" % i)
        expect = interpolate(r, ev, x)
    if g_at(r, terms, finals) != expect:
        bad.append("the last value differs from g(f_k(r))")
    return bad


def hash_challenge(r, seed):
    """challenge(i, evals) from a seeded hash of the round evaluations"""
    def challenge(i, evals):
        h = hashlib.sha256(b"%d|%d|" % (seed, i) + b"".join(int(e).to_bytes(32, "little") for e in evals)).digest()
        return int.from_bytes(h + hashlib.sha256(h).digest(), "little") % r
    return challenge


# ---- raw inputs -----------------------------------------------------------------------------------------------------------------------

def specials(field):
    r = nc.modulus(field)
    return [0, 1, r - 1, r, 2 * r, (1 << 256) - 1]


def raw_values(field, n, rng, only=None):
    """n raw 256-bit patterns: `only` everywhere, or a quarter from 0, 1, r - 1, r, 2r, 2^256 - 1 and the rest random bytes"""
    if only is not None:
        return [only] * n
    sp = specials(field)
    return [sp[rng.randrange(len(sp))] if rng.randrange(4) == 0 else rng.getrandbits(256) for _ in range(n)]


def raw_bytes(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def fills(field):
    """(name, only): random values with the special patterns among them, all r - 1, zeros, and the patterns r, 2r and 2^256 - 1"""
    r = nc.modulus(field)
    return [("random", None), ("all r - 1", r - 1), ("zeros", 0), ("the pattern r", r), ("the pattern 2r", 2 * r), ("the pattern 2^256 - 1", (1 << 256) - 1)]


# ---- term lists -----------------------------------------------------------------------------------------------------------------------

def term_lists(field, rng):
    """name -> (number of tables, [(coefficient, factors)]); coefficients are residues"""
    r = nc.modulus(field)
    c = lambda: rng.randrange(r)
    return {
        "one table of degree 1": (1, [(1, [0])]),
        # eq (a b - c): tables eq, a, b, c
        "spartan": (4, [(1, [0, 1, 2]), (r - 1, [0, 3])]),
        # vanilla HyperPlonk's gate qL a + qR b + qM a b - qO c + qC over the tables qL qR qM qO qC a b c and a ninth (eq) on every term
        "hyperplonk": (9, [(1, [8, 0, 5]), (1, [8, 1, 6]), (1, [8, 2, 5, 6]), (r - 1, [8, 3, 7]), (1, [8, 4])]),
        # 8 terms of 5 factors over 12 tables, one a fifth power
        "worst": (12, [(c(), [0, 0, 0, 0, 0]), (c(), [1, 2, 3, 4, 5]), (r - 1, [6, 7, 8, 9, 10]), (c(), [11, 0, 1, 2, 3]), (c(), [4, 4, 5, 5, 6]),
                       (c(), [7, 8, 9, 10, 11]), (1, [11, 10, 9, 8, 7]), (c(), [6, 5, 4, 3, 11])]),
    }


class RoundCase:
    """m tables of 2^nv raw patterns, a term list with raw coefficients, and a raw challenge for the fused round"""

    def __init__(self, field, name, nv, rng, only=None):
        self.field, self.name, self.nv = field, name, nv
        self.m, terms = term_lists(field, rng)[name]
        self.tables = [raw_values(field, 1 << nv, rng, only) for _ in range(self.m)]
        self.coeffs = [cf for cf, _ in terms]            # residues, given to the call in its form
        self.factors = [list(fs) for _, fs in terms]
        self.r_prev = raw_values(field, 1, rng, only)[0]

    def decoded(self, normal):
        return [nc.decode(self.field, raw_bytes(t), normal) for t in self.tables]

    def terms(self):
        return list(zip(self.coeffs, self.factors))

    def expected(self, normal, fused):
        """(round evaluations as residues, folded tables as bytes or None)"""
        r = nc.modulus(self.field)
        tabs = self.decoded(normal)
        if not fused:
            return round_evals(r, tabs, self.terms()), None
        rp = nc.decode(self.field, raw_bytes([self.r_prev]), normal)[0]
        folded = [fix_variables(r, t, [rp]) for t in tabs]
        return round_evals(r, folded, self.terms()), [nc.encode(self.field, f, normal) for f in folded]


def fix_cases(tile_log):
    """(num_vars, k) for a tile of 2^tile_log: num_vars 0, 1, 2, one below, at and one above the tile; k = 0, 1, tile_log,
    tile_log + 1, 2 tile_log + 1 and num_vars, so that one, two and three passes and the ping-pong run"""
    out = set()
    for nv in (0, 1, 2, tile_log - 1, tile_log, tile_log + 1):
        for k in (0, 1, tile_log, tile_log + 1, nv):
            if k <= nv:
                out.add((nv, k))
    big = 2 * tile_log + 2
    if tile_log == 4:
        for k in (0, 1, tile_log, tile_log + 1, 2 * tile_log + 1, big):
            out.add((big, k))
    return sorted(out)
