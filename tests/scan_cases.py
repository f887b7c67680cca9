"""Big-integer models and input builders for the tests of csrc/scan.hpp (prefix product, prefix sum, the Plonk permutation product),
next to the helpers of ntt_cases.py and poly_cases.py.  Nothing here comes from the code under test: the models are a running product,
a running sum and the grand-product formula with pow(x, -1, r)."""
import random

import ntt_cases as nc
import poly_cases as pc

PRODUCT, SUM = 0, 1
FLAG_NORMAL, FLAG_INCLUSIVE = 1, 2
RUN = pc.RUN


def vector(field, n, tile_log, seed, zeros=True):
    """n raw 256-bit patterns: random ones (two in three above r), r - 1 and 2^256 - 1 and, with zeros=True, every multiple of r
    planted at the first and last position of a lane run and of a tile (poly_cases.vector).  Without zeros the same spots hold r - 1
    and 2^256 - 1 in turn, so a running product stays away from zero over the whole vector."""
    raw = pc.vector(field, n, tile_log, seed, zeros=zeros)
    if not zeros:
        r = nc.modulus(field)
        T = 1 << tile_log
        for j, pos in enumerate([0, RUN - 1, RUN, 2 * RUN - 1, T - 1, T, 2 * T - 1, n - 1, n - RUN, n - T]):
            if 0 <= pos < n:
                raw[pos] = (r - 1, (1 << 256) - 1)[j & 1]
    return raw


def single_zero(field, n, tile_log, seed, which=0):
    """a vector without zeros but for one multiple of r in the middle of the second tile; returns (raw, position or None)"""
    raw = vector(field, n, tile_log, seed, zeros=False)
    T = 1 << tile_log
    pos = T + T // 2
    if pos >= n:
        return raw, None
    mult = pc.multiples_of_r(field)
    raw[pos] = mult[which % len(mult)]
    return raw, pos


def ref_scan(vals, op, inclusive, r):
    """(the scan of vals, the combination of all of them)"""
    acc = 1 if op == PRODUCT else 0
    out = []
    for v in vals:
        if not inclusive:
            out.append(acc)
        acc = acc * v % r if op == PRODUCT else (acc + v) % r
        if inclusive:
            out.append(acc)
    return out, acc


def coset_representatives(field, m):
    """k_i = g^i: 1 and powers of the multiplicative generator, which lie in distinct cosets of every radix-2 domain"""
    r, g = nc.modulus(field), nc.generator(field)
    return [pow(g, i, r) for i in range(m)]


def domain_elements(field, k):
    r, w = nc.modulus(field), nc.root_of_unity(field, k)
    out = [1] * (1 << k)
    for j in range(1, 1 << k):
        out[j] = out[j - 1] * w % r
    return out


class Permutation:
    """wires[i][j], sigmas[i][j] (integers), ks, beta, gamma of a domain of 2^k rows and m columns"""

    def __init__(self, field, k, m, wires, sigmas, ks, beta, gamma):
        self.field, self.k, self.m, self.n = field, k, m, 1 << k
        self.wires, self.sigmas, self.ks, self.beta, self.gamma = wires, sigmas, ks, beta, gamma

    def factors(self, rows=None):
        """(num[j], den[j]) of the formula, for all rows or the given ones"""
        r = nc.modulus(self.field)
        if rows is None:
            om = domain_elements(self.field, self.k)
            rows = range(self.n)
            ids = lambda j: om[j]
        else:
            w = nc.root_of_unity(self.field, self.k)
            ids = lambda j: pow(w, j, r)
        out = []
        for j in rows:
            num = den = 1
            idj = ids(j)
            for i in range(self.m):
                num = num * (self.wires[i][j] + self.beta * self.ks[i] * idj + self.gamma) % r
                den = den * (self.wires[i][j] + self.beta * self.sigmas[i][j] + self.gamma) % r
            out.append((num, den))
        return out

    def model(self):
        """(z: n values, total); a zero denominator gives the factor 0, as a batch inversion that leaves zeros alone does"""
        r = nc.modulus(self.field)
        z, acc = [], 1
        for num, den in self.factors():
            z.append(acc)
            acc = acc * num * (pow(den, -1, r) if den else 0) % r
        return z, acc

    def columns(self, which, normal, stride, lift=True):
        """the m columns as one byte string, `stride` elements apart (the gaps hold 0xEE bytes); with lift, every third element that
        allows it has r added to its pattern, which leaves its residue alone"""
        r = nc.modulus(self.field)
        cols = []
        for i, col in enumerate(which):
            raw = bytearray(nc.encode(self.field, col, normal))
            if lift:
                for j in range(i % 3, self.n, 3):
                    v = int.from_bytes(raw[32 * j:32 * j + 32], "little") + r
                    if v < 1 << 256:
                        raw[32 * j:32 * j + 32] = v.to_bytes(32, "little")
            if i + 1 < self.m:
                raw += b"\xee" * (32 * (stride - self.n))
            cols.append(bytes(raw))
        return b"".join(cols)


def permutation(field, k, m, seed):
    """a valid instance: sigma is a permutation of the m n values ks[i] omega^j made of random cycles (lengths 1 .. 6), and the wire
    values are constant on every cycle"""
    rng = random.Random(seed)
    r = nc.modulus(field)
    n = 1 << k
    ks = coset_representatives(field, m)
    om = domain_elements(field, k)
    cells = [(i, j) for i in range(m) for j in range(n)]
    rng.shuffle(cells)
    wires = [[0] * n for _ in range(m)]
    sigmas = [[0] * n for _ in range(m)]
    at = 0
    while at < len(cells):
        cyc = cells[at:at + rng.randint(1, 6)]
        at += len(cyc)
        v = rng.randrange(r)
        for t, (i, j) in enumerate(cyc):
            ni, nj = cyc[(t + 1) % len(cyc)]
            wires[i][j] = v
            sigmas[i][j] = ks[ni] * om[nj] % r
    return Permutation(field, k, m, wires, sigmas, ks, rng.randrange(1, r), rng.randrange(1, r))


def broken(p, seed):
    """p with one wire value changed, in a cell that sigma does not map to itself: the copy constraints no longer hold"""
    rng = random.Random(seed)
    r = nc.modulus(p.field)
    om = domain_elements(p.field, p.k)
    wires = [list(c) for c in p.wires]
    while True:
        i, j = rng.randrange(p.m), rng.randrange(p.n)
        if p.sigmas[i][j] != p.ks[i] * om[j] % r:
            break
    wires[i][j] = (wires[i][j] + 1 + rng.randrange(1 << 64)) % nc.modulus(p.field)
    return Permutation(p.field, p.k, p.m, wires, p.sigmas, p.ks, p.beta, p.gamma)


def zero_denominator(p):
    """p with gamma = -(w + beta sigma) at one cell: that row's denominator is zero.  The same gamma zeroes the numerator of the cell
    sigma points to (the same wire value, that id), so the cell is the first one from the middle row on whose sigma points to a
    later row: every row before it keeps non-zero factors.  Returns (the instance, the row)."""
    r = nc.modulus(p.field)
    om = domain_elements(p.field, p.k)
    row_of = {p.ks[i] * om[j] % r: j for i in range(p.m) for j in range(p.n)}
    row, col = next((j, i) for j in range(p.n // 2, p.n) for i in range(p.m) if row_of[p.sigmas[i][j]] > j)
    gamma = -(p.wires[col][row] + p.beta * p.sigmas[col][row]) % r
    return Permutation(p.field, p.k, p.m, p.wires, p.sigmas, p.ks, p.beta, gamma), row
