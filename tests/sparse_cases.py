"""Big-integer models and case generators for the tests of csrc/sparse.hpp (resident sparse matrices over Fr, y = M z, and Groth16's
witness map built on them), next to the helpers of ntt_cases.py.  Nothing here comes from the code under test and nothing needs a GPU
to import: y = M z is a double loop over Python integers, and the witness map is judged by an identity at a random point tau that shares
nothing with the transforms -- with L_i the Lagrange basis of the domain,

    (sum_i L_i(tau) a_i) (sum_i L_i(tau) b_i) - sum_i L_i(tau) a_i b_i == h(tau) (tau^size - 1).

The shapes are placed by the two constants of the kernels, E entries per lane and L lanes per block, which the tests read from the
library: a lane boundary lies at every multiple of E, a block boundary at every multiple of E L, and with tiles of 16 the prefix sum
over the lanes reaches its second and third level at 16 E and 256 E entries."""
import random

import ntt_cases as nc


def specials(field):
    r = nc.modulus(field)
    return [0, 1, r - 1, r, 2 * r, (1 << 256) - 1]


def raw_values(field, n, rng, only=None):
    """n raw 256-bit patterns: `only` everywhere, or a third from 0, 1, r - 1, r, 2r, 2^256 - 1 and the rest random bytes"""
    if only is not None:
        return [only] * n
    sp = specials(field)
    return [sp[rng.randrange(len(sp))] if rng.randrange(3) == 0 else rng.getrandbits(256) for _ in range(n)]


def raw_bytes(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


class Case:
    """one matrix and one vector as raw 256-bit patterns; what they stand for depends on the form they are read in"""

    def __init__(self, name, field, lengths, cols, rng, tile4=False, col_of=None, only=None):
        self.name, self.field, self.tile4 = name, field, tile4
        self.rows, self.cols = len(lengths), cols
        self.row_ptr = [0]
        for n in lengths:
            self.row_ptr.append(self.row_ptr[-1] + n)
        self.nnz = self.row_ptr[-1]
        self.col_idx = [col_of(k) if col_of else rng.randrange(cols) for k in range(self.nnz)]
        self.values = raw_values(field, self.nnz, rng, only)
        self.z = raw_values(field, cols, rng, only)

    def values_raw(self):
        return raw_bytes(self.values)

    def z_raw(self):
        return raw_bytes(self.z)

    def expected(self, create_normal, normal):
        """the bytes of y = M z with the values read in the form given at create and z read, y written, in the form of the call"""
        r = nc.modulus(self.field)
        vals = nc.decode(self.field, self.values_raw(), create_normal)
        z = nc.decode(self.field, self.z_raw(), normal)
        return nc.encode(self.field, ref_apply(r, self.row_ptr, self.col_idx, vals, z), normal)


def ref_apply(r, row_ptr, col_idx, vals, z):
    return [sum(vals[k] * z[col_idx[k]] for k in range(row_ptr[i], row_ptr[i + 1])) % r for i in range(len(row_ptr) - 1)]


def lengths_with_ends(targets, total, rng):
    """row lengths (0 .. 4 entries, about one empty row in eight) summing to `total`, with a row ending exactly at every target"""
    out, at = [], 0
    for stop in sorted(set(targets)) + [total]:
        while at < stop:
            n = min(stop - at, rng.choice((1, 1, 2, 2, 3, 3, 4, 0)))
            out.append(n)
            at += n
    return out


def power_law_lengths(rows, rng, longest):
    """most rows hold 1 - 3 entries, a few hold hundreds (a Pareto tail cut at `longest`)"""
    return [min(longest, int(rng.paretovariate(1.1))) if rng.randrange(20) else 0 for _ in range(rows)]


def cases(field, E, L, seed=0x5BA25E):
    """every shape the kernels can go wrong on, as small as it can still go wrong; tile4: the case runs with poly_tile_log = 4"""
    rng = random.Random(seed ^ nc.FIELD_IDS[field])
    r = nc.modulus(field)
    B = E * L
    out = [
        Case("nnz 0, rows 5", field, [0] * 5, 3, rng),
        Case("rows 0", field, [], 4, rng),
        Case("1 x 1", field, [1], 1, rng),
        Case("empty rows at the start, the end and three in the middle", field, [0, 0, 3, 1, 0, 0, 0, 2, E + 2, 0], 7, rng),
    ]
    for n, tile4 in ((E - 1, False), (E, False), (E + 1, False), (B - 1, False), (B, False), (B + 1, False), (16 * E + 1, True), (256 * E + 3, True)):
        out.append(Case("one row of %d" % n, field, [n], 37, rng, tile4=tile4))
    out += [
        # ends at E (exactly at a lane boundary), 2E - 1 (one entry before), 3E + 1 (one after), between rows of any length
        Case("rows that end at, before and after a lane boundary", field, [E, E - 1, E + 2, 5], 11, rng),
        Case("short rows that end at, before and after a lane boundary", field, lengths_with_ends([E, 2 * E - 1, 3 * E + 1, 5 * E], 6 * E + 5, rng), 11, rng),
        Case("rows that end at, before and after a block boundary", field, [B, B - 1, B + 2, 5], 29, rng),
        Case("short rows that end at, before and after a block boundary", field, lengths_with_ends([B, 2 * B - 1, 3 * B + 1], 3 * B + 9, rng), 29, rng, tile4=True),
        Case("a row from a lane's first entry to another lane's last", field, [E, 3 * E, 2], 5, rng),
        Case("a row from a block's first entry to another block's last", field, [B, 2 * B, 1], 5, rng),
        Case("nnz no multiple of E", field, lengths_with_ends([], 5 * E + 7, rng), 13, rng),
        Case("one column", field, lengths_with_ends([], 3 * E + 1, rng), 1, rng, col_of=lambda k: 0),
        Case("duplicate columns in a row", field, [6, E + 3, 2], 4, rng, col_of=lambda k: (k // 3) % 4),
        Case("power-law row lengths, 3000 rows", field, power_law_lengths(3000, rng, 40 * E), 2000, rng),
        Case("4E entries of 2^256 - 1 in one row", field, [2, 4 * E, 1], 3, rng, only=(1 << 256) - 1),
        Case("4E entries of r - 1 in one row", field, [2, 4 * E, 1], 3, rng, only=r - 1),
    ]
    return out


# ---- the witness map ------------------------------------------------------------------------------------------------------------------

def lagrange_at(field, k, tau):
    """L_i(tau) for the domain of 2^k points, tau outside it: (tau^n - 1) / n * omega^i / (tau - omega^i)"""
    r = nc.modulus(field)
    n = 1 << k
    om = nc.root_of_unity(field, k)
    c = (pow(tau, n, r) - 1) * pow(n, -1, r) % r
    out, w = [], 1
    for _ in range(n):
        out.append(c * w % r * pow((tau - w) % r, -1, r) % r)
        w = w * om % r
    return out


def horner(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


def witness_identity(field, k, a, b, h, tau):
    """(left side, right side) of the identity above for the padded vectors a and b and the coefficients h, all integers"""
    r = nc.modulus(field)
    lag = lagrange_at(field, k, tau)
    at = sum(l * x for l, x in zip(lag, a)) % r
    bt = sum(l * x for l, x in zip(lag, b)) % r
    ct = sum(l * x * y for l, x, y in zip(lag, a, b)) % r
    return (at * bt - ct) % r, horner(h, tau, r) * (pow(tau, 1 << k, r) - 1) % r


class R1cs:
    """a random instance of n constraints over `nvars` variables, z[0] = 1: A and B as arkworks' Matrix<F> (lists of rows of
    (coefficient, column)), and a C of one entry a row that makes it satisfied -- or, with satisfied=False, misses it in one row"""

    def __init__(self, field, n, nvars, num_inputs, rng, satisfied=True):
        r = nc.modulus(field)
        self.field, self.n, self.nvars, self.num_inputs = field, n, nvars, num_inputs
        self.z = [1] + [rng.randrange(1, r) for _ in range(nvars - 1)]
        row = lambda: [(rng.randrange(r), rng.randrange(nvars)) for _ in range(rng.choice((1, 1, 2, 3, 3, 7)))]
        self.A = [row() for _ in range(n)]
        self.B = [row() for _ in range(n)]
        self.a = [sum(c * self.z[j] for c, j in rw) % r for rw in self.A]
        self.b = [sum(c * self.z[j] for c, j in rw) % r for rw in self.B]
        self.C = []
        for i in range(n):
            j = rng.randrange(nvars)
            self.C.append([(self.a[i] * self.b[i] * pow(self.z[j], -1, r) % r, j)])
        if not satisfied:
            c, j = self.C[n // 2][0]
            self.C[n // 2] = [((c + 1) % r, j)]

    def padded(self, size):
        """(a, b) as the witness map pads them: z[0 .. num_inputs) appended to a at rows n .., zeros to `size`"""
        a = self.a + self.z[:self.num_inputs]
        return a + [0] * (size - len(a)), self.b + [0] * (size - self.n)
