"""Big-integer models and input builders for the tests of csrc/quotient.hpp (the rows of the TurboPlonk quotient, the linear
combination), next to the helpers of ntt_cases.py, poly_cases.py and scan_cases.py.  Nothing here comes from the code under test: the
rows follow the formulas of the reference prover (Jellyfish, plonk/src/proof_system/prover.rs:368-395, 414-447, 457-500) with
pow(x, -1, r), the combination is a sum."""
import random

import ntt_cases as nc
import poly_cases as pc
import scan_cases as sc

GATE_WIRES, SELECTORS = 5, 13
Q_LC, Q_MUL, Q_HASH, Q_O, Q_C, Q_ECC = 0, 4, 6, 10, 11, 12      # the reference's order: q_lc[0..3], q_mul[0..1], q_hash[0..3], q_o, q_c, q_ecc


def gate(w, q, pi, r):
    """compute_quotient_circuit_contribution for one row: w the 5 wire values, q the 13 selector values"""
    t = q[Q_C] + pi
    for j in range(4):
        t += q[Q_LC + j] * w[j] + q[Q_HASH + j] * pow(w[j], 5, r)
    t += q[Q_MUL] * w[0] * w[1] + q[Q_MUL + 1] * w[2] * w[3] + q[Q_ECC] * w[0] * w[1] * w[2] * w[3] * w[4] - q[Q_O] * w[4]
    return t % r


def ref_quotient_rows(field, K, n, wires, sigmas, selectors, z, pi, ks, alpha, beta, gamma, g=None):
    """out[i] for all M = 2^K rows; every vector is a list of M integers, wires / sigmas / selectors lists of columns; selectors None:
    the gate is pi alone; pi None: 0; g None: the field's generator"""
    r = nc.modulus(field)
    M = 1 << K
    ratio = M // n
    g = nc.generator(field) if g is None else g % r
    om = nc.root_of_unity(field, K)
    zh_inv = [pow((pow(g * pow(om, i, r), n, r) - 1) % r, -1, r) for i in range(ratio)]
    n_inv = pow(n, -1, r)
    out = []
    x = g
    for i in range(M):
        w = [col[i] for col in wires]
        p = pi[i] if pi is not None else 0
        t_circ = gate(w, [col[i] for col in selectors], p, r) if selectors is not None else p
        a, b = z[i], z[(i + ratio) % M]
        for j, wj in enumerate(w):
            a = a * (wj + beta * ks[j] * x + gamma) % r
            b = b * (wj + beta * sigmas[j][i] + gamma) % r
        t_perm1 = alpha * (a - b) % r
        t_perm2 = alpha * alpha * (z[i] - 1) * n_inv * pow((x - 1) % r, -1, r) % r
        out.append(((t_circ + t_perm1) * zh_inv[i % ratio] + t_perm2) % r)
        x = x * om % r
    return out


def ref_lincomb(cols, coeffs, r):
    n = max((len(c) for c in cols), default=0)
    return [sum(c * col[i] for c, col in zip(coeffs, cols) if i < len(col)) % r for i in range(n)]


# ---- rows: raw 256-bit patterns in every vector ---------------------------------------------------------------------------------

def planted(field, M, rng):
    """M raw 256-bit patterns: random ones (two in three above r is possible), and r, 2r, 2^256 - 1 and 0 planted -- the byte
    patterns of poly_cases -- at the two ends, at random rows and, so that they meet in one row across the vectors, at row M // 2"""
    r = nc.modulus(field)
    raw = [rng.getrandbits(256) if i % 3 else rng.randrange(r) for i in range(M)]
    special = [r, 2 * r, (1 << 256) - 1, 0]
    spots = [0, M - 1, M // 2, rng.randrange(M), rng.randrange(M), 1, M - 2, rng.randrange(M)]
    for t, pos in enumerate(spots):
        raw[pos % M] = special[t if t < 4 else rng.randrange(4)]
    return raw


class Rows:
    """one call of plonk_quotient: raw patterns of every vector and the scalars as integers"""

    def __init__(self, field, K, n, m, seed, selectors=True, pi=True, offset=None, z_one=False):
        rng = random.Random(seed)
        self.field, self.K, self.n, self.m, self.M = field, K, n, m, 1 << K
        r = nc.modulus(field)
        self.wires = [planted(field, self.M, rng) for _ in range(m)]
        self.sigmas = [planted(field, self.M, rng) for _ in range(m)]
        self.selectors = [planted(field, self.M, rng) for _ in range(SELECTORS)] if selectors else None
        self.z = None if z_one else planted(field, self.M, rng)      # None: identically 1, encoded in the form of the call
        self.pi = planted(field, self.M, rng) if pi else None
        self.ks = sc.coset_representatives(field, m)
        self.alpha, self.beta, self.gamma = rng.randrange(1, r), rng.randrange(1, r), rng.randrange(1, r)
        self.offset = offset

    def raw_z(self, normal):
        return self.z if self.z is not None else [int.from_bytes(nc.encode(self.field, [1], normal), "little")] * self.M

    def model(self, normal):
        v = lambda raw: pc.values(self.field, raw, normal)
        cols = lambda c: None if c is None else [v(x) for x in c]
        return ref_quotient_rows(self.field, self.K, self.n, cols(self.wires), cols(self.sigmas), cols(self.selectors), v(self.raw_z(normal)),
                                 None if self.pi is None else v(self.pi), self.ks, self.alpha, self.beta, self.gamma, self.offset)

    def columns(self, which, stride):
        """the columns as one byte string, `stride` elements apart (the gaps hold 0xEE bytes)"""
        out = []
        for i, col in enumerate(which):
            raw = pc.to_raw(col)
            if i + 1 < len(which):
                raw += b"\xee" * (32 * (stride - self.M))
            out.append(raw)
        return b"".join(out)


def row_cases(field):
    """(name, Rows, the tile logs worth running): the sizes at which the rows take another path -- ratio 2 with the wrap of z over the
    last two rows, ratio 8 with two inversion tiles at tile 16, two default tiles, the pi-only gate at ratio 16 with 1, 3 and 8 columns,
    z identically 1, no pi, an offset of the caller's"""
    f = {"bls12_377": 0x377000, "bls12_381": 0x381000}[field]
    return [
        ("K3_n4", Rows(field, 3, 4, 5, f + 1), (4, 10)),
        ("K5_n4", Rows(field, 5, 4, 5, f + 2), (4, 10)),
        ("K11_n256", Rows(field, 11, 256, 5, f + 3), (4, 10)),
        ("nosel_m1", Rows(field, 6, 4, 1, f + 4, selectors=False), (4, 10)),
        ("nosel_m3", Rows(field, 6, 4, 3, f + 5, selectors=False), (4,)),
        ("nosel_m8", Rows(field, 6, 4, 8, f + 6, selectors=False), (4,)),
        ("z_one", Rows(field, 5, 4, 5, f + 7, z_one=True), (4, 10)),
        ("no_pi_offset", Rows(field, 5, 8, 5, f + 8, pi=False, offset=pow(nc.generator(field), 5, nc.modulus(field))), (4,)),
        ("nosel_no_pi", Rows(field, 4, 4, 2, f + 9, selectors=False, pi=False), (4,)),
    ]


LINCOMB_LENGTHS = (0, 1, 255, 256, 257, 1025)


def lincomb_cases(field):
    """(raw columns, coefficients): m in 1, 2, 15, 32 with the lengths mixed within one call, and the all-empty call"""
    rng = random.Random({"bls12_377": 0x377AAA, "bls12_381": 0x381AAA}[field])
    r = nc.modulus(field)
    out = []
    for m in (1, 2, 15, 32):
        for rot in (0, 3):
            lens = [LINCOMB_LENGTHS[(j + rot + (m == 1) * 5) % len(LINCOMB_LENGTHS)] for j in range(m)]
            cols = [planted(field, ln, rng) if ln > 8 else [rng.getrandbits(256) for _ in range(ln)] for ln in lens]
            coeffs = [rng.randrange(r) for _ in range(m)]
            coeffs[rng.randrange(m)] = (0, 1, r - 1)[rng.randrange(3)]
            out.append((cols, coeffs))
    out.append(([[], []], [3, 4]))
    return out


# ---- a small satisfying circuit ---------------------------------------------------------------------------------------------------

class Circuit:
    """n = 2^k rows of a TurboPlonk circuit whose gate and copy constraints hold: values on H_n as integers"""

    def __init__(self, field, k, seed):
        rng = random.Random(seed)
        r = nc.modulus(field)
        self.field, self.k, self.n = field, k, 1 << k
        # a random permutation of the 5n cells made of cycles, wire values constant on its cycles, sigmas as ks[i'] omega^j'
        self.perm = sc.permutation(field, k, GATE_WIRES, seed)
        self.wires, self.sigmas, self.ks = self.perm.wires, self.perm.sigmas, self.perm.ks
        self.pi = [rng.randrange(r) for _ in range(self.n)]
        self.selectors = [[rng.randrange(r) for _ in range(self.n)] for _ in range(SELECTORS)]
        for i in range(self.n):               # q_c solved per row so that the gate holds
            q = [col[i] for col in self.selectors]
            q[Q_C] = 0
            self.selectors[Q_C][i] = -gate([col[i] for col in self.wires], q, self.pi[i], r) % r
        for i in range(self.n):
            assert gate([col[i] for col in self.wires], [col[i] for col in self.selectors], self.pi[i], r) == 0

    def broken(self):
        """one wire value changed: the gate of that row (and the copy constraint of that cell) no longer holds"""
        other = Circuit.__new__(Circuit)
        other.__dict__.update(self.__dict__)
        other.wires = [list(c) for c in self.wires]
        other.wires[2][self.n // 3] = (other.wires[2][self.n // 3] + 1) % nc.modulus(self.field)
        return other


def poly_eval(coeffs, x, r):
    return pc.ref_evaluate(coeffs, x, r)


def blind(coeffs, n, blinders, r):
    """coeffs + (b0 + b1 X + ..) Z_H(X) for Z_H = X^n - 1"""
    out = list(coeffs) + [0] * (n + len(blinders) - len(coeffs))
    for t, b in enumerate(blinders):
        out[t] = (out[t] - b) % r
        out[n + t] = (out[n + t] + b) % r
    return out
