"""A big-integer evaluator of expression DAGs (the nodes of mi355_msm_expr_create) and the case builders of tests/test_expr_host.py and
tests/test_gpu_expr.py.  The evaluator shares nothing with the compiler of csrc/expr.hpp: it walks the nodes in the order given, with
Python integers modulo r, a whole column of rows per node.  Rows that read the same element of every column (periodic columns) are
evaluated once and the result is copied, which changes no value."""
import random
import zlib
from math import gcd

import ntt_cases as nc

COL, CONST, CHAL, ADD, SUB, MUL, NEG, SQR = range(8)
MAX_SLOTS = 32            # csrc/expr.hpp EXPR_MAX_SLOTS (the host library reports it: ht_expr_max_slots)
LENS = (1, 63, 64, 65, 1000, 4096)


def u32(rot):
    return rot & 0xFFFFFFFF


def evaluate(field, nodes, consts, chals, cols, length, rot_step=1):
    """cols: lists of integers (already decoded), len(cols[j]) divides length -> the `length` values of the last node"""
    r = nc.modulus(field)
    refs = {}
    for op, a, b in nodes:
        if op == COL and (a, b) not in refs:
            rot = b - (1 << 32) if b >> 31 else b
            refs[(a, b)] = [((i + rot * rot_step) % length) % len(cols[a]) for i in range(length)]
    keys = list(zip(*refs.values())) if refs else [()] * length
    first, row_of = {}, []
    for k in keys:
        row_of.append(first.setdefault(k, len(first)))
    rows = sorted(first.values())
    pick = {ref: [None] * len(rows) for ref in refs}
    for i in reversed(range(length)):
        for ref, idx in refs.items():
            pick[ref][row_of[i]] = idx[i]
    vals = []
    for op, a, b in nodes:
        if op == COL:
            v = [cols[a][j] % r for j in pick[(a, b)]]
        elif op == CONST:
            v = [consts[a] % r] * len(rows)
        elif op == CHAL:
            v = [chals[a] % r] * len(rows)
        elif op == ADD:
            v = [(x + y) % r for x, y in zip(vals[a], vals[b])]
        elif op == SUB:
            v = [(x - y) % r for x, y in zip(vals[a], vals[b])]
        elif op == MUL:
            v = [x * y % r for x, y in zip(vals[a], vals[b])]
        elif op == NEG:
            v = [-x % r for x in vals[a]]
        elif op == SQR:
            v = [x * x % r for x in vals[a]]
        else:
            raise ValueError(op)
        vals.append(v)
    return [vals[-1][row_of[i]] for i in range(length)]


class Case:
    """nodes, the constants, the number of challenges and columns; lens(length) -> the column lengths; edge: raw edge patterns as inputs"""

    def __init__(self, name, nodes, consts=(), n_chal=0, n_cols=1, rot_step=1, lens=None, edge=False):
        self.name, self.nodes, self.consts, self.n_chal, self.n_cols = name, list(nodes), list(consts), n_chal, n_cols
        self.rot_step, self.lens, self.edge = rot_step, lens or (lambda length: [length] * n_cols), edge

    def flat(self):
        return [w for node in self.nodes for w in node]


def edge_patterns(field):
    r = nc.modulus(field)
    return [(1 << 256) - 1, r, r - 1, 2 * r, 0, 1, r + 1, 2 * r - 1, (1 << 255) + 12345, (1 << 256) - r]


def inputs(case, field, length, normal, seed=0):
    """(cols_raw: one bytes object per column, chals: integers, expected: the canonical bytes of the form)"""
    rng = random.Random((zlib.crc32(case.name.encode()) & 0xFFFF) * 7919 + length * 31 + seed)
    r = nc.modulus(field)
    raws = []
    for j, ln in enumerate(case.lens(length)):
        if case.edge:
            pats = edge_patterns(field)
            vals = [pats[(i + 3 * j) % len(pats)] if (i + j) % 3 else rng.getrandbits(256) for i in range(ln)]
            raws.append(b"".join(v.to_bytes(32, "little") for v in vals))
        else:
            raws.append(nc.encode(field, [rng.randrange(r) for _ in range(ln)], normal))
    chals = [rng.randrange(r) for _ in range(case.n_chal)]
    cols = [nc.decode(field, raw, normal) for raw in raws]
    want = evaluate(field, case.nodes, case.consts, chals, cols, length, case.rot_step)
    return raws, chals, nc.encode(field, want, normal)


# ---- builders -------------------------------------------------------------------------------------------------------------------------------

def random_dag(seed, n_nodes, n_cols=3, n_consts=2, n_chal=2, rots=(0, 0, 1, -1), field_consts=None):
    """n_nodes nodes; operands are drawn from all earlier nodes, so sub-expressions are shared and some nodes are dead"""
    rng = random.Random(seed)
    nodes = []
    for i in range(n_nodes):
        leaf = i == 0 or rng.random() < 0.3
        if leaf:
            kind = rng.choice([COL, COL, COL, CONST, CHAL])
            if kind == COL:
                nodes.append((COL, rng.randrange(n_cols), u32(rng.choice(rots))))
            elif kind == CONST:
                nodes.append((CONST, rng.randrange(n_consts), 0))
            else:
                nodes.append((CHAL, rng.randrange(n_chal), 0))
        else:
            op = rng.choice([ADD, ADD, SUB, SUB, MUL, MUL, MUL, NEG, SQR])
            near = rng.random() < 0.6
            a = rng.randrange(max(0, i - 4), i) if near else rng.randrange(i)
            b = rng.randrange(i)
            nodes.append((op, a, b if op in (ADD, SUB, MUL) else 0))
    crng = random.Random(seed + 1)
    consts = [crng.getrandbits(250) for _ in range(n_consts)]
    return Case("dag%d_%d" % (seed, n_nodes), nodes, consts, n_chal, n_cols)


def add_chain(steps=200):
    nodes = [(COL, 0, 0)]
    for k in range(steps):
        nodes.append((COL, 1 + k % 2, 0))
        nodes.append((ADD, len(nodes) - 2 if k else 0, len(nodes) - 1))
    return Case("add_chain%d" % steps, nodes, n_cols=3)


def doubling_chain(steps=64):
    nodes = [(COL, 0, 0)]
    for _ in range(steps):
        nodes.append((ADD, len(nodes) - 1, len(nodes) - 1))
    return Case("doubling%d" % steps, nodes, n_cols=1)


def sub_chain(steps=64):
    """a = col1 - a, then a = a - col0, alternating: the running value is minuend and subtrahend in turn"""
    nodes = [(COL, 0, 0), (COL, 1, 0), (SUB, 0, 1)]
    for k in range(steps - 1):
        acc = len(nodes) - 1
        nodes.append((SUB, 1, acc) if k % 2 == 0 else (SUB, acc, 0))
    return Case("sub_chain%d" % steps, nodes, n_cols=2)


def sqr_tower(height=24):
    nodes = [(COL, 0, 0), (COL, 1, 0), (ADD, 0, 1)]
    for k in range(height):
        nodes.append((SQR, len(nodes) - 1, 0))
        if k % 5 == 4:
            nodes.append((NEG, len(nodes) - 1, 0))
    return Case("sqr_tower%d" % height, nodes, n_cols=2)


def slot_program(k):
    """k products, each used by a running sum and later by a running product: all k stay live while the sum is formed"""
    nodes, prods = [], []
    for j in range(k):
        nodes.append((COL, j % 4, 0))
        nodes.append((CHAL, j % 2, 0))
        nodes.append((MUL, len(nodes) - 2, len(nodes) - 1))
        prods.append(len(nodes) - 1)
        nodes.append((ADD, prods[-1], 0))                   # (distinct products: p_j = col * chal, then + col_0)
        prods[-1] = len(nodes) - 1
    s = prods[0]
    for p in prods[1:]:
        nodes.append((ADD, s, p))
        s = len(nodes) - 1
    t = prods[0]
    for p in prods[1:]:
        nodes.append((MUL, t, p))
        t = len(nodes) - 1
    nodes.append((SUB, s, t))
    return Case("slots_k%d" % k, nodes, n_chal=2, n_cols=4)


def long_program(steps=3400, periods=(1, 2, 8)):
    """more than 10 000 instructions: a = (a * col + chal) - col', over periodic columns, so that the model stays cheap at every length"""
    def lens(length):
        out = []
        for p in periods:
            out.append(gcd(p, length) if length % p else p)
        small = [d for d in (3, 5, 7, 13) if length % d == 0]
        out.append(small[0] if small else 1)
        return out
    nodes = [(COL, 0, 0)]
    for k in range(steps):
        acc = len(nodes) - 1
        nodes.append((COL, 1 + k % 3, u32((k % 5) - 2)))
        nodes.append((MUL, acc, len(nodes) - 1))
        nodes.append((CHAL, k % 3, 0))
        nodes.append((ADD, len(nodes) - 2, len(nodes) - 1))
        nodes.append((COL, (k + 1) % 4, u32(k % 2)))
        nodes.append((SUB, len(nodes) - 2, len(nodes) - 1))
    return Case("long%d" % steps, nodes, n_chal=3, n_cols=4, lens=lens)


def wide_program(n_cols=64):
    """every one of 64 columns, some twice"""
    nodes = [(COL, 0, 0)]
    for j in range(1, n_cols):
        nodes.append((COL, j, u32(j % 3 - 1)))
        nodes.append(((ADD, MUL, SUB)[j % 3], len(nodes) - 2, len(nodes) - 1))
    nodes.append((COL, n_cols - 1, 0))
    nodes.append((MUL, len(nodes) - 2, len(nodes) - 1))
    return Case("wide%d" % n_cols, nodes, n_cols=n_cols)


def rotation_program(rot_step=8):
    """rotations +-1 and +-3 (times rot_step) of two columns: every length wraps at both ends"""
    nodes, acc = [], None
    for rot in (1, -1, 3, -3, 0):
        nodes.append((COL, 0, u32(rot)))
        nodes.append((COL, 1, u32(-rot)))
        nodes.append((MUL, len(nodes) - 2, len(nodes) - 1))
        if acc is not None:
            nodes.append((ADD, acc, len(nodes) - 1))
        acc = len(nodes) - 1
    return Case("rot_step%d" % rot_step, nodes, n_cols=2, rot_step=rot_step)


def periodic_program(periods=(1, 8)):
    """full-length columns beside a scalar (length 1) and a column of period 8 (2 and the length itself in the host tests)"""
    def lens(length):
        return [length] + [p if length % p == 0 else 1 for p in periods]
    n = 1 + len(periods)
    nodes = [(COL, 0, 0)]
    for j in range(1, n):
        nodes.append((COL, j, u32(1)))
        nodes.append((MUL, len(nodes) - 2, len(nodes) - 1))
        nodes.append((COL, j, 0))
        nodes.append((SUB, len(nodes) - 2, len(nodes) - 1))
    return Case("periodic" + "_".join(map(str, periods)), nodes, n_cols=n, lens=lens)


def edge_program():
    """edge-value inputs through every op"""
    nodes = [(COL, 0, 0), (COL, 1, 0), (ADD, 0, 1), (SUB, 0, 1), (MUL, 2, 3), (NEG, 0, 0), (SQR, 1, 0), (ADD, 5, 6), (SUB, 4, 7), (CONST, 0, 0), (MUL, 8, 9),
             (COL, 0, u32(1)), (ADD, 10, 11)]
    return Case("edge", nodes, consts=[(1 << 256) - 1], n_cols=2, edge=True)


def single_leaf():
    return Case("leaf", [(COL, 0, u32(-1))], n_cols=1)


def dags():
    return [random_dag(11, 1), random_dag(12, 2), random_dag(13, 7), random_dag(14, 50), random_dag(15, 150), random_dag(16, 400),
            random_dag(17, 400, n_cols=6, n_consts=5, n_chal=4, rots=(0, 2, -2, 5))]


def chains():
    return [add_chain(200), doubling_chain(64), sub_chain(64)]


# ---- the Jellyfish quotient row as an expression (tests/test_gpu_expr.py, tools/expr_bench.py) --------------------------------------------

def jellyfish_columns(m, selectors):
    """column numbers: wires 0 .. m-1, sigmas m .. 2m-1, z 2m, pi 2m+1, x 2m+2, 1/Z_H 2m+3, 1/(n (x - 1)) 2m+4, then the 13 selectors"""
    base = 2 * m
    return {"w": list(range(m)), "sigma": list(range(m, 2 * m)), "z": base, "pi": base + 1, "x": base + 2, "zh_inv": base + 3, "l1_den": base + 4,
            "q": list(range(base + 5, base + 18)) if selectors else [], "ncols": base + 5 + (13 if selectors else 0)}


def jellyfish_expr(ea, m, selectors, ks):
    """out = (gate + alpha (z prod (w + beta k x + gamma) - z' prod (w + beta sigma + gamma))) / Z_H + alpha^2 (z - 1) / (n (x - 1)) with the
    challenges alpha, beta, gamma = challenge 0, 1, 2; the gate is pi alone without selectors (Radix2EvaluationDomain.plonk_quotient)"""
    E = ea.Expr
    at = jellyfish_columns(m, selectors)
    w = [E.col(j) for j in at["w"]]
    sg = [E.col(j) for j in at["sigma"]]
    z, zn, pi, x = E.col(at["z"]), E.col(at["z"], 1), E.col(at["pi"]), E.col(at["x"])
    alpha, beta, gamma = E.challenge(0), E.challenge(1), E.challenge(2)
    gate = pi
    if selectors:
        q = [E.col(j) for j in at["q"]]
        q_lc, q_mul, q_hash, q_o, q_c, q_ecc = q[0:4], q[4:6], q[6:10], q[10], q[11], q[12]
        gate = q_c + pi
        for j in range(4):
            gate = gate + q_lc[j] * w[j]
        gate = gate + q_mul[0] * (w[0] * w[1]) + q_mul[1] * (w[2] * w[3])
        gate = gate + q_ecc * (w[0] * w[1] * w[2] * w[3] * w[4])
        for j in range(4):
            gate = gate + q_hash[j] * w[j] ** 5
        gate = gate - q_o * w[4]
    bx = beta * x
    p1, p2 = z, zn
    for j in range(m):
        p1 = p1 * (w[j] + bx * E.const(ks[j]) + gamma)
        p2 = p2 * (w[j] + beta * sg[j] + gamma)
    return (gate + alpha * (p1 - p2)) * E.col(at["zh_inv"]) + alpha * alpha * (z - 1) * E.col(at["l1_den"])
