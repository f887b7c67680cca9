#!/usr/bin/env python3
"""Time compiled expressions (ea.Expr, dom.compile_expression, GateProgram.run) per scalar field; writes profiles/expr.txt -- every line
of that file comes from this script.

  python tools/expr_bench.py [--fields bls12_377,bls12_381] [--log 22] [--ratio 8] [--chain-log 22] [--out profiles/expr.txt]

(a) the Jellyfish gate and permutation terms of dom.plonk_quotient (5 wires, 13 selectors) written as an Expr (tests/expr_cases.py) and run
    at M = 2^log, ratio 8, against plonk_quotient itself on the same inputs; the outputs must be byte-equal.  The x column comes from
    coset_fft of the polynomial X, 1 / (n (x - 1)) from the batch inversion, the `ratio` values 1 / Z_H from Python integers.
(b) the same expression evaluated node by node with dom.mul / add / sub / scale on GPU tensors, one launch and one pass over HBM per
    node: what a caller has to do today.  Rotated and periodic leaves and the constant vectors are prepared OUTSIDE the timed window
    (generous to the baseline); nothing else about it is tuned.  Its output must be byte-equal too.
(c) products per second of a synthetic product chain over S live values, S = 4, 16 and the limit: the cost of occupancy.

Device-resident inputs, median of five synchronised calls after two warm-ups, on two clocks: query "last_device_us" (between events on
the stream of the call) and time.perf_counter around the call, which ends synchronised; the GPU's shader clock and socket power are
sampled while the calls run (bench.py's Telemetry)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import bench  # noqa: E402  (the clock / power sampler)
import entries_amd as ea  # noqa: E402
import expr_cases as xc  # noqa: E402
import ntt_cases as nc  # noqa: E402

CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
REPS, WARM = 5, 2


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def timed(call, device_us):
    dev, host = [], []
    for it in range(REPS + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= WARM:
            dev.append(device_us() / 1e3 if device_us else float("nan"))
            host.append((t1 - t0) * 1e3)
    return statistics.median(dev), statistics.median(host)


def random_elements(shape, seed):
    """canonical for both fields: below 2^252"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 256, shape + (32,), dtype=torch.uint8, device="cuda", generator=g)
    t[..., 31] &= 0x0F
    return t


def elements(field, values):
    return torch.frombuffer(bytearray(nc.encode(field, values, False)), dtype=torch.uint8).cuda().reshape(-1, 32)


def const_vector(leaves, v):
    t = leaves.get(("const", v))
    if t is None:
        raise KeyError("the vector of the scalar %d was not prepared" % v)
    return t


def node_by_node(dom, nodes, consts, chals, leaves, M):
    """the DAG with one library call per interior node; leaves: {(col, rot): tensor of M elements}, constants as integers"""
    r = dom.modulus
    val = [None] * len(nodes)
    for i, (op, a, b) in enumerate(nodes):
        if op == xc.COL:
            val[i] = leaves[(a, b)]
        elif op == xc.CONST:
            val[i] = consts[a]
        elif op == xc.CHAL:
            val[i] = chals[a]
        else:
            x, y = val[a], (val[b] if op in (xc.ADD, xc.SUB, xc.MUL) else None)
            if isinstance(x, int) and (y is None or isinstance(y, int)):         # scalars among themselves: host arithmetic
                val[i] = {xc.NEG: -x, xc.SQR: x * x, xc.MUL: x * (y or 0), xc.ADD: x + (y or 0), xc.SUB: x - (y or 0)}[op] % r
            elif op == xc.NEG:
                val[i] = dom.scale(x, r - 1)
            elif op == xc.SQR:
                val[i] = dom.mul(x, x)
            elif op == xc.MUL:
                if isinstance(x, int) or isinstance(y, int):
                    s, v = (x, y) if isinstance(x, int) else (y, x)
                    val[i] = dom.scale(v, s)
                else:
                    val[i] = dom.mul(x, y)
            else:
                x = const_vector(leaves, x) if isinstance(x, int) else x
                y = const_vector(leaves, y) if isinstance(y, int) else y
                val[i] = dom.add(x, y) if op == xc.ADD else dom.sub(x, y)
    return val[-1]


def chain_program(dom, live, products):
    """`live` running values t_j = col0 * challenge_j + col1, then rounds of t_j = t_j * t_(j+1) until `products` products; their sum"""
    E = ea.Expr
    t = [E.col(0) * E.challenge(j % 4) + E.col(1, j) for j in range(live)]
    done = 0
    while done < products:
        for j in range(live):
            t[j] = t[j] * t[(j + 1) % live]
            done += 1
    s = t[0]
    for v in t[1:]:
        s = s + v
    return dom.compile_expression(s, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="bls12_377,bls12_381")
    ap.add_argument("--log", type=int, default=22)
    ap.add_argument("--ratio", type=int, default=8)
    ap.add_argument("--chain-log", type=int, default=22)
    ap.add_argument("--chain-products", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expr.txt"))
    a = ap.parse_args()
    tel = bench.Telemetry(0)
    lines = ["# tools/expr_bench.py on %s; device-resident inputs, median of %d after %d warm-ups; ms device (events) / ms host clock"
             % (torch.cuda.get_device_name(0), REPS, WARM), "# clock / power: %s" % tel.describe()]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(label, call, device_us, extra=""):
        tel.start()
        d, h = timed(call, device_us)
        t = tel.stop()
        say("%-64s %9.3f / %9.3f ms%s | %s, %s (%d samples)" % (label, d, h, extra, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"), t["samples"]))
        return h

    for field in a.fields.split(","):
        K, ratio = a.log, a.ratio
        M, n, r = 1 << K, (1 << K) // ratio, nc.modulus(field)
        dom = ea.Radix2EvaluationDomain(M, CURVE_OF[field])
        m, ks = 5, [1, 7, 13, 17, 23]
        alpha, beta, gamma = 0x123456789ABCDEF0123456789ABCDEF, 0xFEDCBA9876543210FEDCBA987654321, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F
        wires, sigmas, sel = [random_elements((M,), 10 + j) for j in range(m)], [random_elements((M,), 20 + j) for j in range(m)], [random_elements((M,), 30 + j) for j in range(13)]
        z, pi = random_elements((M,), 50), random_elements((M,), 51)
        # x = g omega^i: the evaluations of the polynomial X on the coset; 1 / (n (x - 1)); the `ratio` values of 1 / Z_H
        poly_x = torch.zeros((M, 32), dtype=torch.uint8, device="cuda")
        poly_x[1] = elements(field, [1])[0]
        xs = dom.coset_fft(poly_x)
        ones = elements(field, [1]).repeat(M, 1)
        l1_den = dom.batch_inversion_and_mul(dom.sub(xs, ones), pow(n, -1, r))
        g, om = nc.generator(field), nc.root_of_unity(field, K)
        zh_inv = elements(field, [pow((pow(g * pow(om, i, r), n, r) - 1) % r, -1, r) for i in range(ratio)])
        del poly_x
        at = xc.jellyfish_columns(m, True)
        cols = wires + sigmas + [z, pi, xs, zh_inv, l1_den] + sel
        expr = xc.jellyfish_expr(ea, m, True, ks)
        out_q, out_e = torch.empty((M, 32), dtype=torch.uint8, device="cuda"), torch.empty((M, 32), dtype=torch.uint8, device="cuda")
        # (a)
        h_q = run("%s (a) plonk_quotient M = 2^%d ratio %d" % (field, K, ratio),
                  lambda: dom.plonk_quotient(wires, sigmas, z, alpha, beta, gamma, ks, n, selectors=sel, pi=pi, out=out_q), lambda: dom.query("last_device_us"))
        with dom.compile_expression(expr, at["ncols"]) as prog:
            info = {k: prog.query(k) for k in ("nodes", "instructions", "slots", "products", "reduces", "lds_bytes")}
            h_e = run("%s (a) the same rows as an expression" % field, lambda: prog.run(cols, challenges=(alpha, beta, gamma), rot_step=ratio, out=out_e),
                      lambda: prog.query("last_device_us"))
            say("%s (a) program: %s" % (field, info))
            assert torch.equal(out_q, out_e), "the expression and plonk_quotient disagree"
            say("%s (a) outputs byte-equal; expression / plonk_quotient = %.2f; %.2f G products/s" % (field, h_e / h_q, M * info["products"] / h_e / 1e6))
        # (b)
        nodes, consts, n_chal, _ = expr.nodes(r)
        leaves = {}
        for op, c, rot in nodes:
            if op == xc.COL and (c, rot) not in leaves:
                col = cols[c]
                if col.shape[0] != M:
                    col = col.repeat(M // col.shape[0], 1)
                sh = (rot - (1 << 32) if rot >> 31 else rot) * ratio
                leaves[(c, rot)] = torch.roll(col, -sh, 0).contiguous() if sh else col
        for v in list(consts) + [alpha, beta, gamma]:             # what an ADD or a SUB of a constant or a challenge needs: its vector
            leaves[("const", v)] = elements(field, [v]).repeat(M, 1)
        interior = sum(1 for op, _, _ in nodes if op > xc.CHAL)
        res = [None]

        def by_node():
            res[0] = node_by_node(dom, nodes, consts, [alpha, beta, gamma], leaves, M)

        h_n = run("%s (b) node by node: %d library calls" % (field, interior), by_node, None)
        assert torch.equal(res[0], out_q), "node by node and plonk_quotient disagree"
        say("%s (b) outputs byte-equal; node by node / expression = %.2f; node by node / plonk_quotient = %.2f" % (field, h_n / h_e, h_n / h_q))
        del res, leaves, wires, sigmas, sel, cols, xs, ones, l1_den, out_q, out_e, z, pi
        torch.cuda.empty_cache()
        dom.close()
        # (c)
        L = 1 << a.chain_log
        dom = ea.Radix2EvaluationDomain(1 << 4, CURVE_OF[field])
        c0, c1 = random_elements((L,), 70), random_elements((L,), 71)
        out = torch.empty((L, 32), dtype=torch.uint8, device="cuda")
        limit = xc.MAX_SLOTS
        for want in (4, 16, limit):
            prog = None
            for live in range(want + 1, 1, -1):
                try:
                    p = chain_program(dom, live, a.chain_products)
                except ea.MsmError:
                    continue
                if p.query("slots") <= want:
                    prog = p
                    break
                p.close()
            S, products = prog.query("slots"), prog.query("products")
            h = run("%s (c) product chain S = %d (%d live values), %d products per row, 2^%d rows" % (field, S, live, products, a.chain_log),
                    lambda: prog.run([c0, c1], challenges=(3, 5, 7, 11)[:prog.n_chal], out=out), lambda: prog.query("last_device_us"),
                    "  LDS %d KiB per block" % (prog.query("lds_bytes") >> 10))
            say("%s (c) S = %d: %.2f G products/s (host clock)" % (field, S, L * products / h / 1e6))
            prog.close()
        dom.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
