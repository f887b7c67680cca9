#!/usr/bin/env python3
"""Time the lookup-table calls (ea.LookupTable: create, multiplicities with the index, sorted) and the logUp running sum
(dom.logup_sum) per scalar field, beside dom.prefix_sum and dom.permutation_product of the same length in the same session; writes
profiles/lookup.txt -- every line of that file comes from this script.

  python tools/lookup_bench.py [--fields bls12_381] [--table-sizes 16,20,24] [--value-sizes 20,24] [--table-log 20] [--logup-log 20]
                               [--out profiles/lookup.txt]

Device-resident inputs, median of three synchronised calls after one warm-up, on two clocks:
  device ms   query "last_device_us": between events on the stream the call ran on (create, count, logup_sum; sorted reports the whole
              call, whose host look at the missing count lies between its two halves)
  host ms     time.perf_counter around the call, which ends synchronised
with the GPU's shader clock and socket power sampled while the calls ran (bench.py's Telemetry).  The four distributions of the values:
uniform over the table; all on one entry; half on one entry (a padded column) and half uniform; uniform with 1 % of the values outside
the table.  `sorted` refuses the last one by contract and is timed on the other three."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (the clock / power sampler)
import entries_amd as ea  # noqa: E402

CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def timed(call, dom, reps=3):
    dev, host = [], []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it:
            dev.append(dom.query("last_device_us") / 1e3)
            host.append((t1 - t0) * 1e3)
    return statistics.median(dev), statistics.median(host)


def random_elements(shape, seed):
    """canonical for both fields: below 2^252"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 256, shape + (32,), dtype=torch.uint8, device="cuda", generator=g)
    t[..., 31] &= 0x0F
    return t


def values_of(table, n_f, kind, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n_t = table.shape[0]
    idx = torch.randint(0, n_t, (n_f,), device="cuda", generator=g)
    if kind == "one entry":
        idx[:] = n_t // 3
    elif kind == "half padding":
        idx[torch.rand(n_f, device="cuda", generator=g) < 0.5] = n_t // 3
    v = table[idx]
    if kind == "1 % missing":
        gone = torch.rand(n_f, device="cuda", generator=g) < 0.01
        v[gone] = random_elements((int(gone.sum()),), seed + 1)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="bls12_381")
    ap.add_argument("--table-sizes", default="16,20,24")
    ap.add_argument("--value-sizes", default="20,24")
    ap.add_argument("--table-log", type=int, default=20)
    ap.add_argument("--logup-log", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup.txt"))
    a = ap.parse_args()
    tel = bench.Telemetry(0)
    lines = ["# tools/lookup_bench.py on %s; device-resident inputs, median of 3 after a warm-up; ms device (events) / ms host clock" % torch.cuda.get_device_name(0),
             "# clock / power: %s" % tel.describe()]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(label, call, dom, n, extra=""):
        tel.start()
        d, h = timed(call, dom)
        t = tel.stop()
        say("%-58s %8.3f / %8.3f ms  %6.2f ns per element%s | %s, %s (%d samples)" % (label, d, h, h * 1e6 / n, extra, fmt(t["clock_MHz_mean"], "MHz"),
                                                                                fmt(t["power_W_mean"], "W"), t["samples"]))
        return h

    for field in a.fields.split(","):
        dom = ea.Radix2EvaluationDomain(1 << a.logup_log, CURVE_OF[field])
        for k in [int(s) for s in a.table_sizes.split(",")]:
            table = random_elements((1 << k,), k)
            made = []

            def create():
                for lt in made:
                    lt.close()
                made[:] = [ea.LookupTable(dom, table)]

            run("%s create n_t = 2^%d" % (field, k), create, dom, 1 << k)
            lt = made[0]
            say("%s create n_t = 2^%d: slots 2^%d, distinct %d, max_probe %d, table_bytes %d" % (field, k, lt.query("slots").bit_length() - 1, lt.query("distinct"),
                                                                                             lt.query("max_probe"), lt.query("table_bytes")))
            lt.close()
            del table
            torch.cuda.empty_cache()
        table = random_elements((1 << a.table_log,), 77)
        with ea.LookupTable(dom, table) as lt:
            for k in [int(s) for s in a.value_sizes.split(",")]:
                n_f = 1 << k
                uniform = {}
                for kind in ("uniform", "one entry", "half padding", "1 % missing"):
                    v = values_of(table, n_f, kind, k)
                    h = run("%s count + index n_t = 2^%d n_f = 2^%d %s" % (field, a.table_log, k, kind), lambda: lt.multiplicities(v, index=True), dom, n_f)
                    uniform.setdefault("count", h)
                    say("%s ratio count %s / uniform at 2^%d: %.3f" % (field, kind, k, h / uniform["count"]))
                    if kind != "1 % missing":
                        out = torch.empty((lt.n + n_f, 32), dtype=torch.uint8, device="cuda")
                        h = run("%s sorted n_t = 2^%d n_f = 2^%d %s" % (field, a.table_log, k, kind), lambda: lt.sorted(v, out=out), dom, n_f)
                        uniform.setdefault("sorted", h)
                        say("%s ratio sorted %s / uniform at 2^%d: %.3f" % (field, kind, k, h / uniform["sorted"]))
                        del out
                    del v
                    torch.cuda.empty_cache()
            say("%s n_t = 2^%d lookup_work_bytes %d" % (field, a.table_log, lt.query("lookup_work_bytes")))
        # the logUp sum beside the cheapest Fr-vector pass and the permutation product of the same length and columns
        n = 1 << a.logup_log
        t = table[:n] if table.shape[0] >= n else random_elements((n,), 5)
        x, out = random_elements((n,), 6), torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        h_sum = run("%s prefix_sum n = 2^%d" % (field, a.logup_log), lambda: dom.prefix_sum(x, out=out), dom, n)
        beta, gamma = 0x123456789ABCDEF0123456789ABCDEF, 0xFEDCBA9876543210FEDCBA987654321
        for m in (1, 4):
            cols = torch.stack([values_of(t, n, "half padding", 100 + c) for c in range(m)])
            with ea.LookupTable(dom, t) as lt:
                mult = lt.multiplicities(cols.reshape(-1, 32))[0]
            sig = random_elements((m, n), 9)
            h_perm = run("%s permutation_product n = 2^%d m = %d" % (field, a.logup_log, m), lambda: dom.permutation_product(cols, sig, beta, gamma, [7 ** i for i in range(m)], out=out),
                         dom, n)
            for helpers in (False, True):
                res = []
                h = run("%s logup_sum n = 2^%d m = %d helpers %s" % (field, a.logup_log, m, "on" if helpers else "off"),
                        lambda: res.append(dom.logup_sum(t, mult, cols, beta, helpers=helpers, out=out)[1]), dom, n)
                assert res[-1] == 0, "the bench's own inputs satisfy the multiset relation"
                say("%s ratio logup_sum m = %d helpers %s: %.3f x permutation_product, %.2f x prefix_sum" % (field, m, "on" if helpers else "off", h / h_perm,
                                                                                                         h / h_sum))
            del cols, sig, mult
            torch.cuda.empty_cache()
        say("%s n = 2^%d logup_work_bytes %d, scan_work_bytes %d" % (field, a.logup_log, dom.query("logup_work_bytes"), dom.query("scan_work_bytes")))
        dom.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
