#!/usr/bin/env python3
"""Time the Poseidon calls (mi355_msm_poseidon_hash, _merkle with device pointers) per scalar field and rate; writes
profiles/poseidon.txt -- every line of that file comes from this script.

  python tools/poseidon_bench.py [--fields a,b] [--rates 2,4,8] [--log-n 20] [--out profiles/poseidon.txt]

Per field and rate, with snarkVM's round numbers (alpha 17, 8 + 31 rounds), on device-resident random rows with a preallocated output,
median of five after one warm-up, host clock around a call that ends synchronised / events on the stream (the domain's
"last_device_us"):
  hash       2^log_n sponges of `rate` inputs and one output, no header: two permutations each
  dense      the same with the option "sparse" = 0: the A/B of the sparse partial rounds
  product    (dense - sparse) time over (dense - sparse) products: the marginal time of one Fr product per lane in this kernel.  The
             library has no launchable product-only kernel (the ISA yardstick moves 108 bytes per product and is bound by memory), so
             the fraction of a product-bound kernel is reported against this figure and not against an independent yardstick
  merkle     a tree of 2^log_n leaves of one element against the flat batches of the same hashes (2^log_n leaf hashes of two
             elements, 2^log_n - 1 node hashes of three): the difference is the latency tail of the top levels, one launch per level
  clock_rate, power_draw   torch.cuda.clock_rate (MHz) and torch.cuda.power_draw (as reported) sampled right after each timed loop"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import entries_amd as ea  # noqa: E402

CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
PAR = dict(alpha=17, full_rounds=8, partial_rounds=31)


def sample():
    """what torch reports right after a loop: the clock in MHz and the power sensor's reading as it comes (documented as milliwatts;
    the ROCm build returns watts)"""
    out = []
    for name, fn in (("clock_rate", getattr(torch.cuda, "clock_rate", None)), ("power_draw", getattr(torch.cuda, "power_draw", None))):
        try:
            out.append("%s %d" % (name, fn()))
        except Exception:
            out.append("%s n/a" % name)
    return ", ".join(out)


def timed(fn, dom, reps=5):
    dev, host = [], []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it:
            host.append((t1 - t0) * 1e3)
            dev.append(dom.query("last_device_us") / 1e3)
    return statistics.median(dev), statistics.median(host), sample()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="bls12_377,bls12_381")
    ap.add_argument("--rates", default="2,4,8")
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon.txt"))
    a = ap.parse_args()
    n = 1 << a.log_n
    lines = ["# tools/poseidon_bench.py on %s; 2^%d sponges, device-resident data, median of 5 after a warm-up; ms device (events) / ms host clock"
             % (torch.cuda.get_device_name(0), a.log_n)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    g = torch.Generator(device="cuda")
    g.manual_seed(a.log_n)
    for field in a.fields.split(","):
        dom = ea.Radix2EvaluationDomain(16, CURVE_OF[field])
        for rate in [int(s) for s in a.rates.split(",")]:
            with ea.Poseidon(dom, rate, parameters=PAR, domain="bench") as h:
                x = torch.randint(0, 256, (n, rate, 32), dtype=torch.uint8, device="cuda", generator=g)
                y = torch.empty((n, 1, 32), dtype=torch.uint8, device="cuda")
                res = {}
                for name, sparse in (("hash", 1), ("dense", 0)):
                    h.set_option("sparse", sparse)
                    products = h.query("products_per_permutation")
                    d, ho, smp = timed(lambda: h.sponge(x, 1, out=y), dom)
                    res[name] = (d, products)
                    say("%s rate %d %-6s %9.3f / %9.3f ms   %5d products per permutation, 2 permutations: %.3f ns per sponge, %.2f ps per product and lane; %s"
                        % (field, rate, name, d, ho, products, d * 1e6 / n, d * 1e9 / n / (2 * products), smp))
                h.set_option("sparse", 1)
                (ds, ps), (dd, pd) = res["hash"], res["dense"]
                marginal = (dd - ds) * 1e9 / n / (2 * (pd - ps))
                say("%s rate %d product marginal %.2f ps per product and lane (dense - sparse); sparse / dense time %.3f against products %.3f; the sparse form runs at %.2f of that product rate"
                    % (field, rate, marginal, ds / dd, ps / pd, marginal * 2 * ps * n / (ds * 1e9)))
                say("%s rate %d lds_bytes %d work_bytes %d" % (field, rate, h.query("lds_bytes"), h.query("work_bytes")))
                del x, y
                if rate >= 2:
                    leaves = torch.randint(0, 256, (n, 1, 32), dtype=torch.uint8, device="cuda", generator=g)
                    nodes = torch.empty((2 * n - 1, 32), dtype=torch.uint8, device="cuda")
                    dm, hm, smp = timed(lambda: h.merkle_tree(leaves, out=nodes), dom)
                    pairs = torch.randint(0, 256, (n, 3, 32), dtype=torch.uint8, device="cuda", generator=g)
                    two = pairs[:, :2].contiguous()
                    o1 = torch.empty((n, 1, 32), dtype=torch.uint8, device="cuda")
                    dl, _, _ = timed(lambda: h.hash_many(two, 1, out=o1), dom)
                    dn, _, _ = timed(lambda: h.hash_many(pairs, 1, out=o1), dom)
                    flat = dl + dn * (n - 1) / n
                    say("%s rate %d merkle 2^%d leaves %9.3f / %9.3f ms; the flat batches of the same hashes %.3f ms (leaves %.3f, nodes %.3f): the tail of the top levels %.3f ms, %.1f %%; %s"
                        % (field, rate, a.log_n, dm, hm, flat, dl, dn * (n - 1) / n, dm - flat, 100 * (dm - flat) / dm, smp))
                    del leaves, nodes, pairs, two, o1
                torch.cuda.empty_cache()
        dom.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
