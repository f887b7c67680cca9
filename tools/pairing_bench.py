#!/usr/bin/env python3
"""Time the pairing calls (mi355_msm_pairing_run with device pointers) for both families; writes profiles/pairing.txt -- every line of
that file comes from this script.

  python tools/pairing_bench.py [--families a,b] [--logs 10,16,20] [--out profiles/pairing.txt] [--reps 3]

Per family, on device-resident subgroup points (tools-generated, replicated) with a preallocated output, median of `reps` calls after one
warm-up, host clock around a call that ends synchronised:
  batch      n = 2^k pairings with group 1, for every k of --logs
  groth16    n = 2^18 pairs in groups of 4, the shape of a batch of Groth16 verifications
  product    one product of 2^16 pairs.  Its final exponentiation runs on ONE lane; a call of one pair with group 1 is one Miller loop and
             one final exponentiation on one lane each, so that call's time, split by the products the handle counts for the two, gives
             the single-lane final exponentiation and its share of the product call
  yardstick  the Fp products of one pairing as the handle counts them (an Fp2 product is two fused dual products, 3.04 plain Fp products
             in multiply-adds) times the marginal time of one Fp product of the family as RECORDED in profiles/r01_ubench_mul.txt (1 / 80.84 and
             1 / 80.33 Gmul/s from tools/ubench_mul.hip; that program is not run again here)
  clock_rate, power_draw   torch.cuda.clock_rate (MHz) and torch.cuda.power_draw (as reported), sampled by a thread every 20 ms DURING
             each timed loop: minimum / median / maximum"""
import argparse
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import entries_amd as ea  # noqa: E402

CURVES = {"bls12_377": ("bls12_377_g1", "bls12_377_g2"), "bls12_381": ("bls12_381_g1", "bls12_381_g2")}
# Fp products per second of the whole chip, dependent fe_mul chains: the figures RECORDED in profiles/r01_ubench_mul.txt (asm chains,
# 20000 iterations) -- tools/ubench_mul.hip is not run again here
FP_PRODUCTS_PER_S = {"bls12_377": 80.84e9, "bls12_381": 80.33e9}
MADS_PER_FP2 = 3.04                    # an Fp2 product in plain Fp products, by multiply-adds (tests/test_isa_pairing.py)


class Sampler:
    """clock and power while a loop runs"""

    def __init__(self):
        self.rows, self.stop = [], threading.Event()
        self.thread = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while not self.stop.is_set():
            row = []
            for fn in (getattr(torch.cuda, "clock_rate", None), getattr(torch.cuda, "power_draw", None)):
                try:
                    row.append(fn())
                except Exception:
                    row.append(None)
            self.rows.append(row)
            self.stop.wait(0.02)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()

    def text(self):
        out = []
        for i, name in enumerate(("clock_rate", "power_draw")):
            v = [r[i] for r in self.rows if r[i] is not None]
            out.append("%s %d / %d / %d (%d samples)" % (name, min(v), statistics.median(v), max(v), len(v)) if v else "%s n/a" % name)
        return ", ".join(out)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    with Sampler() as s:
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), s.text()


def points(curve, n):
    """n subgroup points on the device: 2^10 distinct ones, replicated"""
    base = torch.from_numpy(ea.generate_points(1 << 10, distinct=1 << 10, seed=0x50414952, curve=curve)).cuda()
    return base.repeat((n + (1 << 10) - 1) >> 10, 1)[:n].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default="bls12_377,bls12_381")
    ap.add_argument("--logs", default="10,16,20")
    ap.add_argument("--groth16-log", type=int, default=18)
    ap.add_argument("--product-log", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing.txt"))
    a = ap.parse_args()
    lines = ["# tools/pairing_bench.py on %s; device-resident points, median (min .. max) of %d calls after a warm-up, ms by the host clock around a synchronised call"
             % (torch.cuda.get_device_name(0), a.reps)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    top = max([int(k) for k in a.logs.split(",")] + [a.groth16_log, a.product_log])
    for fam in a.families.split(","):
        c1, c2 = CURVES[fam]
        with ea.Pairing(c1) as h:
            pm, pf = h.query("products_miller"), h.query("products_final_exponentiation")
            ps = 1e12 / FP_PRODUCTS_PER_S[fam]
            yard_ns = (pm + pf) / 4 * MADS_PER_FP2 * ps / 1e3
            say("%s products per pairing: Miller loop %d, final exponentiation %d Fp products (Fp2 products x 4); as %.0f plain Fp products at %.2f ps each (recorded in profiles/r01_ubench_mul.txt, not run again): %.1f ns per pairing when nothing but products ran"
                % (fam, pm, pf, (pm + pf) / 4 * MADS_PER_FP2, ps, yard_ns))
            P, Q = points(c1, 1 << top), points(c2, 1 << top)
            for k in [int(s) for s in a.logs.split(",")]:
                n = 1 << k
                out = torch.empty((n, 576), dtype=torch.uint8, device="cuda")
                med, lo, hi, smp = timed(lambda: h.pairing(P[:n], Q[:n], out=out), a.reps)
                say("%s batch   n 2^%-2d group 1      %10.3f ms (%.3f .. %.3f)  %8.1f ns per pairing, %.2f x the product yardstick; %s"
                    % (fam, k, med, lo, hi, med * 1e6 / n, med * 1e6 / n / yard_ns, smp))
                del out
            n = 1 << a.groth16_log
            out = torch.empty((n // 4, 576), dtype=torch.uint8, device="cuda")
            med, lo, hi, smp = timed(lambda: h.pairing(P[:n], Q[:n], group=4, out=out), a.reps)
            say("%s groth16 n 2^%-2d group 4      %10.3f ms (%.3f .. %.3f)  %8.1f ns per pair; %s" % (fam, a.groth16_log, med, lo, hi, med * 1e6 / n, smp))
            n = 1 << a.product_log
            out = torch.empty((1, 576), dtype=torch.uint8, device="cuda")
            med, lo, hi, smp = timed(lambda: h.pairing(P[:n], Q[:n], group=n, out=out), a.reps)
            launches = h.query("last_launches")
            one = torch.empty((1, 576), dtype=torch.uint8, device="cuda")
            m1, _, _, _ = timed(lambda: h.pairing(P[:1], Q[:1], out=one), a.reps)
            fe_ms = m1 * pf / (pm + pf)
            say("%s product n 2^%-2d group 2^%-2d   %10.3f ms (%.3f .. %.3f)  %d launches; one pair on one lane takes %.3f ms, of which the final exponentiation %.3f ms by its share of the products: %.1f %% of the product call; %s"
                % (fam, a.product_log, a.product_log, med, lo, hi, launches, m1, fe_ms, 100 * fe_ms / med, smp))
            say("%s workspace_bytes %d work_bytes %d" % (fam, h.query("workspace_bytes"), h.query("work_bytes")))
            del P, Q, out, one
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
