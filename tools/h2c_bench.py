#!/usr/bin/env python3
"""Time hash-to-curve (mi355_msm_h2c_hash and _field with device pointers) for both groups of BLS12-381; writes profiles/h2c.txt --
every line of that file comes from this script.

  python tools/h2c_bench.py [--groups g1,g2] [--logs 16,20] [--out profiles/h2c.txt] [--reps 3]

Per group, on device-resident messages of 32 bytes with a preallocated output, median of `reps` calls after one warm-up, host clock
around a call that ends synchronised:
  hash       n = 2^k messages -> n points (hash_to_curve)
  field      the same messages -> 2 n field elements (hash_to_field alone: SHA-256 and the reduction)
  yardstick  in the same run, mul_points_by with a 64-bit k on the same number of points of the same group
  count      the field products of one hash and of one yardstick multiplication, counted from the code (below), and the ratio the
             count predicts next to the measured one
  clock_rate, power_draw   torch.cuda.clock_rate (MHz) and torch.cuda.power_draw (as reported), sampled by a thread every 20 ms DURING
             each timed loop: minimum / median / maximum

The count (products of the coordinate field; a squaring counts as a product, a fused dual product as two):
  per u      the map's straight-line part 22, the exponentiation of sqrt_ratio (bits - 1 squarings and 3/4 of bits / 2 products, plus
             2 for the table: 378 + 144 over Fp, 756 + 286 over Fp2), 3 per sqrt_ratio candidate (2 / 8), 3 for the signs and the
             input, the Horner chains 3 per step (31 / 7 steps) and 8 to assemble the XYZZ point
  per hash   two u, the pair sum 14, the cofactor: G1 63 doublings of 11 and 6 additions of 14; G2 two such walks with 5 additions
             each, one more doubling, 6 additions, 4 psi of 4 and 4 negations; the output 5
  yardstick  63 doublings of 11, 21 mixed additions of 11 (a 64-bit k in non-adjacent form), the output 5"""
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

CURVES = {"g1": "bls12_381_g1", "g2": "bls12_381_g2"}
K64 = 0xd201000000010001


def counts(group):
    bits, cands, steps = (379, 2, 31) if group == "g1" else (757, 8, 7)
    per_u = 22 + (bits - 1) + (3 * (bits // 2)) // 4 + 2 + 3 * cands + 3 + 3 * steps + 8
    walk = 63 * 11
    clear = walk + 6 * 14 if group == "g1" else 2 * (walk + 5 * 14) + 11 + 6 * 14 + 4 * 4 + 4
    return 2 * per_u + 14 + clear + 5, walk + 21 * 11 + 5


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", default="g1,g2")
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h2c.txt"))
    a = ap.parse_args()
    lines = ["# tools/h2c_bench.py on %s; device-resident 32-byte messages, median (min .. max) of %d calls after a warm-up, ms by the host clock around a synchronised call"
             % (torch.cuda.get_device_name(0), a.reps)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for group in a.groups.split(","):
        curve = CURVES[group]
        per_hash, per_mul = counts(group)
        say("%s counted from the code: %d field products per hash, %d per 64-bit multiplication: ratio %.2f" % (group, per_hash, per_mul, per_hash / per_mul))
        with ea.HashToCurve(curve, dst=b"QUUX-V01-CS02-with-BLS12381-bench") as h:
            ctx = ea.MultiScalarMultContext(curve)
            try:
                for k in [int(s) for s in a.logs.split(",")]:
                    n = 1 << k
                    gen = torch.Generator(device="cuda").manual_seed(k)
                    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=gen)
                    out = torch.empty((n, ea.affine_stride(curve)), dtype=torch.uint8, device="cuda")
                    hm, lo, hi, smp = timed(lambda: h.hash(msgs, out=out), a.reps)
                    say("%s hash      n 2^%-2d  %10.3f ms (%.3f .. %.3f)  %8.1f ns per message, %d launches, %d lanes in flight; %s"
                        % (group, k, hm, lo, hi, hm * 1e6 / n, h.query("last_launches"), h.query("lanes_in_flight"), smp))
                    fld = torch.empty((2 * n, 48 * h.m), dtype=torch.uint8, device="cuda")
                    fm, lo, hi, smp = timed(lambda: h.hash_to_field(msgs, out=fld), a.reps)
                    say("%s field     n 2^%-2d  %10.3f ms (%.3f .. %.3f)  %8.1f ns per message (%.1f %% of the hash); %s" % (group, k, fm, lo, hi, fm * 1e6 / n, 100 * fm / hm, smp))
                    ym, lo, hi, smp = timed(lambda: ctx.mul_points_by(out, K64), a.reps)
                    say("%s yardstick n 2^%-2d  %10.3f ms (%.3f .. %.3f)  %8.1f ns per point: hash / yardstick %.2f measured, %.2f counted; %s"
                        % (group, k, ym, lo, hi, ym * 1e6 / n, hm / ym, per_hash / per_mul, smp))
                    del msgs, out, fld
                say("%s work_bytes %d" % (group, h.query("work_bytes")))
            finally:
                ctx.close()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
