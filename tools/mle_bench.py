#!/usr/bin/env python3
"""Time the multilinear-extension and sumcheck calls of the domain handle (mi355_msm_domain_mle_fix, _sumcheck_round with device
pointers) per scalar field beside the forward NN transform of 2^20 elements and a device-to-device copy of the bytes each call moves;
writes profiles/mle.txt -- every line of that file comes from this script.

  python tools/mle_bench.py [--fields a,b] [--sizes 20,22,24] [--out profiles/mle.txt]

Per size nv, on device-resident random tables with preallocated outputs, median of five after one warm-up, on two clocks:
  evaluate   mle_evaluate of one table of 2^nv elements (reads it once; the later passes are 2^-10 of it)
  round      one FUSED round of Spartan's list eq (a b - c) over four tables of 2^nv elements: reads 4 * 2^nv elements, writes
             4 * 2^(nv-1), returns four evaluations
  plain      the plain round of the same list (no fold, no output vectors)
  device ms  the domain's query "last_device_us": between events on the stream the call ran on
  host ms    time.perf_counter around the call, which ends synchronised
The `ratio round nv = 22` and `ratio evaluate nv = 24` lines of BLS12-381 (host clock, over the transform of 2^20) are what
tests/test_gpu_mle.py takes its speed bounds from."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import entries_amd as ea  # noqa: E402

CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
NTT_LOG = 20


def timed(fn, dom=None, reps=5):
    dev, host = [], []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it:
            host.append((t1 - t0) * 1e3)
            if dom is not None:
                dev.append(dom.query("last_device_us") / 1e3)
    return (statistics.median(dev) if dev else None), statistics.median(host)


def copy_ms(moved):
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    _, h = timed(lambda: dst.copy_(src))
    del src, dst
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="bls12_377,bls12_381")
    ap.add_argument("--sizes", default="20,22,24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mle.txt"))
    a = ap.parse_args()
    lines = ["# tools/mle_bench.py on %s; device-resident data, median of 5 after a warm-up; ms device (events) / ms host clock" % torch.cuda.get_device_name(0)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for field in a.fields.split(","):
        dom = ea.Radix2EvaluationDomain(1 << NTT_LOG, CURVE_OF[field])
        r = dom.modulus
        rng = random.Random(NTT_LOG)
        g = torch.Generator(device="cuda")
        g.manual_seed(NTT_LOG)
        x = torch.randint(0, 256, (1 << NTT_LOG, 32), dtype=torch.uint8, device="cuda", generator=g)
        y = torch.empty_like(x)
        d_ntt, h_ntt = timed(lambda: dom.fft(x, out=y), dom)
        say("%s 2^%d forward NN                 %8.3f / %8.3f ms" % (field, NTT_LOG, d_ntt, h_ntt))
        terms = [(1, [0, 1, 2]), (r - 1, [0, 3])]
        for nv in [int(s) for s in a.sizes.split(",")]:
            n = 1 << nv
            tabs = [torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
            folded = [torch.empty((n // 2, 32), dtype=torch.uint8, device="cuda") for _ in range(4)]
            point = [rng.randrange(r) for _ in range(nv)]
            jobs = (
                # (name, bytes read + written, call)
                ("evaluate", 32 * n + 2 * 36 * (n >> 10), lambda: dom.mle_evaluate(tabs[0], point)),
                ("round", 4 * 32 * n + 4 * 32 * (n // 2), lambda: dom.sumcheck_round(tabs, terms, r_prev=point[0], out=folded)),
                ("plain", 4 * 32 * n, lambda: dom.sumcheck_round(tabs, terms)),
            )
            for which, moved, fn in jobs:
                h_copy = copy_ms(moved)
                d, h = timed(fn, dom)
                say("%s nv = %d %-9s %8.3f / %8.3f ms   %.2f x forward NN 2^%d; %d bytes read + written, a copy of them %.3f ms (%.2f x), %.0f GB/s"
                    % (field, nv, which, d, h, h / h_ntt, NTT_LOG, moved, h_copy, h / h_copy, moved / (d * 1e-3) / 1e9))
                say("%s ratio %s nv = %d / forward NN 2^%d: %.4f" % (field, which, nv, NTT_LOG, h / h_ntt))
            say("%s nv = %d mle_work_bytes %d" % (field, nv, dom.query("mle_work_bytes")))
            del tabs, folded
            torch.cuda.empty_cache()
        dom.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
