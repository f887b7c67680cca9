#!/usr/bin/env python3
"""Time the prefix scans and the permutation product (mi355_msm_domain_scan_device, _permutation_product_device) per scalar field beside
a forward NN transform and a device-to-device copy of the same length; writes profiles/scan.txt -- every line of that file comes from
this script.

  python tools/scan_bench.py [--fields a,b] [--sizes 20,22,24] [--out profiles/scan.txt]

Device-resident data, preallocated outputs, median of five after one warm-up, on two clocks:
  device ms   query "last_device_us": between events on the stream the call ran on
  host ms     time.perf_counter around the call, which ends synchronised
The `ratio prefix_product` line of BLS12-381 at 2^22 is what tests/test_gpu_scan.py takes its speed bound from (host clock); the sum
scan and the permutation product (m = 5 columns of random elements: the arithmetic does not depend on the copy constraints) are
recorded and not guarded."""
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
COLUMNS = 5


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


def random_elements(shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 256, shape + (32,), dtype=torch.uint8, device="cuda", generator=g)
    t[..., 31] &= 0x0F
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="bls12_377,bls12_381")
    ap.add_argument("--sizes", default="20,22,24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan.txt"))
    a = ap.parse_args()
    lines = ["# tools/scan_bench.py on %s; device-resident data, median of 5 after a warm-up; ms device (events) / ms host clock" % torch.cuda.get_device_name(0)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    beta, gamma, ks = 0x123456789ABCDEF0123456789ABCDEF, 0xFEDCBA9876543210FEDCBA987654321, [1, 7, 49, 343, 2401]
    for field in a.fields.split(","):
        for k in [int(s) for s in a.sizes.split(",")]:
            n = 1 << k
            dom = ea.Radix2EvaluationDomain(n, CURVE_OF[field])
            x = random_elements((n,), k)
            out = torch.empty_like(x)
            _, h_copy = timed(lambda: out.copy_(x))
            d_ntt, h_ntt = timed(lambda: dom.fft(x, out=out), dom)
            say("%s 2^%d forward NN                 %8.3f / %8.3f ms" % (field, k, d_ntt, h_ntt))
            say("%s 2^%d device-to-device copy      %8s / %8.3f ms (%.0f GB/s read + written)" % (field, k, "", h_copy, 64.0 * n / (h_copy * 1e-3) / 1e9))
            wires, sigmas = random_elements((COLUMNS, n), k + 200), random_elements((COLUMNS, n), k + 300)
            for label, fn, nbytes in (("prefix_product", lambda: dom.prefix_product(x, out=out), 96), ("prefix_sum", lambda: dom.prefix_sum(x, out=out), 96),
                                      ("permutation_product", lambda: dom.permutation_product(wires, sigmas, beta, gamma, ks, out=out), 64 * COLUMNS + 32 + 6 * 64)):
                d, h = timed(fn, dom)
                say("%s 2^%d %-26s %8.3f / %8.3f ms   %.2f x forward NN, %.2f x copy, %.0f GB/s, %.2f ns per element"
                    % (field, k, label, d, h, h / h_ntt, h / h_copy, nbytes * n / (d * 1e-3) / 1e9 if d else 0, h * 1e6 / n))
                say("%s ratio %s 2^%d / forward NN 2^%d: %.4f" % (field, label, k, k, h / h_ntt))
            say("%s 2^%d scan_work_bytes %d, poly_work_bytes %d, poly_tile_log %d"
                % (field, k, dom.query("scan_work_bytes"), dom.query("poly_work_bytes"), dom.query("poly_tile_log")))
            dom.close()
            del x, out, wires, sigmas
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
