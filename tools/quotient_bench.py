#!/usr/bin/env python3
"""Time the rows of the Plonk quotient and the linear combination (mi355_msm_domain_plonk_quotient_device, _linear_combination_device)
per scalar field beside a forward NN transform and a device-to-device copy of the same length; writes profiles/quotient.txt -- every
line of that file comes from this script.

  python tools/quotient_bench.py [--fields a,b] [--sizes 20,23,25] [--out profiles/quotient.txt]

Device-resident data, preallocated outputs, median of five after one warm-up, on two clocks:
  device ms   query "last_device_us": between events on the stream the call ran on
  host ms     time.perf_counter around the call, which ends synchronised
M = 2^size is the quotient domain, n = M / 8 the constraint domain: 5 wires, 5 sigmas, 13 selectors, z and pi of random elements (the
arithmetic does not depend on the constraints holding).  The `ratio plonk_quotient` line of BLS12-381 at 2^20 is what
tests/test_gpu_quotient.py takes its speed bound from (host clock); the linear combination of 15 vectors, beside the 15 scale and 14
add calls it replaces, is recorded and not guarded."""
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
WIRES, SELECTORS, COMBINED = 5, 13, 15


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
    ap.add_argument("--sizes", default="20,23,25")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quotient.txt"))
    a = ap.parse_args()
    lines = ["# tools/quotient_bench.py on %s; device-resident data, median of 5 after a warm-up; ms device (events) / ms host clock" % torch.cuda.get_device_name(0)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    alpha, beta, gamma = 0x1F2E3D4C5B6A79880123456789ABCDEF, 0x123456789ABCDEF0123456789ABCDEF, 0xFEDCBA9876543210FEDCBA987654321
    ks = [1, 7, 49, 343, 2401]
    coeffs = [pow(0x9E3779B97F4A7C15F39CC0605CEDC835, j + 1, 1 << 250) for j in range(COMBINED)]
    for field in a.fields.split(","):
        for k in [int(s) for s in a.sizes.split(",")]:
            M = 1 << k
            dom = ea.Radix2EvaluationDomain(M, CURVE_OF[field])
            x = random_elements((M,), k)
            out = torch.empty_like(x)
            _, h_copy = timed(lambda: out.copy_(x))
            d_ntt, h_ntt = timed(lambda: dom.fft(x, out=out), dom)
            say("%s 2^%d forward NN                 %8.3f / %8.3f ms" % (field, k, d_ntt, h_ntt))
            say("%s 2^%d device-to-device copy      %8s / %8.3f ms (%.0f GB/s read + written)" % (field, k, "", h_copy, 64.0 * M / (h_copy * 1e-3) / 1e9))
            wires, sigmas = random_elements((WIRES, M), k + 200), random_elements((WIRES, M), k + 300)
            selectors, pi = random_elements((SELECTORS, M), k + 400), random_elements((M,), k + 500)
            nbytes = 32 * (2 * WIRES + SELECTORS + 2 + 1 + 1) + 32 + 6 * 32          # the inputs (z twice), the output, x - 1 written and read by the inversion
            d, h = timed(lambda: dom.plonk_quotient(wires, sigmas, x, alpha, beta, gamma, ks, M // 8, selectors=selectors, pi=pi, out=out), dom)
            say("%s 2^%d %-26s %8.3f / %8.3f ms   %.2f x forward NN, %.2f x copy, %.0f GB/s, %.2f ns per row"
                % (field, k, "plonk_quotient", d, h, h / h_ntt, h / h_copy, nbytes * M / (d * 1e-3) / 1e9, h * 1e6 / M))
            say("%s ratio plonk_quotient 2^%d / forward NN 2^%d: %.4f" % (field, k, k, h / h_ntt))
            say("%s 2^%d quotient_work_bytes %d, scan_work_bytes %d, poly_work_bytes %d, poly_tile_log %d"
                % (field, k, dom.query("quotient_work_bytes"), dom.query("scan_work_bytes"), dom.query("poly_work_bytes"), dom.query("poly_tile_log")))
            del selectors, sigmas, pi
            torch.cuda.empty_cache()
            cols = [wires[j] for j in range(WIRES)] + [random_elements((M,), k + 600 + j) for j in range(COMBINED - WIRES)]
            d, h = timed(lambda: dom.linear_combination(cols, coeffs, out=out), dom)
            say("%s 2^%d %-26s %8.3f / %8.3f ms   %.2f x forward NN, %.2f x copy, %.0f GB/s, %.2f ns per element"
                % (field, k, "linear_combination m=15", d, h, h / h_ntt, h / h_copy, 32 * (COMBINED + 1) * M / (d * 1e-3) / 1e9, h * 1e6 / M))
            tmp = torch.empty_like(x)

            def by_hand():
                dom.scale(cols[0], coeffs[0], out=out)
                for j in range(1, COMBINED):
                    dom.scale(cols[j], coeffs[j], out=tmp)
                    dom.add(out, tmp, out=out)

            _, h_hand = timed(by_hand)
            say("%s 2^%d %-26s %8s / %8.3f ms   %.2f x linear_combination" % (field, k, "15 scale + 14 add", "", h_hand, h_hand / h))
            dom.close()
            del x, out, tmp, wires, cols
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
