#!/usr/bin/env python3
"""Time the radix-2 transforms (mi355_msm_domain_transform_device) per scalar field beside a device-to-device copy of the same bytes and
one MSM of the same length on the family's G1 context; writes profiles/ntt.txt -- every line of that file comes from this script.

  python tools/ntt_bench.py [--fields a,b] [--sizes 16,20,22,24,26] [--pass-logs 7,8,9,10] [--out profiles/ntt.txt]

Device-resident data, a preallocated output, median of five after one warm-up, on two clocks:
  device ms   query "last_device_us": between events on the stream the call ran on
  host ms     time.perf_counter around the call, which ends synchronised
for forward NN and NR, inverse, coset forward, a batch of 16 at 2^20, forward NN at other values of pass_log, with the pass count and
the bytes per second each pass comes to (2 x 32 bytes per element per pass over the device time).  The `ratio` line is what
tests/test_gpu_ntt.py takes its speed bound from (host clock)."""
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
    ap.add_argument("--sizes", default="16,20,22,24,26")
    ap.add_argument("--pass-logs", default="7,9,10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ntt.txt"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    lines = ["# tools/ntt_bench.py on %s; device-resident data, median of 5 after a warm-up; ms device (events) / ms host clock" % torch.cuda.get_device_name(0)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for field in a.fields.split(","):
        curve = CURVE_OF[field]
        ratio_parts = {}
        for k in sizes:
            n = 1 << k
            dom = ea.Radix2EvaluationDomain(n, curve)
            x = random_elements((n,), k)
            out = torch.empty_like(x)
            passes = dom.query("passes")
            for label, fn in (("forward NN", lambda: dom.fft(x, out=out)), ("forward NR", lambda: dom.fft(x, out=out, order="NR")),
                              ("inverse", lambda: dom.ifft(x, out=out)), ("coset forward", lambda: dom.coset_fft(x, out=out))):
                d, h = timed(fn, dom)
                say("%s 2^%d %-13s %8.3f / %8.3f ms   %d passes (pass_log %d), %.0f GB/s per pass, %.2f ns per element"
                    % (field, k, label, d, h, passes, dom.query("pass_log"), passes * 64.0 * n / (d * 1e-3) / 1e9 if d else 0, h * 1e6 / n))
                if label == "forward NN":
                    ratio_parts[k] = h
            if k >= 20:
                for pl in [int(p) for p in a.pass_logs.split(",")]:
                    dom.set_option("pass_log", pl)
                    d, h = timed(lambda: dom.fft(x, out=out), dom)
                    say("%s 2^%d forward NN, pass_log %2d: %8.3f / %8.3f ms   %d passes" % (field, k, pl, d, h, dom.query("passes")))
                dom.set_option("pass_log", 0)
            _, h = timed(lambda: out.copy_(x))
            say("%s 2^%d device-to-device copy of the same bytes: %8.3f ms host (%.0f GB/s read + written)" % (field, k, h, 64.0 * n / (h * 1e-3) / 1e9))
            if k == 20:
                xb = random_elements((16, n), 99)
                ob = torch.empty_like(xb)
                d, h = timed(lambda: dom.fft(xb, out=ob), dom)
                say("%s 2^%d forward NN, batch 16: %8.3f / %8.3f ms   (%.3f ms per vector)" % (field, k, d, h, h / 16))
                del xb, ob
            if k in (22, 24, 26) or k == max(sizes):
                bases = ea.generate_points(n, distinct=1 << 15, seed=0x5EED, curve=curve)
                ctx = ea.multi_scalar_mult_init(torch.from_numpy(bases).cuda(), curve)
                del bases
                _, hm = timed(lambda: ctx.run(x), reps=3)
                ctx.close()
                say("%s 2^%d one MSM on %s, device scalars: %8.3f ms host" % (field, k, curve, hm))
                if k == 22:
                    say("%s ratio forward NN 2^22 / msm 2^22: %.4f" % (field, ratio_parts[k] / hm))
            dom.close()
            del x, out
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
