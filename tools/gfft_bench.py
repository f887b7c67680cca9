#!/usr/bin/env python3
"""Time the transforms over curve points (mi355_msm_fft_points_device) per curve and size beside pairwise mul_points on the same n
points; writes profiles/gfft.txt -- every line of that file comes from this script.

  python tools/gfft_bench.py [--curves a,b] [--sizes 12,16,20] [--g2-sizes 12,16] [--out profiles/gfft.txt]

Per curve and size, 2^size device-resident points h_j * G with random h_j (made by the fixed-base entry, so all distinct and in the
subgroup), a preallocated device output, median of three after one warm-up, on two clocks:
  device ms   query "last_fft_points_device_us" / "last_mul_device_us": between events on the stream the call ran on
  host ms     time.perf_counter around the call, which ends synchronised
for the forward, the inverse and the coset inverse transform and for mul_points with random scalars below r.  The `ratio` lines
(host clock) are what tests/test_gpu_gfft.py takes its speed bounds from; `model` is the count of multiplications per point against
mul_points' one: (k - 1) / 2 forward, one more for the inverse kinds."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the clock / power sampler)
import entries_amd as ea  # noqa: E402
import pymodel as pm  # noqa: E402

CURVES = ("bls12_377_g1", "bls12_381_g1", "bls12_377_g2", "bls12_381_g2")
KINDS = (("forward", 0), ("inverse", 1), ("coset inverse", 3))


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def timed(call, query, reps=3):
    dev, host = [], []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if it:
            dev.append(query() / 1000.0)
            host.append((t1 - t0) * 1000.0)
    return statistics.median(dev), statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default=",".join(CURVES))
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--g2-sizes", default="12,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gfft.txt"))
    a = ap.parse_args()
    tel = bench.Telemetry(0)
    lines = ["# tools/gfft_bench.py on %s: transforms of 2^k device-resident subgroup points, Affine output, median of 3 after 1 warm-up" % (
                 torch.cuda.get_device_name(0)),
             "# clock / power: %s" % tel.describe(),
             "# curve n what: device ms (events), host ms (the whole call), ns per point | clock, power"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for name in a.curves.split(","):
        curve = pm.CURVES[name]
        stride = curve.affine_stride
        sizes = [int(s) for s in (a.g2_sizes if curve.ext == 2 else a.sizes).split(",") if s]
        ctx = ea.MultiScalarMultContext(name)
        for k in sizes:
            n = 1 << k
            rng = np.random.default_rng(k)
            scal = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
            scal[:, 31] &= 0x0F                        # below r for both fields
            d_s = torch.from_numpy(scal.reshape(-1)).cuda()
            with ea.FixedBase.get_window_table(curve.encode_affine(curve.generator()), curve=name, expected_scalars=n) as table:
                d_pts = table.msm(d_s)
            out = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
            with ea.Radix2EvaluationDomain(n, curve=name) as dom:
                tel.start()
                dev_m, host_m = timed(lambda: ctx.mul_points(d_pts, d_s), lambda: ctx.query("last_mul_device_us"))
                t = tel.stop()
                emit("%s n=2^%d mul_points w=%d: device %.3f ms, host %.3f ms, %.2f ns/point | %s, %s (%d samples)" % (
                    name, k, ctx.query("mul_window"), dev_m, host_m, host_m * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"),
                    t["samples"]))
                for label, kind in KINDS:
                    tel.start()
                    dev, host = timed(lambda: ctx.fft_points(dom, d_pts, kind=kind, out=out), lambda: ctx.query("last_fft_points_device_us"))
                    t = tel.stop()
                    emit("%s n=2^%d %s (chunk 2^%d): device %.3f ms, host %.3f ms, %.2f ns/point | %s, %s (%d samples)" % (
                        name, k, label, ctx.query("fft_points_chunk").bit_length() - 1, dev, host, host * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"),
                        fmt(t["power_W_mean"], "W"), t["samples"]))
                    model = (k - 1) / 2 + (1 if kind & 1 else 0)
                    emit("%s n=2^%d ratio %s / mul_points: %.3f (model %.1f)" % (name, k, label, host / host_m, model))
                emit("%s n=2^%d work memory: %.1f MiB" % (name, k, ctx.query("fft_points_work_bytes") / 2.0 ** 20))
            del d_pts, d_s, out
            torch.cuda.empty_cache()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
