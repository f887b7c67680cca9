#!/usr/bin/env python3
"""Time the segmented MSM (mi355_msm_segments) beside what a user does without it; writes profiles/segments.txt -- every line of that
file comes from this script.

  python tools/segments_bench.py [--curves a:20,b:18] [--lengths 16,64,256,1024,4096] [--windows] [--out profiles/segments.txt]

Per curve, 2^size device-resident subgroup points (generate_points), scalars uniform below r, a preallocated device output, median of
three after one warm-up, host clock (time.perf_counter) around calls that end synchronised.  For every segment length L, S = 2^size / L:
  general   msm_segments over S segments of L pairs
  shared    msm_segments(shared=True): S segments over the first L points
  (a)       multi_scalar_mult with batches over the same L bases, timed on min(S, 256) batches, stated per segment and for S segments
  (b)       mul_points on the same S * L pairs (it never sums)
With --windows, the general form also at every forced window size 4..9 (the measurement behind the table of sm_window_for).
The `guard ratio` line is what tests/test_gpu_segments.py takes its speed bound from."""
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


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def timed(call, reps=3):
    ts = []
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if it:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def uniform_below_r(curve, n, seed):
    w = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    w[:, 3] %= np.uint64(curve.r >> 192)
    return w.view(np.uint8).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bls12_381_g1:20,bls12_377_g2:18")
    ap.add_argument("--lengths", default="16,64,256,1024,4096")
    ap.add_argument("--windows", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments.txt"))
    a = ap.parse_args()
    lengths = [int(x) for x in a.lengths.split(",") if x]
    tel = bench.Telemetry(0)
    lines = ["# tools/segments_bench.py on %s: S sums of L pairs, S * L = 2^size device-resident pairs, Affine output, host clock, median of 3 after 1 warm-up"
             % torch.cuda.get_device_name(0),
             "# clock / power: %s" % tel.describe(),
             "# curve L S what: ms for the S segments (us per segment) | clock, power"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for spec in a.curves.split(","):
        name, size = spec.split(":")
        curve = pm.CURVES[name]
        n = 1 << int(size)
        d_pts = torch.from_numpy(ea.generate_points(n, seed=21, curve=name)).cuda()
        d_s = torch.from_numpy(uniform_below_r(curve, n, 21)).cuda()
        ctx = ea.MultiScalarMultContext(name)
        big = ea.MultiScalarMultContext(name)
        tel.start()
        t_mul = timed(lambda: ctx.mul_points(d_pts, d_s))
        t = tel.stop()
        emit("%s (b) mul_points on 2^%s pairs: %.3f ms | %s, %s (%d samples)" % (name, size, t_mul, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"),
                                                                                t["samples"]))
        for L in lengths:
            S = n // L
            offsets = np.arange(S + 1, dtype=np.uint64) * L
            out = torch.zeros((S, curve.affine_stride), dtype=torch.uint8, device="cuda")
            tel.start()
            t_gen = timed(lambda: ctx.msm_segments(d_pts, d_s, offsets, out=out))
            t_sh = timed(lambda: ctx.msm_segments(d_pts[:L], d_s, shared=True, out=out))
            t = tel.stop()
            tele = "%s, %s (%d samples)" % (fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"), t["samples"])
            nb = min(S, 256)
            big.set_bases(d_pts[:L])
            d_batch = d_s[:32 * L * nb]
            t_a = timed(lambda: ea.multi_scalar_mult(big, None, d_batch)) / nb
            emit("%s L=%d S=%d general: %.3f ms (%.2f us/segment) | %s" % (name, L, S, t_gen, 1e3 * t_gen / S, tele))
            emit("%s L=%d S=%d shared: %.3f ms (%.2f us/segment)" % (name, L, S, t_sh, 1e3 * t_sh / S))
            emit("%s L=%d S=%d (a) multi_scalar_mult, %d batches timed: %.2f us/segment, %.3f ms for S" % (name, L, S, nb, 1e3 * t_a, t_a * S))
            emit("%s L=%d S=%d ratios: general / (a) %.4f, general / (b) %.3f, shared / (b) %.3f" % (name, L, S, t_gen / (t_a * S), t_gen / t_mul, t_sh / t_mul))
            if a.windows:
                per = {}
                for c in range(4, 10):
                    ctx.set_option("seg_window", c)
                    per[c] = timed(lambda: ctx.msm_segments(d_pts, d_s, offsets, out=out))
                ctx.set_option("seg_window", 0)
                emit("%s L=%d S=%d by window: %s; fastest c=%d" % (name, L, S, ", ".join("c=%d %.3f ms" % kv for kv in per.items()), min(per, key=per.get)))
        if name == "bls12_381_g1":
            # the shape of the speed guard: S = 256, L = 1024, against mul_points on the same pairs
            S, L = 256, 1024
            m = S * L
            offsets = np.arange(S + 1, dtype=np.uint64) * L
            p, s = d_pts[:m], d_s[:32 * m]
            t_seg = timed(lambda: ctx.msm_segments(p, s, offsets), reps=5)
            t_m = timed(lambda: ctx.mul_points(p, s), reps=5)
            emit("%s guard S=256 L=1024: msm_segments %.3f ms, mul_points %.3f ms" % (name, t_seg, t_m))
            emit("%s guard ratio msm_segments S=256 L=1024 / mul_points: %.3f" % (name, t_seg / t_m))
        ctx.close()
        big.close()
        del d_pts, d_s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
