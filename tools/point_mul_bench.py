#!/usr/bin/env python3
"""Time batch variable-base multiplication (mi355_msm_mul_points_device) per curve beside check_bases(exact=True) on the same points;
writes profiles/point_mul.txt -- every line of that file comes from this script.

  python tools/point_mul_bench.py [--curves a,b] [--windows 3,4,5] [--size 20] [--out profiles/point_mul.txt]

Per curve, 2^size device-resident subgroup points (generate_points), full 256-bit random scalars, a preallocated device output, median
of three after one warm-up, on two clocks:
  device ms   query "last_mul_device_us": between events on the stream the call ran on
  host ms     time.perf_counter around the call, which ends synchronised
for pairwise multiplication at every window size, one-scalar multiplication by r and by the cofactor, and check_bases(exact=True)
(its own device microseconds and the host clock around the call).  The `ratio` lines are what tests/test_gpu_point_mul.py takes
its speed bounds from (host clock)."""
import argparse
import ctypes
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


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def time_mul(ctx, lib, d_pts, n, stride, scalars, scalar_bytes, flags, out, reps=3):
    dev, host = [], []
    stream = torch.cuda.current_stream().cuda_stream
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        err = lib.mi355_msm_mul_points_device(ctx.context, d_pts.data_ptr(), n, stride, scalars, scalar_bytes, flags, out.data_ptr(), stride, stream)
        t1 = time.perf_counter()
        assert err.code == 0
        if it:
            dev.append(ctx.query("last_mul_device_us") / 1000.0)
            host.append((t1 - t0) * 1000.0)
    return statistics.median(dev), statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default=",".join(CURVES))
    ap.add_argument("--windows", default="3,4,5")
    ap.add_argument("--size", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_mul.txt"))
    a = ap.parse_args()
    windows = [int(w) for w in a.windows.split(",") if w]
    n = 1 << a.size
    lib = ea.load_library()
    tel = bench.Telemetry(0)
    lines = ["# tools/point_mul_bench.py on %s: out[i] = s_i * P_i, 2^%d device-resident points, Affine output, median of 3 after 1 warm-up" % (
                 torch.cuda.get_device_name(0), a.size),
             "# clock / power: %s" % tel.describe(),
             "# curve what: device ms (events), host ms (the whole call), ns per point | clock, power"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for name in a.curves.split(","):
        curve = pm.CURVES[name]
        stride = curve.affine_stride
        d_pts = torch.from_numpy(ea.generate_points(n, seed=20, curve=name)).cuda()
        rng = np.random.default_rng(20)
        d_s = torch.from_numpy(rng.integers(0, 256, size=32 * n, dtype=np.uint8)).cuda()
        out = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
        ctx = ea.MultiScalarMultContext(name)
        host_ms = {}
        for w in windows:
            ctx.set_option("mul_window", w)
            tel.start()
            dev, host = time_mul(ctx, lib, d_pts, n, stride, d_s.data_ptr(), 32, 0, out)
            t = tel.stop()
            host_ms[w] = host
            emit("%s pairwise w=%d (chunk 2^%d): device %.3f ms, host %.3f ms, %.2f ns/point | %s, %s (%d samples)" % (
                name, w, ctx.query("mul_chunk").bit_length() - 1, dev, host, host * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"),
                t["samples"]))
        ctx.set_option("mul_window", 0)
        rbytes = ctypes.create_string_buffer(curve.r.to_bytes(32, "little"), 32)
        tel.start()
        dev_r, host_r = time_mul(ctx, lib, d_pts, n, stride, ctypes.addressof(rbytes), 32, 4, out)
        t = tel.stop()
        emit("%s uniform k=r: device %.3f ms, host %.3f ms, %.2f ns/point | %s, %s (%d samples)" % (
            name, dev_r, host_r, host_r * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"), t["samples"]))
        tel.start()
        dev_h, host_h = time_mul(ctx, lib, d_pts, n, stride, None, 0, 8, out)
        t = tel.stop()
        emit("%s uniform cofactor: device %.3f ms, host %.3f ms, %.2f ns/point | %s, %s (%d samples)" % (
            name, dev_h, host_h, host_h * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"), t["samples"]))
        dev, host = [], []
        tel.start()
        for it in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ctx.check_bases(d_pts, exact=True)
            t1 = time.perf_counter()
            assert res.ok
            if it:
                dev.append(res.device_us / 1000.0)
                host.append((t1 - t0) * 1000.0)
        t = tel.stop()
        chk = statistics.median(host)
        emit("%s check_bases(exact): device %.3f ms, host %.3f ms, %.2f ns/point | %s, %s (%d samples)" % (
            name, statistics.median(dev), chk, chk * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"), t["samples"]))
        for w in windows:
            emit("%s ratio pairwise w=%d / check_bases(exact): %.3f" % (name, w, host_ms[w] / chk))
        emit("%s ratio uniform k=r / check_bases(exact): %.3f" % (name, host_r / chk))
        emit("%s fastest window: w=%d" % (name, min(host_ms, key=host_ms.get)))
        ctx.close()
        del d_pts, d_s, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
