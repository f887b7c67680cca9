#!/usr/bin/env python3
"""Time the point codec (k_decompress_points / k_compress_points) beside check_bases (endomorphism) on the same device-resident
points, per curve and size, and set_bases_compressed from host memory beside set_bases of the same points as images; writes
profiles/point_codec.txt -- every line of that file comes from this script.

  python tools/point_codec_bench.py [--sizes 20,24] [--curves ...] [--out profiles/point_codec.txt]

Per curve and size, median of five after one warm-up, on two clocks:
  device ms   out8[7] of the call: the codec (or check) kernels alone, between events on the context's stream
  host ms     time.perf_counter around the call, which ends synchronised: kernels + status bytes copied back and counted
with ns per point on the device clock and the GPU's shader clock and socket power sampled while the five ran (bench.py's Telemetry;
the line says so when the box offers neither).  The decompress / check ratio of a G1 curve is what tests/test_gpu_point_codec.py
guards.  The upload lines are single host-clock calls after one warm-up call of each: records or images in pageable host memory."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the clock / power sampler)
import entries_amd as ea  # noqa: E402

CURVES = ("bls12_377_g1", "bls12_381_g1", "bls12_377_g2", "bls12_381_g2")


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def timed(tel, fn):
    """median device ms, median host ms of five calls after one warm-up, telemetry of the five"""
    td, th = [], []
    for it in range(6):
        if it == 1:
            tel.start()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        assert r.ok
        if it:
            td.append(r.device_us / 1000.0)
            th.append((t1 - t0) * 1000.0)
    return statistics.median(td), statistics.median(th), tel.stop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--curves", default=",".join(CURVES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_codec.txt"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    tel = bench.Telemetry(0)
    lines = ["# tools/point_codec_bench.py on %s: device-resident valid points (generate_points), median of 5 after 1 warm-up" % torch.cuda.get_device_name(0),
             "# clock / power: %s" % tel.describe(),
             "# curve logn op: device ms (kernels alone), host ms (the whole call), ns per point (device) | clock, power while the five ran",
             "# then: decompress / check_bases on the device clock; upload lines: one host-clock call each, records / images in pageable host memory"]
    for name in a.curves.split(","):
        for logn in sizes:
            n = 1 << logn
            host_images = np.asarray(ea.generate_points(n, distinct=1 << 12, seed=9, curve=name)).reshape(-1)
            pts = torch.from_numpy(host_images).cuda()
            ctx = ea.MultiScalarMultContext(name)
            comp = ctx.compress_points(pts)
            assert comp.ok
            recs = comp.points
            back = ctx.decompress_points(recs)
            assert back.ok and torch.equal(back.points.reshape(-1), pts)      # what is timed is also right
            del back
            dev = {}
            for op, fn in (("decompress", lambda: ctx.decompress_points(recs)), ("compress", lambda: ctx.compress_points(pts)),
                           ("check_bases", lambda: ctx.check_bases(pts))):
                d, h, t = timed(tel, fn)
                dev[op] = d
                lines.append("%s 2^%d %s: device %.2f ms, host %.2f ms, %.1f ns/point | %s, %s (%d samples)" % (
                    name, logn, op, d, h, d * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"), t["samples"]))
                print(lines[-1], flush=True)
            lines.append("%s 2^%d decompress / check_bases (endomorphism), device clock: %.3f" % (name, logn, dev["decompress"] / dev["check_bases"]))
            print(lines[-1], flush=True)
            host_recs = recs.cpu().numpy().reshape(-1)
            ups = {}
            for what, fn in (("set_bases_compressed", lambda: ctx.set_bases_compressed(host_recs)), ("set_bases", lambda: ctx.set_bases(host_images))):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ups[what] = (time.perf_counter() - t0) * 1000.0
            lines.append("%s 2^%d upload from host memory: set_bases_compressed %.1f ms (%.0f MB), set_bases of the images %.1f ms (%.0f MB)" % (
                name, logn, ups["set_bases_compressed"], host_recs.nbytes / 1e6, ups["set_bases"], host_images.nbytes / 1e6))
            print(lines[-1], flush=True)
            ctx.close()
            del pts, recs, comp
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
