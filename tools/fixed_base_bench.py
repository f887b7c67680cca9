#!/usr/bin/env python3
"""Time batch fixed-base multiplication (WindowTable.msm, mi355_msm_fixed_*) per curve and window size, beside one MSM of the same
size on the same GPU; writes profiles/fixed_base.txt -- every line of that file comes from this script.

  python tools/fixed_base_bench.py [--curves a,b] [--windows 12,13,14,15,16,17,18] [--sizes 20,24,26] [--msm-sizes 20,24]
                                   [--out profiles/fixed_base.txt]

Per curve and window size: the table build (query "build_us", host clock around the build, and the table's bytes), then per size one
call with device scalars and a preallocated device output, median of three after one warm-up, on two clocks:
  device ms   query "last_device_us": between events on the stream the call ran on
  host ms     time.perf_counter around the call, which ends synchronised
with the GPU's shader clock and socket power sampled while the three ran (bench.py's Telemetry).  Then, per curve: the fastest window per
size, ns per output against ns per pair of one MSM of equal size (ctx.run on resident bases, context defaults, host clock), the
latency of a call with one scalar, and a host-pointer call of 2^24 scalars with its copies."""
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


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def random_scalars(n, seed):
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x0F                     # 252 bits: canonical on both families
    return sc


def time_call(table, lib, out, d_s, n, stride, reps=3):
    dev, host = [], []
    stream = torch.cuda.current_stream().cuda_stream
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        err = lib.mi355_msm_fixed_mul_device(table.handle, out.data_ptr(), stride, d_s.data_ptr(), n, 0, stream)
        t1 = time.perf_counter()
        assert err.code == 0
        if it:
            dev.append(table.query("last_device_us") / 1000.0)
            host.append((t1 - t0) * 1000.0)
    return statistics.median(dev), statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default=",".join(CURVES))
    ap.add_argument("--windows", default="12,13,14,15,16,17,18")
    ap.add_argument("--sizes", default="20,24,26")
    ap.add_argument("--msm-sizes", default="20,24")
    ap.add_argument("--host-size", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixed_base.txt"))
    a = ap.parse_args()
    windows = [int(w) for w in a.windows.split(",") if w]
    sizes = [int(s) for s in a.sizes.split(",") if s]
    msm_sizes = [int(s) for s in a.msm_sizes.split(",") if s]
    lib = ea.load_library()
    tel = bench.Telemetry(0)
    lines = ["# tools/fixed_base_bench.py on %s: out[i] = s_i * g, device scalars, Affine output, median of 3 after 1 warm-up" % torch.cuda.get_device_name(0),
             "# clock / power: %s" % tel.describe(),
             "# curve w: table build ms (host clock), table MB | per size: device ms (events), host ms (the whole call), ns per output | clock, power"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for name in a.curves.split(","):
        curve = pm.CURVES[name]
        img = curve.encode_affine(curve.generator())
        stride = curve.affine_stride
        nmax = 1 << max(sizes)
        d_s = torch.from_numpy(random_scalars(nmax, 1).reshape(-1)).cuda()
        out = torch.zeros((nmax, stride), dtype=torch.uint8, device="cuda")
        best = {}
        for w in windows:
            table = ea.FixedBase.get_window_table(img, curve=name, window=w)
            emit("%s w=%d: build %.2f ms, table %.1f MB, %d levels" % (name, w, table.query("build_us") / 1000.0, table.query("table_bytes") / 1e6,
                                                                    table.query("levels")))
            for logn in sizes:
                n = 1 << logn
                tel.start()
                dev, host = time_call(table, lib, out, d_s, n, stride)
                t = tel.stop()
                emit("%s w=%d 2^%d: device %.3f ms, host %.3f ms, %.2f ns/output | %s, %s (%d samples)" % (
                    name, w, logn, dev, host, host * 1e6 / n, fmt(t["clock_MHz_mean"], "MHz"), fmt(t["power_W_mean"], "W"), t["samples"]))
                if logn not in best or host < best[logn][1]:
                    best[logn] = (w, host)
            table.close()
        for logn, (w, host) in sorted(best.items()):
            emit("%s 2^%d fastest window: w=%d, %.3f ms" % (name, logn, w, host))
        # what a handle chooses by itself, one scalar, and host pointers
        table = ea.FixedBase.get_window_table(img, curve=name)
        w_auto = table.query("window_bits")
        one = [time_call(table, lib, out, d_s, 1, stride, reps=5) for _ in range(1)][0]
        emit("%s auto window w=%d; n = 1 latency: device %.3f ms, host %.3f ms" % (name, w_auto, one[0], one[1]))
        if a.host_size:
            n = 1 << a.host_size
            sc = random_scalars(n, 2)
            table.msm(sc[:1 << 16])
            t0 = time.perf_counter()
            table.msm(sc)
            emit("%s w=%d 2^%d host pointers (copies in and out included): %.1f ms, of which device-side %.1f ms" % (
                name, w_auto, a.host_size, (time.perf_counter() - t0) * 1e3, table.query("last_device_us") / 1000.0))
            del sc
        auto_ms = {}
        for logn in msm_sizes:
            auto_ms[logn] = time_call(table, lib, out, d_s, 1 << logn, stride)[1]
        table.close()
        del out
        for logn in msm_sizes:
            n = 1 << logn
            ctx = ea.MultiScalarMultContext(name)
            ctx.set_bases(ea.generate_points(n, curve=name))
            sc = d_s[:32 * n]
            ctx.run(sc)
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.run(sc)
                ts.append((time.perf_counter() - t0) * 1e3)
            ctx.close()
            msm_ms = statistics.median(ts)
            emit("%s 2^%d: fixed-base (w=%d) %.3f ms = %.2f ns/output; MSM %.3f ms = %.2f ns/pair; ratio %.2f" % (
                name, logn, w_auto, auto_ms[logn], auto_ms[logn] * 1e6 / n, msm_ms, msm_ms * 1e6 / n, auto_ms[logn] / msm_ms))
        del d_s
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
