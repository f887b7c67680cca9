#!/usr/bin/env python3
"""Time MultiScalarMultContext.check_bases (k_check_points) on device-resident valid points, both methods, all four curves, beside one
MSM of the same size on the same GPU; writes profiles/check_points.txt -- every line of that file comes from this script.

  python tools/check_points_bench.py [--sizes 20,24] [--g1-extra 26] [--out profiles/check_points.txt] [--remarks FILE]

Per curve, size and method, median of five after one warm-up, on two clocks:
  device ms   out[7] of mi355_msm_check_bases: the check kernels alone, between events on the context's stream
  host ms     time.perf_counter around the call, which ends synchronised: kernels + the status bytes copied back and counted
with the GPU's shader clock and socket power sampled while the five ran (bench.py's Telemetry; the line says so when the box offers
neither).  Then the exact / endomorphism ratio beside the ratio of modelled field multiplications, and the check / MSM ratio on the
HOST clock for both (one ctx.run of n pairs after a warm-up run, result copy included).
The rule for the default method: endomorphism where this file shows it faster than exact on that curve.

Last, the registers, scratch and occupancy of every k_check_points instantiation from the compiler's resource remarks: the script
compiles csrc/kernels_check.hip with build.py's flags plus -Rpass-analysis=kernel-resource-usage while the measurements run
(--remarks FILE: read the remarks of such a compile from FILE instead)."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402  (the clock / power sampler)
import entries_amd as ea  # noqa: E402

CURVES = ("bls12_377_g1", "bls12_381_g1", "bls12_377_g2", "bls12_381_g2")
# field multiplications (squarings counted as one) of the scalar multiplications: dbl-2008-s-1 = 9, madd-2008-s = 10, add-2008-s = 14;
# exact: bits(r) - 1 doublings and weight(r) - 1 mixed additions; [u]: 63 doublings and weight(u) - 1 additions
MODEL = {
    "bls12_377_g1": {"exact": 252 * 9 + 87 * 10, "endomorphism": 126 * 9 + 6 * 10 + 6 * 14},
    "bls12_381_g1": {"exact": 254 * 9 + 133 * 10, "endomorphism": 126 * 9 + 5 * 10 + 5 * 14},
    "bls12_377_g2": {"exact": 252 * 9 + 87 * 10, "endomorphism": 63 * 9 + 6 * 10},
    "bls12_381_g2": {"exact": 254 * 9 + 133 * 10, "endomorphism": 63 * 9 + 5 * 10},
}
REMARK_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-Rpass-analysis=kernel-resource-usage"]


def start_remarks_compile(tmp):
    """hipcc on csrc/kernels_check.hip with the product's flags + the remarks flag; -> (process, path of its stderr)"""
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    log = os.path.join(tmp, "remarks.txt")
    cmd = [hipcc] + REMARK_FLAGS + ["-c", os.path.join(ROOT, "2022-entries_amd", "csrc", "kernels_check.hip"), "-o", os.path.join(tmp, "kernels_check.o")]
    return subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=open(log, "w")), log


def resource_lines(remarks):
    rows = []
    pat = (r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)"
           r".*?Occupancy \[waves/SIMD\]: (\d+)")
    for m in re.finditer(pat, remarks, flags=re.S):
        k = re.search(r"k_check_pointsINS_\d(Fp2?El)INS_12(Bls12_3\d\d)_Fq(?:ELi\d)?EEELb(\d)ELi(\d)", m.group(1))
        if k:
            rows.append("%s %s %s %s: VGPRs %s AGPRs %s SGPRs %s scratch %s occupancy %s" % (
                k.group(2).lower(), "g1" if k.group(1) == "FpEl" else "g2", "serialized" if k.group(3) == "1" else "in-memory",
                "endomorphism" if k.group(4) == "1" else "exact", m.group(3), m.group(4), m.group(2), m.group(5), m.group(6)))
    return sorted(rows)


def fmt(v, unit):
    return "n/a" if v is None else "%.0f %s" % (v, unit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,24")
    ap.add_argument("--g1-extra", type=int, default=26)
    ap.add_argument("--curves", default=",".join(CURVES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_points.txt"))
    ap.add_argument("--remarks", default=None, help="stderr of a hipcc compile of kernels_check.hip with " + REMARK_FLAGS[-1])
    a = ap.parse_args()
    tmp = tempfile.TemporaryDirectory()
    proc = log = None
    if not a.remarks:
        proc, log = start_remarks_compile(tmp.name)
    sizes = [int(s) for s in a.sizes.split(",") if s]
    tel = bench.Telemetry(0)
    lines = ["# tools/check_points_bench.py on %s: check_bases on device-resident valid points (generate_points), median of 5 after 1 warm-up"
             % torch.cuda.get_device_name(0),
             "# clock / power: %s" % tel.describe(),
             "# curve logn method: device ms (kernels alone), host ms (the whole call), points/s on the host clock | clock, power while the five ran",
             "# then: exact/endo measured (device), modelled | endo check / MSM, both on the host clock (one ctx.run of n pairs)"]
    for name in a.curves.split(","):
        logs = sizes + ([a.g1_extra] if name.endswith("g1") and a.g1_extra and a.g1_extra not in sizes else [])
        for logn in logs:
            n = 1 << logn
            pts = torch.from_numpy(np.asarray(ea.generate_points(n, distinct=1 << 12, seed=9, curve=name)).reshape(-1)).cuda()
            ctx = ea.MultiScalarMultContext(name)
            dev, host = {}, {}
            for method in ("endomorphism", "exact"):
                td, th = [], []
                for it in range(6):
                    if it == 1:
                        tel.start()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r = ctx.check_bases(pts, exact=method == "exact")
                    t1 = time.perf_counter()
                    assert r.ok and r.method == method
                    if it:
                        td.append(r.device_us / 1000.0)
                        th.append((t1 - t0) * 1000.0)
                t = tel.stop()
                dev[method], host[method] = statistics.median(td), statistics.median(th)
                lines.append("%s 2^%d %s: device %.2f ms, host %.2f ms, %.3e points/s | %s, %s (%d samples)" % (
                    name, logn, method, dev[method], host[method], n / (host[method] / 1000.0), fmt(t["clock_MHz_mean"], "MHz"),
                    fmt(t["power_W_mean"], "W"), t["samples"]))
                print(lines[-1], flush=True)
            ctx.set_bases(pts)
            rng = np.random.default_rng(1)
            sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
            sc[:, 31] &= 0x0F
            dsc = torch.from_numpy(sc).cuda()
            ctx.run(dsc)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.run(dsc)
            msm_ms = (time.perf_counter() - t0) * 1000.0
            ctx.close()
            del pts, dsc
            lines.append("%s 2^%d exact/endo measured %.2f modelled %.2f | endo/MSM %.2f (MSM %.2f ms host) | faster: %s"
                         % (name, logn, dev["exact"] / dev["endomorphism"], MODEL[name]["exact"] / MODEL[name]["endomorphism"],
                            host["endomorphism"] / msm_ms, msm_ms, "endomorphism" if dev["endomorphism"] < dev["exact"] else "exact"))
            print(lines[-1], flush=True)
    if proc is not None:
        if proc.wait() != 0:
            raise SystemExit("the remarks compile of kernels_check.hip failed:\n" + open(log).read()[-2000:])
        remarks = open(log).read()
    else:
        remarks = open(a.remarks).read()
    rows = resource_lines(remarks)
    lines.append("# k_check_points, compiler resource remarks (hipcc %s csrc/kernels_check.hip): registers per lane, scratch bytes per lane, waves per SIMD"
                 % " ".join(REMARK_FLAGS))
    lines += rows if rows else ["# (no k_check_points remark found)"]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    tmp.cleanup()


if __name__ == "__main__":
    main()
