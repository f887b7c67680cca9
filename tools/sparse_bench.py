#!/usr/bin/env python3
"""Time y = M z on resident sparse matrices (mi355_msm_sparse_apply with device pointers) per scalar field beside the forward NN
transform of 2^20 elements and a device-to-device copy of the bytes apply moves; writes profiles/sparse.txt -- every line of that file
comes from this script.

  python tools/sparse_bench.py [--fields a,b] [--sizes 20,22] [--out profiles/sparse.txt]

rows = cols = 2^size, nnz = 4 rows, random coefficients, columns and z; two matrices of the same nnz:
  uniform   4 entries a row
  skewed    one row of nnz / 2 entries, 2^10 rows of 2^10, the rest spread evenly over the other rows, in a seeded order
Device-resident z, a preallocated output, median of five after one warm-up, on two clocks:
  device ms   the domain's query "last_device_us": between events on the stream the call ran on
  host ms     time.perf_counter around the call, which ends synchronised
The `ratio apply uniform` and `ratio apply skewed` lines of BLS12-381 at 2^20 (host clock, over the transform of 2^20) are what
tests/test_gpu_sparse.py takes its speed bounds from."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
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


def row_lengths(rows, nnz, seed):
    rng = np.random.default_rng(seed)
    uniform = np.full(rows, nnz // rows, dtype=np.int64)
    left = nnz - nnz // 2 - (1 << 20)
    others = rows - 1 - (1 << 10)
    rest = np.full(others, left // others, dtype=np.int64)
    rest[:left - int(rest.sum())] += 1
    skewed = np.concatenate([[nnz // 2], np.full(1 << 10, 1 << 10, dtype=np.int64), rest])
    rng.shuffle(skewed)
    return ("uniform", uniform), ("skewed", skewed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fields", default="bls12_377,bls12_381")
    ap.add_argument("--sizes", default="20,22")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse.txt"))
    a = ap.parse_args()
    lines = ["# tools/sparse_bench.py on %s; device-resident data, median of 5 after a warm-up; ms device (events) / ms host clock" % torch.cuda.get_device_name(0)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for field in a.fields.split(","):
        dom = ea.Radix2EvaluationDomain(1 << NTT_LOG, CURVE_OF[field])
        g = torch.Generator(device="cuda")
        g.manual_seed(NTT_LOG)
        x = torch.randint(0, 256, (1 << NTT_LOG, 32), dtype=torch.uint8, device="cuda", generator=g)
        y = torch.empty_like(x)
        d_ntt, h_ntt = timed(lambda: dom.fft(x, out=y), dom)
        say("%s 2^%d forward NN                 %8.3f / %8.3f ms" % (field, NTT_LOG, d_ntt, h_ntt))
        for k in [int(s) for s in a.sizes.split(",")]:
            rows = cols = 1 << k
            nnz = 4 * rows
            rng = np.random.default_rng(k)
            values = rng.integers(0, 256, size=(nnz, 32), dtype=np.uint8)
            col_idx = rng.integers(0, cols, size=nnz, dtype=np.uint32)
            g.manual_seed(k + 100)
            z = torch.randint(0, 256, (cols, 32), dtype=torch.uint8, device="cuda", generator=g)
            out = torch.empty((rows, 32), dtype=torch.uint8, device="cuda")
            # what apply reads and writes: z in and its class-M copy out; two passes over coefficient, column and the gathered element;
            # a total and a prefix per lane, twice each; the output
            moved = 64 * cols + 2 * nnz * (32 + 4 + 32) + 4 * 32 * (nnz // 16) + 32 * rows
            src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            _, h_copy = timed(lambda: dst.copy_(src))
            say("%s 2^%d device-to-device copy      %8s / %8.3f ms (%d bytes read + written, %.0f GB/s)" % (field, k, "", h_copy, moved, moved / (h_copy * 1e-3) / 1e9))
            del src, dst
            for which, lens in row_lengths(rows, nnz, 0xD15C):
                row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
                t0 = time.perf_counter()
                M = dom.sparse_matrix(rows, cols, row_ptr, col_idx, values)
                t_create = (time.perf_counter() - t0) * 1e3
                d, h = timed(lambda: M.apply(z, out=out), dom)
                say("%s 2^%d apply %-20s %8.3f / %8.3f ms   %.2f x forward NN 2^%d, %.2f x copy, %.0f GB/s, %.3f ns per entry; create %.0f ms, work_bytes %d"
                    % (field, k, which, d, h, h / h_ntt, NTT_LOG, h / h_copy, moved / (d * 1e-3) / 1e9, h * 1e6 / nnz, t_create, M.query("work_bytes")))
                say("%s ratio apply %s 2^%d / forward NN 2^%d: %.4f" % (field, which, k, NTT_LOG, h / h_ntt))
                M.close()
            del z, out
            torch.cuda.empty_cache()
        dom.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
