"""GPU: the -DMSM_DEBUG build (libmi355msm_debug.so, see test_gpu_debug_build.py) on skewed scalars -- its device-side invariant checks
(segment tables, sorted keys, the entry count against an independent count of the non-zero digits, slot keys) on the long-segment paths:
all scalars equal (the default plan and c = 22: two generic passes), the same digit in every window over six shared table levels, and
mostly-zero scalars under the anchored window (the default one on BLS12-381 G1; option anchor = 2 on BLS12-377, whose 2^20 plans have
none).  Every result equals the fold-by-tile reference (tests/skew_cases.py).

Run in a subprocess so that the product library of this test session and the debug build never share a process."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SCRIPT = r"""
import ctypes, json, os, sys
sys.path.insert(0, os.environ["REPO"])
sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import torch
import entries_amd as ea
import skew_cases as sk
lib = ea.load_library()
assert b"+debug-invariants" in lib.mi355_msm_version(), lib.mi355_msm_version()
oracle = ctypes.CDLL(os.path.join(os.environ["REPO"], "oracle", "liboracle.so"))
oracle.oracle_msm.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
out = {}
for cid, npow in ((0, 20), (1, 20), (2, 18)):
    n, D = 1 << npow, 1 << 10
    name = sk.NAMES[cid]
    tile = sk.random_tile(ea, cid, D, seed=700 + cid)
    bases = torch.from_numpy(tile).cuda().repeat(n // D, 1).contiguous()
    c_default = ea.plan(n, name)["window_bits"]
    # zeros_90 under an anchored window: the default one where the plan has it (BLS12-381 from c = 15), else the option's "always" (2)
    anchored = sk.anchor_window(c_default, sk.scalar_bits(cid)) is not None
    cases = [("all_equal", {}), ("all_equal", {"window_bits": 22}), ("zeros_90", {} if anchored else {"anchor": 2})]
    if cid < 2:   # (no G2 tables in the product's test matrix either: test_gpu_debug_build.py)
        cases.append(("window_periodic", {"precompute": 1, "table_levels": 6}))
    for gen, opts in cases:
        ctx = ea.MultiScalarMultContext(name)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.set_bases(bases)
        c = ctx.query("table_window_bits") if opts.get("precompute") else c_default
        sc = sk.make_scalars(gen, cid, n, 40 + cid, c=c)
        got = ctx.run(torch.from_numpy(sc).cuda())[0]
        checks = ctx.query("debug_checks")
        info = dict(gen=gen, opts=opts, checks=checks, window_bits=ctx.last_timings()["window_bits"], group_passes=ctx.query("group_passes"),
                    bucket_windows=ctx.query("bucket_windows"), anchored_window=ctx.query("anchored_window"))
        ctx.close()
        assert checks >= 3, (name, info)     # level 1, the sorted output + digit count, the slot keys: per chunk
        assert got == sk.fold_reference(oracle, cid, tile, sc), (name, info)
        if opts.get("window_bits") == 22:
            assert info["group_passes"] == 2, info
        if gen == "zeros_90":
            assert info["anchored_window"] > 0, info
        if opts.get("precompute"):
            assert info["bucket_windows"] < (257 + c - 1) // c, info
        out.setdefault(name, []).append(info)
print("DEBUG_SKEW_OK " + json.dumps(out))
"""


def test_debug_build_holds_its_invariants_on_skewed_scalars(built):
    assert os.path.exists(os.path.join(ROOT, "2022-entries_amd", "libmi355msm_debug.so")), "build.py builds it beside the product"
    env = dict(os.environ, REPO=ROOT, MI355_MSM_LIBRARY="libmi355msm_debug.so")
    r = subprocess.run([sys.executable, "-c", SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEBUG_SKEW_OK ")]
    assert line, r.stdout[-2000:]
    runs = json.loads(line[0][len("DEBUG_SKEW_OK "):])
    assert set(runs) == {"bls12_377_g1", "bls12_381_g1", "bls12_377_g2"}
    print(json.dumps(runs))
