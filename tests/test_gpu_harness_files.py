"""GPU: the ZPrize FPGA harness's persisted data sets (tests/golden/harness/, TEST_LOAD_DATA_FROM layout) reproduced byte for byte.

scalars.bin holds normal-form integers a_i; the harness runs the MSM on their Fr limbs, the Montgomery images a_i * 2^256 mod r
(P1B hardcaml/zprize/msm_pippenger/test_fpga_harness/src/util.rs:72-140, tests/msm.rs:17-40).  The context option
"scalars_to_montgomery" does that conversion on the device (csrc/digits.hpp, fused into load_scalar); every path that hands scalars
to the grouping kernels is run with it -- device and host scalars, host pieces and carried chunks, run_async, both streaming
accumulators, a sharded context, and on BLS12-377 the Weierstrass / twisted-Edwards, plain / anchored and table paths -- and must
give arkworks_results.bin; without the option the random sets must miss every batch.  At scale the conversion is checked against
the fold-by-tile reference of tests/skew_cases.py (it is linear: the fold of the images is 2^256 * (sum a_i) mod r per tile point),
next to "scalars_montgomery" on the same workload; each run's plan numbers and wall time are printed as one JSON line."""
import json
import os
import time

import numpy as np
import pytest

import pymodel as m
import skew_cases as sk
from conftest import ROOT

pytestmark = pytest.mark.gpu

HDIR = os.path.join(ROOT, "tests", "golden", "harness")
SETS = {"377_g1_random": m.BLS12_377_G1, "377_g1_trivial": m.BLS12_377_G1, "381_g1_random": m.BLS12_381_G1}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _load(ea, name):
    return ea.formats.load_harness_dir(os.path.join(HDIR, name), SETS[name].name)


def _serialized(ea, curve, results):
    return [ea.formats.point_to_serialized(r, curve.name) for r in results]


def _affine_images(curve, data):
    """the data set's bases as the FFI's affine images (the streaming accumulators take those)"""
    cb = curve.coord_bytes
    pts = []
    for i in range(data.n):
        rec = data.records[i * 2 * cb:(i + 1) * 2 * cb]
        pts.append(None if rec[-1] & 0x40 else (int.from_bytes(rec[:cb], "little"),
                                                int.from_bytes(rec[cb:2 * cb - 1] + bytes([rec[-1] & 0x3F]), "little")))
    return curve.encode_affine_array(pts)


@pytest.mark.parametrize("name", sorted(SETS))
def test_harness_data_sets_through_every_path(ea, torch_cuda, name):
    torch = torch_cuda
    curve = SETS[name]
    f = ea.formats
    data = _load(ea, name)
    exp = data.expected

    def fresh(devices=None, **opts):
        ctx = ea.MultiScalarMultContext(curve.name, devices=devices)
        for k, v in opts.items():
            ctx.set_option(k, v)
        return ctx

    # host scalars (run_harness_dir): default plan, then pieces of the first batch and carried chunks
    for opts in ({}, {"max_chunk": 300, "first_piece_div": 4}):
        ctx = fresh(**opts)
        assert f.run_harness_dir(ctx, data) == [True] * 4, (name, "host scalars", opts)
        # without the option: the file's integers as they are -- what the package did before -- miss every batch
        assert f.run_harness_dir(ctx, data, to_montgomery=False) == [False] * 4, (name, "negative control", opts)
        ctx.close()
    # device-resident scalars, synchronous and stream-ordered
    dev = torch.frombuffer(bytearray(data.scalars), dtype=torch.uint8).cuda()
    ctx = fresh()
    assert f.run_harness_dir(ctx, data, scalars=dev) == [True] * 4, (name, "device scalars")
    job = ctx.run_async(dev, data.n)
    assert _serialized(ea, curve, job.wait()) == exp, (name, "run_async")
    # the two options exclude each other (-1), whichever comes second
    with pytest.raises(ea.MsmError) as e:
        ctx.set_option("scalars_montgomery", 1)
    assert e.value.code == -1
    ctx.set_option("scalars_to_montgomery", 0)
    ctx.set_option("scalars_montgomery", 1)
    with pytest.raises(ea.MsmError) as e:
        ctx.set_option("scalars_to_montgomery", 1)
    assert e.value.code == -1
    ctx.close()
    # a sharded context (three logical shards on one GPU): the option reaches every shard
    ctx = fresh(devices=[0, 0, 0])
    assert f.run_harness_dir(ctx, data) == [True] * 4, (name, "sharded, host scalars")
    assert f.run_harness_dir(ctx, data, scalars=dev) == [True] * 4, (name, "sharded, device scalars")
    ctx.close()
    # the streaming accumulators: each batch through add() in uneven slices, several flushes
    bases = _affine_images(curve, data)
    stride = curve.affine_stride
    for cls in (ea.ChunkedPippenger, ea.HashMapPippenger):
        for b in range(data.batches):
            acc = cls(100, curve.name)
            acc.set_option("scalars_to_montgomery", 1)
            with pytest.raises(ea.MsmError):
                acc.set_option("scalars_montgomery", 1)
            sc = data.scalars[b * data.n * 32:(b + 1) * data.n * 32]
            for lo, hi in ((0, 77), (77, 700), (700, data.n)):
                lo, hi = min(lo, data.n), min(hi, data.n)
                acc.add(bases[lo * stride:hi * stride], sc[lo * 32:hi * 32])
            got = acc.finalize()
            if cls is ea.ChunkedPippenger:
                assert acc.query("flushes") >= -(-data.n // 100)
            assert f.point_to_serialized(got, curve.name) == exp[b], (name, cls.__name__, b)
            acc.close()
    if curve.curve_id == 0:
        for opts in ({"twisted_edwards": 0}, {"twisted_edwards": 1}, {"anchor": 0}, {"anchor": 2},
                     {"precompute": 1, "table_levels": 6}, {"precompute": 1, "table_levels": 6, "twisted_edwards": 0, "anchor": 2}):
            ctx = fresh(**opts)
            assert f.run_harness_dir(ctx, data) == [True] * 4, (name, opts)
            assert f.run_harness_dir(ctx, data, scalars=dev) == [True] * 4, (name, opts, "device")
            if "twisted_edwards" in opts:
                assert ctx.query("twisted_edwards") == opts["twisted_edwards"], opts
            if opts.get("precompute"):
                assert ctx.query("table_levels") == 6, opts
            ctx.close()


# ------------------------------------------------------------------------------------------------------------------------ at scale

def _uniform_below_r(cid, n, seed):
    rng = np.random.default_rng(seed)
    limbs = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    limbs[:, 3] %= np.uint64(sk.r_of(cid) >> 192)           # < r (and uniform images for the from-Montgomery run)
    return limbs.view(np.uint8).reshape(n, 32)


def _times(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, sorted(ts)[len(ts) // 2]


@pytest.mark.parametrize("cid,npow", [(0, 26), (1, 24)])
def test_montgomery_entries_at_scale(ea, oracle, torch_cuda, cid, npow):
    """4 host batches of 2^26 (BLS12-377, the harness's own shape) / 2^24 (BLS12-381) pairs, bases a tile of D points repeated on the
    device.  Batch b is batch 0 rotated by b rows, so its tile fold is batch 0's rotated by b.  The same scalars run plain (fold F),
    as normal-form integers with scalars_to_montgomery (R F mod r) and as Montgomery images with scalars_montgomery (R^-1 F mod r)."""
    torch = torch_cuda
    n, D = 1 << npow, 1 << 12
    r = sk.r_of(cid)
    R = (1 << 256) % r
    tile = sk.random_tile(ea, cid, D, seed=700 + cid, infinity_at=5)
    s0 = _uniform_below_r(cid, n, 90 + cid)
    host = np.empty((4 * n, 32), dtype=np.uint8)
    for b in range(4):
        host[b * n:(b + 1) * n] = np.roll(s0, b, axis=0)
    f0 = [int.from_bytes(row.tobytes(), "little") for row in sk.fold_scalars(cid, s0, D)]

    def reference(mult):
        out = []
        for b in range(4):
            fb = np.roll(np.array([sk._int_row(x * mult % r) for x in f0], dtype=np.uint8), b, axis=0)
            out.append(sk.oracle_msm(oracle, cid, tile, fb))
        return out

    ctx = ea.MultiScalarMultContext(sk.NAMES[cid])
    ctx.set_bases(torch.from_numpy(tile).cuda().repeat(n // D, 1).contiguous())
    dev = torch.from_numpy(s0).cuda()
    for label, opt, mult in (("plain", None, 1), ("scalars_to_montgomery", "scalars_to_montgomery", R),
                             ("scalars_montgomery", "scalars_montgomery", pow(R, -1, r))):
        for k in ("scalars_to_montgomery", "scalars_montgomery"):
            ctx.set_option(k, 0)
        if opt:
            ctx.set_option(opt, 1)
        exp = reference(mult)
        got, host_ms = _times(lambda: ctx.run(host), reps=1 if npow == 26 else 2)
        assert got == exp, (sk.NAMES[cid], label, "host batches")
        t = ctx.last_timings()
        chunks = t["launches"]
        got, dev_ms = _times(lambda: ctx.run(dev), reps=3)
        assert got == exp[:1], (sk.NAMES[cid], label, "device scalars")
        t = ctx.last_timings()
        print(json.dumps(dict(label=f"{sk.NAMES[cid]} 2^{npow} {label}", n=n, batches=4, host_batches_ms=round(host_ms, 1),
                              host_chunks=chunks, device_batch_ms=round(dev_ms, 2), window_bits=t["window_bits"], windows=t["windows"],
                              lane_entries=t["lane_entries"], lanes=t["lanes"], anchored_window=ctx.query("anchored_window"),
                              te=t["twisted_edwards"])))
    ctx.close()
