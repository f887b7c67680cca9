"""GPU: skewed and degenerate scalars at the sizes the library is built for (2^20 .. 2^26 pairs), every result checked against the exact
fold-by-tile reference of tests/skew_cases.py (bases = a tile of D points repeated on the device).

What these inputs reach that uniform scalars do not: segments longer than PART_SUBJOB in the grouping passes (sub-jobs), in a second pass
(c = 22) and in the merged segments of shared table levels; one hot bucket spread over thousands of accumulate lanes whose fragments are
EQUAL points (all bases equal: the merges must double) or cancel (Q / -Q); the default anchored window on mostly-zero scalars; the K fit
and the host-scalar pieces of a batch on non-uniform entry counts.  Coverage is asserted, not assumed: the hot bucket of every run that is
meant to have one is measured with the digit model (skew_cases.hot_spots) against PART_SUBJOB and the entries per lane, the model's entry
count is checked against the device's, and the anchored window against the engine's rule.  The plan numbers of every run are printed as
one JSON line each (pytest -s shows them)."""
import json

import numpy as np
import pytest

import skew_cases as sk

pytestmark = pytest.mark.gpu

SUBJOB = sk.part_subjob()
HOT = ("all_equal", "all_one", "r_minus_1", "two_values", "witness", "window_periodic")   # a bucket of >= n / 2 entries on any plan


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _device_bases(torch, tile, n):
    return torch.from_numpy(tile).cuda().repeat(n // len(tile), 1).contiguous()


_MODEL = {}


def _plan(ctx, label, n, sc=None, prefix=None):
    """the run's plan numbers; with `sc` (device scalars, plain digits) the digit model's hot bucket, longest level-1 segment and entry
    count -- on the first `prefix` pairs only where a whole batch would take too long (a lower bound then), else on all of them, and the
    entry count checked against the device's"""
    t = ctx.last_timings()
    rec = dict(label=label, n=n, window_bits=t["window_bits"], windows=t["windows"], lane_entries=t["lane_entries"], lanes=t["lanes"],
               chunks=t["launches"], group_passes=ctx.query("group_passes"), l1_bits=ctx.query("l1_bits"), l1_bins=ctx.query("l1_bins"),
               bucket_windows=ctx.query("bucket_windows"), anchored_window=ctx.query("anchored_window"), te=t["twisted_edwards"],
               part_subjob=SUBJOB)
    if sc is not None and ctx.query("assume_subgroup") == 0:
        anchor = rec["anchored_window"] - 1 if rec["anchored_window"] else None
        m = len(sc) if prefix is None else prefix
        key = (sc.ctypes.data, m, rec["window_bits"], rec["bucket_windows"], rec["l1_bits"], anchor)
        if key not in _MODEL:
            _MODEL.clear()
            _MODEL[key] = sk.hot_spots(sc[:m], rec["window_bits"], rec["bucket_windows"], rec["l1_bits"], anchor)
        hot, seg, entries = _MODEL[key]
        rec.update(model_pairs=m, hot_bucket=hot, longest_l1_segment=seg, hot_lanes=hot // rec["lane_entries"])
        if rec["chunks"] == 1 and m == len(sc):
            assert ctx.query("sorted_entries") == entries, (label, "the digit model and the device disagree on the entry count")
    print(json.dumps(rec))
    return rec


def _assert_hot(rec):
    """the run had the paths this file is about: a bucket (hence a segment of every pass) longer than a sub-job, over >= 64 lanes"""
    assert rec["hot_bucket"] > SUBJOB, (rec, "no segment longer than PART_SUBJOB")
    assert rec["longest_l1_segment"] > SUBJOB, rec
    assert rec["hot_lanes"] >= 64, (rec, "the hot bucket spans fewer than 64 accumulate lanes")


def _assert_te(ctx, cid, rec):
    if cid == 0:
        assert ctx.query("twisted_edwards") == 1 and rec["te"], rec
        assert ctx.query("twisted_edwards_fallbacks") == 0, rec


def _run_dev(torch, ctx, sc):
    return ctx.run(torch.from_numpy(sc).cuda())


# ------------------------------------------------------------------------------------------------------------------------ 2^22

@pytest.mark.parametrize("cid", [0, 1])
def test_every_generator_at_2_22(ea, oracle, torch_cuda, cid):
    """Every generator at 2^22 pairs on a 4096-point tile, default options and anchor = 0, device scalars (one chunk)."""
    n, D = 1 << 22, 1 << 12
    bits = sk.scalar_bits(cid)
    tile = sk.random_tile(ea, cid, D, seed=100 + cid)
    ctx = ea.MultiScalarMultContext(sk.NAMES[cid])
    ctx.set_bases(_device_bases(torch_cuda, tile, n))
    c_default = ea.plan(n, sk.NAMES[cid])["window_bits"]
    anchored = []
    for i, name in enumerate(list(sk.GENERATORS) + ["window_periodic"]):
        sc = sk.make_scalars(name, cid, n, seed=200 + i, c=c_default)
        exp = sk.fold_reference(oracle, cid, tile, sc)
        got = {}
        for anchor in (1, 0):
            ctx.set_option("anchor", anchor)
            got[anchor] = _run_dev(torch_cuda, ctx, sc)[0]
            rec = _plan(ctx, f"{sk.NAMES[cid]} 2^22 {name} anchor={anchor}", n, sc)
            assert rec["chunks"] == 1, rec
            a = sk.anchor_window(rec["window_bits"], bits) if anchor else None
            assert rec["anchored_window"] == (0 if a is None else a + 1), (rec, "not the engine's anchored-window rule")
            if anchor and a is not None:
                anchored.append(name)
            _assert_te(ctx, cid, rec)
            if name in HOT or (anchor and a is not None and name in ("all_zero", "zeros_90", "short64")):
                _assert_hot(rec)
        assert got[1] == exp, (sk.NAMES[cid], name, "default options")
        assert got[0] == exp, (sk.NAMES[cid], name, "anchor = 0")
    ctx.close()
    print(sk.NAMES[cid], "2^22 anchored runs:", anchored)


# ------------------------------------------------------------------------------------------------------------------------ 2^20

@pytest.mark.parametrize("cid", [0, 1])
def test_targeted_paths_at_2_20(ea, oracle, torch_cuda, cid):
    torch = torch_cuda
    n, D = 1 << 20, 1 << 10
    name = sk.NAMES[cid]
    tile = sk.random_tile(ea, cid, D, seed=300 + cid)
    bases = _device_bases(torch, tile, n)

    def fresh(**opts):
        ctx = ea.MultiScalarMultContext(name)
        for k, v in opts.items():
            ctx.set_option(k, v)
        return ctx

    # two generic passes (c = 22) with the whole window in one segment
    sc = sk.make_scalars("all_equal", cid, n, 1)
    exp = sk.fold_reference(oracle, cid, tile, sc)
    ctx = fresh(window_bits=22)
    ctx.set_bases(bases)
    assert _run_dev(torch, ctx, sc)[0] == exp
    rec = _plan(ctx, f"{name} 2^20 all_equal c=22", n, sc)
    assert rec["window_bits"] == 22 and ctx.query("group_passes") == 2, rec
    _assert_hot(rec)
    _assert_te(ctx, cid, rec)
    ctx.close()

    # shared table levels: every window's digit in ONE bucket of the merged level-1 segments (k_l1_merge_shared)
    ctx = fresh(precompute=1, table_levels=6)
    ctx.set_bases(bases)
    c = ctx.query("table_window_bits")
    sc = sk.make_scalars("window_periodic", cid, n, 2, c=c)
    exp = sk.fold_reference(oracle, cid, tile, sc)
    assert _run_dev(torch, ctx, sc)[0] == exp
    rec = _plan(ctx, f"{name} 2^20 window_periodic tables=6", n, sc)
    assert rec["bucket_windows"] < rec["windows"], rec
    assert rec["hot_bucket"] >= 2 * n, (rec, "the shared bucket should merge several windows")
    _assert_hot(rec)
    _assert_te(ctx, cid, rec)
    ctx.close()

    # the fold path (assume_subgroup): r - 1 runs as 1 x (-P)
    ctx = fresh(assume_subgroup=1)
    ctx.set_bases(bases)
    for gen in ("r_minus_1", "all_equal"):
        sc = sk.make_scalars(gen, cid, n, 3)
        assert _run_dev(torch, ctx, sc)[0] == sk.fold_reference(oracle, cid, tile, sc), gen
        _plan(ctx, f"{name} 2^20 {gen} assume_subgroup", n)
    ctx.close()

    # equal points (one base) and cancelling points (Q, -Q) in the hot bucket's fragments, quad merges off and for everything
    for label, t, sc in (("same_base", sk.same_base_tile(ea, cid, 4), sk.make_scalars("all_equal", cid, n, 4)),
                         ("cancel", sk.cancel_tile(ea, cid, 5), sk.make_scalars("all_equal", cid, n, 5))):
        exp = sk.fold_reference(oracle, cid, t, sc)
        for ql in (0, 1 << 24):
            ctx = fresh(quad_limit=ql)
            ctx.set_bases(_device_bases(torch, t, n))
            assert _run_dev(torch, ctx, sc)[0] == exp, (label, ql)
            rec = _plan(ctx, f"{name} 2^20 {label} quad_limit={ql}", n, sc)
            _assert_hot(rec)
            _assert_te(ctx, cid, rec)
            ctx.close()

    # carried chunks
    sc = sk.make_scalars("witness", cid, n, 6)
    exp = sk.fold_reference(oracle, cid, tile, sc)
    ctx = fresh(max_chunk=n // 3 + 1)
    ctx.set_bases(bases)
    assert _run_dev(torch, ctx, sc)[0] == exp
    assert ctx.run(sc)[0] == exp, "host scalars"
    rec = _plan(ctx, f"{name} 2^20 witness max_chunk=n/3+1", n)
    assert rec["chunks"] == 3, rec
    ctx.close()

    if cid == 0:
        # the twisted-Edwards accumulation against the XYZZ one on the same skewed inputs
        ws = sk.make_scalars("witness", cid, n, 7)
        for label, t, sc in (("witness", tile, ws), ("same_base", sk.same_base_tile(ea, cid, 4), sk.make_scalars("all_equal", cid, n, 4)),
                             ("cancel", sk.cancel_tile(ea, cid, 5), sk.make_scalars("all_equal", cid, n, 5))):
            exp = sk.fold_reference(oracle, cid, t, sc)
            b = _device_bases(torch, t, n)
            for te in (0, 1):
                ctx = fresh(twisted_edwards=te)
                ctx.set_bases(b)
                assert _run_dev(torch, ctx, sc)[0] == exp, (label, te)
                rec = _plan(ctx, f"{name} 2^20 {label} twisted_edwards={te}", n)
                assert rec["te"] == bool(te), rec
                if te:
                    _assert_te(ctx, cid, rec)
                ctx.close()


# ------------------------------------------------------------------------------------------------------------------------ 2^24

@pytest.mark.parametrize("cid", [0, 1])
def test_skewed_at_2_24(ea, oracle, torch_cuda, cid):
    torch = torch_cuda
    n = 1 << 24
    name, bits = sk.NAMES[cid], sk.scalar_bits(cid)
    cases = (("witness", sk.random_tile(ea, cid, 1 << 12, seed=400 + cid), sk.make_scalars("witness", cid, n, 8)),
             ("same_base", sk.same_base_tile(ea, cid, 9), sk.make_scalars("all_equal", cid, n, 9)),
             ("cancel", sk.cancel_tile(ea, cid, 10), sk.make_scalars("all_equal", cid, n, 10)))
    for label, tile, sc in cases:
        ctx = ea.MultiScalarMultContext(name)
        ctx.set_bases(_device_bases(torch, tile, n))
        assert _run_dev(torch, ctx, sc)[0] == sk.fold_reference(oracle, cid, tile, sc), label
        rec = _plan(ctx, f"{name} 2^24 {label}", n, sc, prefix=n // 8)
        a = sk.anchor_window(rec["window_bits"], bits)
        assert rec["anchored_window"] == (0 if a is None else a + 1), rec
        _assert_hot(rec)
        _assert_te(ctx, cid, rec)
        ctx.close()
        del sc


# ------------------------------------------------------------------------------------------------------------------------ 2^26

def _fill(name, cid, out, seed, parts=4):
    """generator `name` into `out` in `parts` slices (bounded temporaries at 2^26)"""
    m = len(out) // parts
    for i in range(parts):
        out[i * m:(i + 1) * m] = sk.make_scalars(name, cid, m, seed + i)


def test_bench_workload_skewed_at_2_26(ea, oracle, torch_cuda):
    """BLS12-377 G1 at 2^26 (the benchmark's workload): witness scalars from the device; then two host batches (witness, zeros_90), whose
    first is handed over in the growing pieces of a host-scalar batch (carried chunks at one forced window size)."""
    torch = torch_cuda
    cid, n, D = 0, 1 << 26, 1 << 12
    tile = sk.random_tile(ea, cid, D, seed=500)
    ctx = ea.MultiScalarMultContext(sk.NAMES[cid])
    ctx.set_bases(_device_bases(torch, tile, n))
    host = np.empty((2 * n, 32), dtype=np.uint8)
    _fill("witness", cid, host[:n], 11)
    _fill("zeros_90", cid, host[n:], 21)
    exp = [sk.fold_reference(oracle, cid, tile, host[:n]), sk.fold_reference(oracle, cid, tile, host[n:])]
    prefix = n // 32   # smaller than any piece of a batch: its hot bucket is a lower bound for the first piece's
    dev = torch.from_numpy(host[:n]).cuda()
    assert ctx.run(dev)[0] == exp[0], "device scalars"
    del dev
    rec = _plan(ctx, "bls12_377_g1 2^26 witness device", n, host[:n], prefix=prefix)
    _assert_hot(rec)
    _assert_te(ctx, cid, rec)
    got = ctx.run(host)
    assert got == exp, "two host batches"
    rec = _plan(ctx, "bls12_377_g1 2^26 host batches witness + zeros_90", n)
    assert rec["chunks"] >= 3, (rec, "the first host batch should arrive in pieces")
    for lo, gen in ((0, "witness"), (n, "zeros_90")):
        r2 = _plan(ctx, f"bls12_377_g1 2^26 host batch {gen} (model)", n, host[lo:lo + prefix])
        if rec["anchored_window"] or gen == "witness":   # zeros_90 has a hot bucket only where zeros have an entry (the anchored window)
            _assert_hot(r2)
    _assert_te(ctx, cid, rec)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------ G2

@pytest.mark.parametrize("cid", [2, 3])
def test_g2_skewed_at_2_20(ea, oracle, torch_cuda, cid):
    torch = torch_cuda
    n = 1 << 20
    name = sk.NAMES[cid]
    cases = (("same_base", sk.same_base_tile(ea, cid, 12), sk.make_scalars("all_equal", cid, n, 12)),
             ("cancel", sk.cancel_tile(ea, cid, 13), sk.make_scalars("all_equal", cid, n, 13)),
             ("witness", sk.random_tile(ea, cid, 1 << 10, seed=600 + cid), sk.make_scalars("witness", cid, n, 14)))
    for label, tile, sc in cases:
        exp = sk.fold_reference(oracle, cid, tile, sc)
        b = _device_bases(torch, tile, n)
        default = None
        for paired in (None, 0):
            ctx = ea.MultiScalarMultContext(name)
            if paired is not None:
                ctx.set_option("g2_paired", paired)
            ctx.set_bases(b)
            got = _run_dev(torch, ctx, sc)[0]
            assert got == exp, (label, paired)
            rec = _plan(ctx, f"{name} 2^20 {label} g2_paired={'default' if paired is None else paired}", n, sc)
            _assert_hot(rec)
            default = default or ctx.query("g2_paired")
            ctx.close()
        assert default != 0, "g2_paired = 0 should differ from the default"
