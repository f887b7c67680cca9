"""GPU: MSMs at size on ALL-DISTINCT bases, byte-equal to a discrete-log oracle (tests/distinct_cases.py).

bases[i] = h_i * G for known h_i, made on the device by the fixed-base entry, so sum_i s_i * bases[i] = ((sum_i s_i h_i) mod r) * G: an
integer dot product on the CPU and one multiplication by the CPU oracle.  Every other at-size test repeats a tile of D = 2^12..2^15
points, and its reference cannot tell base i from base i + D; here every entry has a base of its own, so a tile, chunk, shard or batch
offset that is wrong by ANY amount, a packed index that loses bits and a tail that is dropped all move the expected point.  Nothing is
compared with another GPU run.

Sizes: the smallest at which the at-size machinery is in play -- 2^20 pairs arm the anchored window (Context::anchor_wanted) and are far
above the entry counts at which Context::plan changes its lane and fan-in rules; 2^20 - 3 is just below the anchor rule and off every
power of two; 3 * 2^20 + 1 and 2^22 have a ragged tail and the block-generation fit of Context::plan.  Three cases sit elsewhere than
at 2^20, because the branch they are about starts elsewhere:
  * "precompute = auto" builds no tables for BLS12-381 G1 from 3 * 2^18 pairs on (precompute_auto_levels): that curve's automatic tables
    are tested at 3 * 2^18 - 1, the largest size of the 6-level branch there;
  * a host-scalar batch is split into pieces from 2^23 pairs on (msm_host::first_batch_pieces): host scalars run at 2^20 and
    3 * 2^20 + 1 (one piece) and at 2^23 + 1 (the split first piece), which is why the G1 bases are 2^23 + 1 long;
  * the stateless call cuts its operands into slices of at least 2^20 pairs and only above 1.5 slices (msm_host::stateless_slices): it
    runs at 3 * 2^20 + 1, in five slices."""
import numpy as np
import pytest

import distinct_cases as dc
import pymodel as pm

pytestmark = pytest.mark.gpu

G1 = ("bls12_377_g1", "bls12_381_g1")
G2 = ("bls12_377_g2", "bls12_381_g2")
ALL = G1 + G2
M = 1 << 20
SIZES = {name: (M - 3, M, 3 * M + 1, 4 * M) for name in G1}
SIZES.update({name: ((1 << 18) + 5, M) for name in G2})
SPLIT = 8 * M + 1          # host scalars in pieces
N_MAX = {name: SPLIT if name in G1 else M for name in ALL}
LOG_SEED = 0xD15C


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


class World:
    """One curve: the logs and the device bases at the largest size (smaller cases use a prefix), and the expectations already computed."""

    def __init__(self, ea, oracle, name):
        self.ea, self.oracle, self.name = ea, oracle, name
        self.curve = pm.CURVES[name]
        self.cid = self.curve.curve_id
        self.n_max = N_MAX[name]
        self.logs, self.planted = dc.make_logs(self.cid, self.n_max, LOG_SEED)
        self.bases = dc.device_bases(ea, name, self.logs)
        self.memo = {}

    def pair(self, n, kind="uniform", seed=1):
        """(scalars (n, 4) uint64, the expected image of their MSM over the first n bases)"""
        s = dc.make_scalars(self.cid, n, seed, kind)
        key = (n, kind, seed)
        if key not in self.memo:
            self.memo[key] = dc.expected(self.oracle, self.curve, self.logs[:n], s)
        return s, self.memo[key]

    def planted_flat(self):
        return sorted(x for v in self.planted.values() for x in (v if isinstance(v, tuple) else (v,)))


def _world_fixture(name):
    @pytest.fixture(scope="module", name="world_" + name)
    def fixture(ea, oracle, torch_cuda):
        w = World(ea, oracle, name)
        yield w
        w.bases = None
        torch_cuda.cuda.empty_cache()
    return fixture


world_bls12_377_g1 = _world_fixture("bls12_377_g1")
world_bls12_381_g1 = _world_fixture("bls12_381_g1")
world_bls12_377_g2 = _world_fixture("bls12_377_g2")
world_bls12_381_g2 = _world_fixture("bls12_381_g2")


@pytest.fixture
def world(request):
    return lambda name: request.getfixturevalue("world_" + name)


def dev(torch, words):
    return torch.from_numpy(dc.as_bytes(words).reshape(-1)).cuda()


def run(w, scalars, n=None, bases=None, options=(), devices=None, npoints=None, check=None):
    """the images of one run over the first n bases of w (or `bases`), on a fresh context with `options` set before the bases go in"""
    ctx = w.ea.MultiScalarMultContext(w.name, devices=devices)
    try:
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_bases(w.bases[:n] if bases is None else bases)
        out = ctx.run(scalars, npoints=npoints)
        if check:
            check(ctx)
        return out
    finally:
        ctx.close()


# ---- the bases, by something other than the MSM ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_bases_are_what_the_logs_say(world, name):
    """The subgroup check accepts every base and counts the planted infinities; the first 64 images and the planted rows equal the
    Python model's h * G."""
    w = world(name)
    curve = w.curve
    ctx = w.ea.MultiScalarMultContext(name)
    try:
        chk = ctx.check_bases(w.bases)
    finally:
        ctx.close()
    assert chk.ok and not chk.status.any()
    assert chk.counts["flagged_infinity"] == dc.planted_infinities(w.planted) == 2
    rows = sorted(set(range(64)) | set(w.planted_flat()))
    got = w.bases[rows].cpu().numpy()
    g = curve.generator()
    for t, i in enumerate(rows):
        assert got[t].tobytes() == curve.encode_affine(curve.mul(dc.row_int(w.logs[i]), g)), (name, i)
    flag = 2 * curve.coord_bytes
    assert got[rows.index(w.planted["zero"]), flag] == 1 and got[rows.index(w.planted["r"]), flag] == 1
    for label, where in w.planted.items():
        if label.startswith("equal"):
            assert got[rows.index(where[0])].tobytes() == got[rows.index(where[1])].tobytes(), label
        elif label.startswith("opposite"):                                   # same x, another y
            a, b = got[rows.index(where[0])], got[rows.index(where[1])]
            assert a[:flag // 2].tobytes() == b[:flag // 2].tobytes() and a[flag // 2:flag].tobytes() != b[flag // 2:flag].tobytes(), label


# ---- the default plan --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n", [(name, n) for name in ALL for n in SIZES[name]])
def test_default_plan(world, torch_cuda, name, n):
    w = world(name)
    s, want = w.pair(n)

    def check(ctx):
        t = ctx.last_timings()
        assert t["launches"] == 1 and not t["tables"]
        assert t["twisted_edwards"] == (name == "bls12_377_g1")

    assert run(w, dev(torch_cuda, s), n, check=check)[0] == want, (name, n)


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("kind", ["any256", "hot"])
def test_default_plan_full_width_and_hot_scalars(world, torch_cuda, name, kind):
    w = world(name)
    s, want = w.pair(M, kind)
    assert run(w, dev(torch_cuda, s), M)[0] == want, (name, kind)


@pytest.mark.parametrize("name,n", [(name, n) for name in G1 for n in (M, 3 * M + 1, SPLIT)])
def test_host_scalars(world, name, n):
    """NumPy scalars.  From 2^23 pairs on the first piece of the batch is computed while the rest crosses PCIe, as chunks of one carried
    batch: 1/13 + 3/13 + 9/13 of it (BLS12-377 G1, whose pieces cost no merge: 1/26 + 3/26 + 9/26 + the rest)."""
    w = world(name)
    s, want = w.pair(n)

    def check(ctx):
        assert ctx.last_timings()["launches"] == (1 if n < SPLIT else 4 if name == "bls12_377_g1" else 3)

    assert run(w, dc.as_bytes(s), n, check=check)[0] == want, (name, n)


# ---- chunks, batches, tables, kernel families, shards, prefixes --------------------------------------------------------------

@pytest.mark.parametrize("name,carry", [(name, 1) for name in ALL] + [("bls12_377_g1", 0)])
def test_chunks_at_three_base_offsets(world, torch_cuda, name, carry):
    w = world(name)
    s, want = w.pair(M)

    def check(ctx):
        assert ctx.last_timings()["launches"] == 3

    assert run(w, dev(torch_cuda, s), M, options=(("max_chunk", M // 3 + 1), ("carry", carry)), check=check)[0] == want, (name, carry)


@pytest.mark.parametrize("name", G1)
def test_two_batches_in_one_run(world, torch_cuda, name):
    w = world(name)
    s0, want0 = w.pair(M)
    s1, want1 = w.pair(M, seed=2)
    assert want0 != want1
    both = dev(torch_cuda, np.concatenate([s0, s1]))
    assert run(w, both, M) == [want0, want1], name


TABLE_CASES = ([(name, "all", M) for name in ALL]
               + [(name, "auto", 3 * (1 << 18) - 1 if name == "bls12_381_g1" else M) for name in ALL]
               + [("bls12_377_g1", "three", M)])


@pytest.mark.parametrize("name,mode,n", TABLE_CASES)
def test_precomputed_tables(world, torch_cuda, name, mode, n):
    """"all": precompute = 1, a level per window.  "auto": precompute = 2, the 6-level branch of precompute_auto_levels (BLS12-381 G1:
    at 3 * 2^18 - 1 pairs, the last size at which that curve gets tables).  "three": table_levels = 3."""
    w = world(name)
    s, want = w.pair(n)
    options = {"all": (("precompute", 1),), "auto": (("precompute", 2),), "three": (("precompute", 1), ("table_levels", 3))}[mode]

    def check(ctx):
        levels = ctx.query("table_levels")
        assert ctx.last_timings()["tables"] and levels > 1, (name, mode, levels)
        if mode == "all":
            assert levels > 6
        else:
            assert levels <= (6 if mode == "auto" else 3), (name, mode, levels)

    assert run(w, dev(torch_cuda, s), n, options=options, check=check)[0] == want, (name, mode)


@pytest.mark.parametrize("name,option", [("bls12_377_g1", "twisted_edwards")] + [(name, "g2_paired") for name in G2])
def test_the_other_kernel_family(world, torch_cuda, name, option):
    """BLS12-377 G1 on the XYZZ kernels instead of the twisted-Edwards ones; G2 with one lane per point instead of two"""
    w = world(name)
    s, want = w.pair(M)

    def check(ctx):
        assert not ctx.last_timings()["twisted_edwards"] and ctx.query(option) == 0

    assert run(w, dev(torch_cuda, s), M, options=((option, 0),), check=check)[0] == want, (name, option)


def test_logical_shards_with_a_ragged_last_shard(world, torch_cuda):
    w = world("bls12_377_g1")
    n = M - 3
    assert n % 3
    s, want = w.pair(n)

    def check(ctx):
        assert ctx.query("shards") == 3 and ctx.query("bases") == n

    assert run(w, dev(torch_cuda, s), n, devices=[0] * 3, check=check)[0] == want
    assert run(w, dc.as_bytes(s), n, devices=[0] * 3)[0] == want


@pytest.mark.parametrize("name", G1)
def test_prefix_run(world, torch_cuda, name):
    """npoints below the number of resident bases: the 2^22 bases stay, the run reads n - 4097 of them"""
    w = world(name)
    n = 4 * M - 4097
    s, want = w.pair(n)
    assert run(w, dev(torch_cuda, s), 4 * M, npoints=n)[0] == want, name


def test_stateless_call_with_host_bases(world):
    """ea.msm with both operands in host memory: the pipelined upload slices the bases (five slices at 3 * 2^20 + 1 pairs)"""
    w = world("bls12_377_g1")
    n = 3 * M + 1
    s, want = w.pair(n)
    bases = w.bases[:n].cpu().numpy()
    assert w.ea.msm(bases, dc.as_bytes(s), w.name) == want
    st = w.ea.last_stateless()
    assert st["slices"] > 1 and st["bytes"] == n * (w.curve.affine_stride + 32)


# ---- positive control -----------------------------------------------------------------------------------------------------------

def test_a_base_exchanged_at_a_multiple_of_the_tile_is_seen(world, torch_cuda):
    """Bases i and i + 2^15 exchanged -- the error no tiled reference sees: the result differs from the expectation of the true logs and
    equals the expectation of the logs exchanged the same way."""
    w = world("bls12_377_g1")
    s, want = w.pair(M)
    i, j = 123457, 123457 + (1 << 15)
    assert dc.row_int(s[i]) != dc.row_int(s[j]) and dc.row_int(w.logs[i]) != dc.row_int(w.logs[j])
    assert not {i, j} & set(w.planted_flat())
    bases = w.bases[:M].clone()
    bases[i], bases[j] = w.bases[j], w.bases[i]
    logs = w.logs[:M].copy()
    logs[[i, j]] = logs[[j, i]]
    got = run(w, dev(torch_cuda, s), bases=bases)[0]
    assert got != want
    assert got == dc.expected(w.oracle, w.curve, logs, s)
