"""GPU: the wide anchored window (option "anchor_wide") on every path of the bucket reduction and on every repeat path.

The reduction of a wide window differs from the plain one in each branch of reduce_buckets (csrc/msm_engine.hip): the direct scan copies
R -- the plain sum of the upper bucket set -- out of the scanned row, one chunked level writes it as one more row of chunk sums (with full
rows, or with rows padded to a power of two under a re-cut first level with a partial last chunk), and the recursive levels carry that row to
the end.  query("reduce_path") says which branch a run took (0 recursive, 1 direct scan, 2 chunked level + scan on full rows, 3 the same on
padded rows), "reduce_chunks" and "reduce_row" its geometry; every case below asserts the path it was written for.

Every result is the oracle's bytes on the scalars reduced mod r (the bases are in the prime-order subgroup unless a test says otherwise), and
every clean run's query("sorted_entries") is the number of non-zero digits of the host model (tests/anchor_wide_cases.py).  A scalar with a
bit from 253 on makes the engine repeat the chunk or the carried batch without the option ("anchor_wide_fallbacks"); two repeats in a row
switch it off ("anchor_wide_demotions")."""
import random

import numpy as np
import pytest

import anchor_wide_cases as m

pytestmark = pytest.mark.gpu

NAMES = {0: "bls12_377_g1", 2: "bls12_377_g2"}
STRIDE = {0: 104, 2: 200}
SIZE = {0: 4099, 2: 2051}      # ragged on purpose
INF_AT = 77                    # this base is the point at infinity: no entry, and not in the sum of the bases
KINDS = {"g1_te": (0, 1), "g1_xyzz": (0, 0), "g2": (2, 0)}      # context kind -> curve id, option "twisted_edwards"
QUAD_DEFAULT = 1 << 18
# the reduction's options, as a fresh context has them
DEFAULTS = {"reduce_scan": -1, "reduce_log_chunk0": 0, "reduce_log_chunk": 0, "reduce_scan_log": 0, "reduce_fill": 0, "quad_limit": QUAD_DEFAULT,
            "g2_paired": 31, "max_chunk": 0, "first_piece_div": 0, "scalars_montgomery": 0}


def _to_np(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(len(vals), 32).copy()


def _oracle(oracle, cid, bases, vals):
    """the oracle's bytes for the scalars reduced mod r"""
    out = np.zeros(288 if cid >= 2 else 144, dtype=np.uint8)
    bases, sc = np.ascontiguousarray(bases), _to_np([v % m.R377 for v in vals])
    assert oracle.oracle_msm(cid, bases.ctypes.data, STRIDE[cid], sc.ctypes.data, len(vals), out.ctypes.data, 0) == 0
    return out.tobytes()


class Case:
    """one context of a kind, its bases, and the scalar lists with the oracle's bytes and the model's entry counts for them (made once)"""

    def __init__(self, ea, oracle, kind):
        self.kind, (self.cid, self.te) = kind, KINDS[kind]
        self.n = SIZE[self.cid]
        self.oracle = oracle
        self.bases = ea.generate_points(self.n, distinct=257, seed=410 + self.cid, curve=NAMES[self.cid])
        self.bases[INF_AT, -8] = 1
        self.ctx = ea.MultiScalarMultContext(NAMES[self.cid])
        if self.cid == 0:
            self.ctx.set_option("twisted_edwards", self.te)
        self.ctx.set_option("anchor", 2)        # the anchored window at any size and window size
        self.ctx.set_bases(self.bases)
        assert self.cid != 0 or self.ctx.query("twisted_edwards") == self.te
        self._vals, self._exp, self._np, self._entries = {}, {}, {}, {}

    def vals(self, name, c):
        """name -> list of n integers: "edges", "uniform", "bad@<index>" (uniform with one scalar that has bit 253 set), or an all-equal list"""
        key = (name, c if name == "edges" or name in m.equal_values(c) else 0)
        if key not in self._vals:
            if name == "edges":
                v = m.planted_edges(c, self.n, 100 + c)
            elif name == "uniform":
                v = m.uniform_scalars(self.n, 7)
            elif name.startswith("bad@"):
                v = m.uniform_scalars(self.n, 7)
                v[int(name[4:])] = m.bad_scalar(int(name[4:]))
            elif name == "top@":        # 2^253 - 1 does NOT have the bit: at the first and last index and on the base at infinity
                v = m.uniform_scalars(self.n, 7)
                v[0] = v[self.n - 1] = v[INF_AT] = (1 << 253) - 1
            else:
                v = [m.equal_values(c)[name]] * self.n
            self._vals[key] = v
            self._np[key] = _to_np(v)
            self._exp[key] = _oracle(self.oracle, self.cid, self.bases, v)
        return key

    def entries(self, key, c, wide):
        k = (key, c, wide)
        if k not in self._entries:
            self._entries[k] = m.entry_count(self._vals[key], c, wide, skip=(INF_AT,))
        return self._entries[k]

    def set(self, c, wide, **opts):
        for k, v in {**DEFAULTS, **opts}.items():
            if k != "g2_paired" or self.cid == 2:
                self.ctx.set_option(k, v)
        self.ctx.set_option("window_bits", c)
        self.ctx.set_option("anchor_wide", wide)      # (also re-arms a context an earlier case has switched off, and ends its streak)

    def run(self, name, c, device=False):
        """run the list, compare with the oracle; returns its key"""
        key = self.vals(name, c)
        sc = self._np[key]
        if device:
            import torch

            sc = torch.from_numpy(sc).cuda()
        assert self.ctx.run(sc)[0] == self._exp[key], (self.kind, name, c)
        return key

    def counters(self):
        q = self.ctx.query
        return q("anchor_wide_fallbacks"), q("anchor_wide_demotions")


@pytest.fixture(scope="module")
def cases(ea, oracle):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Case(ea, oracle, kind)
        return made[kind]

    yield get
    for cs in made.values():
        cs.ctx.close()


# ---- a. every reduction path ---------------------------------------------------------------------------------------------------------
# (c, options, reduce_path, (reduce_chunks, reduce_row) or None, also run the all-equal lists, kinds)
# The geometry is Plan's (csrc/msm_engine.hip), worked out by hand: half = 2^(c-1) buckets per set, first-level chunks of L0, T0 = ceil(half / L0).
ALL = ("g1_te", "g1_xyzz", "g2")
G1 = ("g1_te", "g1_xyzz")
ROWS = [
    (6, {}, 1, None, False, ALL),
    (7, {}, 1, None, False, ALL),
    (9, {}, 1, None, False, ALL),
    (12, {}, 1, None, True, ALL),
    (14, {}, 2, (2048, 2048), True, ALL),                  # L0 = 4
    (18, {}, 3, (4229, 8192), True, ALL),                  # re-cut: L0 = 31, the last chunk holds 4 buckets
    (21, {}, 3, (5018, 8192), True, ALL),                  # re-cut: L0 = 209
    # recursive chunked levels only
    (7, {"reduce_scan": 0}, 0, (16, 16), False, ALL),                   # 16, 4, 1
    (14, {"reduce_scan": 0}, 0, (2048, 2048), False, ALL),              # 2048, 512, ..., 2, 1: the last level has a short row
    (18, {"reduce_scan": 0}, 0, (32768, 32768), True, ALL),
    (21, {"reduce_scan": 0}, 0, (32768, 32768), False, ALL),            # L0 = 32
    (6, {"reduce_scan": 0, "reduce_log_chunk0": 5}, 0, (1, 1), True, ALL),      # one chunk per set: no later level runs
    (14, {"reduce_scan": 0, "reduce_log_chunk": 3}, 0, (1024, 1024), False, ALL),   # 1024, 128, 16, 2, 1
    # one chunked level, then a scan on rows of 64
    (9, {"reduce_scan_log": 6}, 2, (64, 64), False, ALL),
    (12, {"reduce_scan_log": 6}, 2, (64, 64), False, ALL),
    (14, {"reduce_scan_log": 14}, 1, None, False, ALL),                 # a direct scan on 8192 buckets
    # two waves per SIMD: L0 = 16 divides the set (full rows of 8192) at c = 18; L0 = 105 and rows of 16384 at c = 21
    (18, {"reduce_fill": 2}, 2, (8192, 8192), False, ALL),
    (21, {"reduce_fill": 2}, 3, (9987, 16384), False, ALL),
    (18, {"reduce_log_chunk0": 7}, 2, (1024, 1024), False, ALL),        # a power-of-two L
    (21, {"reduce_log_chunk0": 7}, 2, (4096, 4096), False, ALL),        # (raised to 2^8: the scan takes 4096 elements)
    # the scan steps in both lane forms: all of them one lane per addition, and split (tree steps of <= 1500 additions run four lanes)
    (12, {"quad_limit": 0}, 1, None, False, G1),
    (12, {"quad_limit": 1500}, 1, None, False, G1),
    (18, {"quad_limit": 0}, 3, (4229, 8192), False, G1),
    (18, {"quad_limit": 1500}, 3, (4229, 8192), False, G1),
    # G2: every kernel one lane per point, and (spelled out) two lanes per point
    (12, {"g2_paired": 0}, 1, None, False, ("g2",)),
    (18, {"g2_paired": 0}, 3, (4229, 8192), False, ("g2",)),
    (12, {"g2_paired": 31}, 1, None, False, ("g2",)),
    (18, {"g2_paired": 31}, 3, (4229, 8192), False, ("g2",)),
]
PATH_PARAMS = [pytest.param(kind, c, opts, path, geom, equal, id="-".join([kind, f"c{c}"] + [f"{k}={v}" for k, v in opts.items()]))
               for c, opts, path, geom, equal, kinds in ROWS for kind in kinds]


def test_every_path_has_a_case_on_every_kind():
    for kind in KINDS:
        assert {path for c, opts, path, geom, equal, kinds in ROWS if kind in kinds} == {0, 1, 2, 3}
        assert {path for c, opts, path, geom, equal, kinds in ROWS if kind in kinds and equal} == {0, 1, 2, 3}


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("kind,c,opts,path,geom,equal", PATH_PARAMS)
def test_reduction_paths(cases, kind, c, opts, path, geom, equal, wide):
    cs = cases(kind)
    q = cs.ctx.query
    cs.set(c, wide, **opts)
    before = cs.counters()
    try:
        for name in ["edges"] + (list(m.equal_values(c)) if equal else []):
            key = cs.run(name, c)
            got = (q("reduce_path"), q("reduce_chunks"), q("reduce_row"))
            print(f"{kind} c={c} {opts} wide={wide} {name}: reduce_path={got[0]} reduce_chunks={got[1]} reduce_row={got[2]} bucket_windows={q('bucket_windows')}")
            assert got[0] == path, (kind, c, opts, name, got)
            if geom:
                assert got[1:] == geom, (kind, c, opts, name, got)
            assert q("anchor_wide_active") == wide and q("anchored_window") == 253 // c
            t = cs.ctx.last_timings()
            assert t["window_bits"] == c and t["windows"] == m.windows_of(c) and t["twisted_edwards"] == bool(cs.te)
            assert q("sorted_entries") == cs.entries(key, c, bool(wide)), (kind, c, opts, name)
        assert cs.counters() == before
    finally:
        cs.set(12, 1)


# ---- b. repeats --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [12, 18])
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_bad_scalar_wherever_it_lies(cases, kind, c):
    """bit 253 at the first index, at the last index of the ragged size, on the base at infinity (the level-1 histogram looks at the scalar
    alone), and in the last chunk of a carried batch: the oracle's bytes, one repeat, no demotion"""
    cs = cases(kind)
    q = cs.ctx.query
    try:
        for at, chunk in ((0, 0), (cs.n - 1, 0), (INF_AT, 0), (cs.n - 1, 1025), (1030, 1025)):
            cs.set(c, 1, max_chunk=chunk)
            f0, d0 = cs.counters()
            key = cs.run(f"bad@{at}", c)
            assert cs.counters() == (f0 + 1, d0), (kind, c, at, chunk)
            assert q("anchor_wide_active") == 0 and q("anchor_wide") == 1 and q("anchored_window") == 253 // c
            if chunk:
                assert cs.ctx.last_timings()["launches"] >= -(-cs.n // chunk)
            else:
                assert q("sorted_entries") == cs.entries(key, c, False)       # the repeat grouped round 6's digits
            # the next clean run is wide again
            key = cs.run("uniform", c)
            assert q("anchor_wide_active") == 1 and cs.counters() == (f0 + 1, d0)
            if not chunk:
                assert q("sorted_entries") == cs.entries(key, c, True)
        # 2^253 - 1 has no bit from 253 on
        cs.set(c, 1)
        f0, d0 = cs.counters()
        key = cs.run("top@", c)
        assert cs.counters() == (f0, d0) and q("anchor_wide_active") == 1 and q("sorted_entries") == cs.entries(key, c, True)
    finally:
        cs.set(12, 1)


@pytest.mark.parametrize("chunk", [0, 1025])
@pytest.mark.parametrize("c", [12, 18])
@pytest.mark.parametrize("kind", list(KINDS))
def test_two_batches_in_one_call(cases, kind, c, chunk):
    """One of two batches falls back: its base-sum term is 2^(c a + c - 1) S, the other's 2^(c a + c) S (both kept by anchor_term).  Both fall
    back: two repeats in a row, the context stops using the option."""
    cs = cases(kind)
    q = cs.ctx.query
    clean, bad, bad2 = cs.vals("edges", c), cs.vals("bad@2000", c), cs.vals(f"bad@{cs.n - 1}", c)
    try:
        for order in ((clean, bad), (bad, clean)):
            cs.set(c, 1, max_chunk=chunk)
            f0, d0 = cs.counters()
            got = cs.ctx.run(np.concatenate([cs._np[k] for k in order]))
            assert got == [cs._exp[k] for k in order], (kind, c, chunk, order)
            assert cs.counters() == (f0 + 1, d0) and q("anchor_wide") == 1
            assert q("anchor_wide_active") == (1 if order[1] is clean else 0)
            cs.run("uniform", c)
            assert q("anchor_wide_active") == 1 and cs.counters() == (f0 + 1, d0)
        cs.set(c, 1, max_chunk=chunk)
        f0, d0 = cs.counters()
        got = cs.ctx.run(np.concatenate([cs._np[bad], cs._np[bad2]]))
        assert got == [cs._exp[bad], cs._exp[bad2]], (kind, c, chunk)
        assert cs.counters() == (f0 + 2, d0 + 1) and q("anchor_wide") == 0 and q("anchor_wide_active") == 0
        cs.run("uniform", c)                   # switched off: round 6's digits, nothing to repeat
        assert q("anchor_wide_active") == 0 and cs.counters() == (f0 + 2, d0 + 1)
        cs.run(f"bad@{cs.n - 1}", c)
        assert cs.counters() == (f0 + 2, d0 + 1)
    finally:
        cs.set(12, 1)
    assert q("anchor_wide") == 1


@pytest.mark.parametrize("c", [12, 18])
@pytest.mark.parametrize("kind", list(KINDS))
def test_device_scalars_and_first_piece(cases, kind, c):
    cs = cases(kind)
    q = cs.ctx.query
    try:
        cs.set(c, 1)
        f0, d0 = cs.counters()
        key = cs.run("edges", c, device=True)
        assert q("anchor_wide_active") == 1 and q("sorted_entries") == cs.entries(key, c, True) and cs.counters() == (f0, d0)
        cs.run("bad@2000", c, device=True)
        assert q("anchor_wide_active") == 0 and cs.counters() == (f0 + 1, d0)
        # host scalars of a carried batch arrive in pieces (1/13, 3/13, 9/13): wide on; a bad scalar in the first piece and in the last
        cs.set(c, 1, max_chunk=1025, first_piece_div=13)
        cs.run("edges", c)
        assert q("anchor_wide_active") == 1 and cs.counters() == (f0 + 1, d0)
        assert cs.ctx.last_timings()["launches"] >= -(-cs.n // 1025)
        cs.run("bad@0", c)
        assert q("anchor_wide_active") == 0 and cs.counters() == (f0 + 2, d0)
        cs.run("edges", c)
        assert q("anchor_wide_active") == 1
        cs.run(f"bad@{cs.n - 1}", c)
        assert q("anchor_wide_active") == 0 and cs.counters() == (f0 + 3, d0) and q("anchor_wide") == 1
    finally:
        cs.set(12, 1)


@pytest.mark.parametrize("c", [12, 18])
def test_montgomery_scalars_never_flag(cases, c):
    """"scalars_montgomery": the digits are read from the converted, canonical value -- also where the IMAGE handed over has bit 253 set"""
    cs = cases("g1_te")
    q = cs.ctx.query
    vals = [v % m.R377 for v in m.planted_edges(c, cs.n, 300 + c)]
    img = m.montgomery_images(vals)
    assert sum(1 for v in img if v >> 253) >= cs.n // 2
    exp = _oracle(cs.oracle, 0, cs.bases, vals)
    try:
        cs.set(c, 1, scalars_montgomery=1)
        before = cs.counters()
        assert cs.ctx.run(_to_np(img))[0] == exp
        assert q("anchor_wide_active") == 1 and cs.counters() == before
        assert q("sorted_entries") == m.entry_count(vals, c, True, skip=(INF_AT,))
    finally:
        cs.set(12, 1)


@pytest.mark.parametrize("levels", [0, 3])
@pytest.mark.parametrize("c", [12, 18])
def test_precomputed_tables_exclude_the_wide_window(ea, oracle, c, levels):
    n = SIZE[0]
    bases = ea.generate_points(n, distinct=257, seed=77)
    bases[INF_AT, -8] = 1
    clean, bad = m.planted_edges(c, n, 5), m.uniform_scalars(n, 6)
    bad[n - 1] = m.bad_scalar(1)
    ctx = ea.MultiScalarMultContext("bls12_377_g1")
    ctx.set_option("window_bits", c)
    ctx.set_option("precompute", 1)
    ctx.set_option("table_levels", levels)
    ctx.set_option("anchor", 2)
    ctx.set_bases(bases)
    try:
        assert ctx.query("anchor_wide") == 1
        for vals in (clean, bad):
            assert ctx.run(_to_np(vals))[0] == _oracle(oracle, 0, bases, vals), (c, levels)
            t = ctx.last_timings()
            assert t["tables"] and t["window_bits"] == c
            assert ctx.query("anchor_wide_active") == 0 and ctx.query("anchor_wide_fallbacks") == 0 and ctx.query("anchored_window") == 253 // c
    finally:
        ctx.close()


@pytest.mark.parametrize("c", [12, 18])
def test_sharded_context(ea, oracle, c):
    """Three logical shards.  query() adds counters and "sorted_entries" up over the shards and reports the largest "anchor_wide_active" and
    reduction geometry: that EVERY shard ran wide shows in the entry count (a wide window has fewer non-zero digits)."""
    n = SIZE[0]
    bases = ea.generate_points(n, distinct=257, seed=78)
    bases[INF_AT, -8] = 1
    lo, hi = ea.shard_bounds(n, 3, 1)
    assert INF_AT < lo
    clean, bad = m.planted_edges(c, n, 8), m.uniform_scalars(n, 9)
    bad[(lo + hi) // 2] = m.bad_scalar(2)
    ctx = ea.multi_scalar_mult_init(bases, "bls12_377_g1", devices=[0, 0, 0])
    try:
        ctx.set_option("anchor", 2)
        ctx.set_option("window_bits", c)
        q = ctx.query
        assert ctx.run(_to_np(clean))[0] == _oracle(oracle, 0, bases, clean)
        assert q("anchor_wide_active") == 1 and q("anchor_wide_fallbacks") == 0 and q("reduce_path") == (1 if c == 12 else 3)
        wide_entries = m.entry_count(clean, c, True, skip=(INF_AT,))
        assert wide_entries < m.entry_count(clean, c, False, skip=(INF_AT,)) - n // 20
        assert q("sorted_entries") == wide_entries
        # a bad scalar in the middle shard's slice: that shard alone repeats
        assert ctx.run(_to_np(bad))[0] == _oracle(oracle, 0, bases, bad)
        assert q("anchor_wide_fallbacks") == 1 and q("anchor_wide_demotions") == 0 and q("anchor_wide") == 1
        assert q("sorted_entries") == (m.entry_count(bad[:lo], c, True, skip=(INF_AT,)) + m.entry_count(bad[lo:hi], c, False) +
                                       m.entry_count(bad[hi:], c, True))
        assert ctx.run(_to_np(clean))[0] == _oracle(oracle, 0, bases, clean) and q("sorted_entries") == wide_entries
    finally:
        ctx.close()


# ---- the wide repeat together with the twisted-Edwards repeat ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def outside_subgroup(oracle):
    """Bases of order 2 r among bases of order r (tests/test_gpu_anchor.py), two of them a pair whose sum the twisted-Edwards law cannot
    compute (tests/test_gpu_robust.py); the pair shares a scalar and so a bucket, one scalar on a base of order r has bit 253 set."""
    import pymodel as pm
    import te_model as te

    C = pm.BLS12_377_G1
    def failing_pair():
        for P in pm.random_points(C, 8, random.Random(9)):
            for E in te.exceptional_points():
                R = C.add(P, E)
                a, b = te.sw_to_te(R), te.sw_to_te(P)
                if a is None or b is None:
                    continue
                if te.te_add(a, b) is None:
                    return R, P
                if te.te_add(a, te.te_neg(b)) is None:
                    return R, C.neg(P)
        raise AssertionError("no failing pair found")

    pair = failing_pair()
    rng = random.Random(3)
    n = 3000
    T = (C.p - 1, 0)
    pts = [C.add(P, T) for P in pm.random_points(C, 30, rng)] + pm.random_points(C, 30, rng)
    seq = [pts[i % 60] for i in range(n)]
    seq[100], seq[2000] = pair
    bases = np.frombuffer(C.encode_affine_array(seq), dtype=np.uint8).reshape(n, 104).copy()
    vals = [0] * n
    vals[100] = vals[2000] = random.Random(5).randrange(1, m.R377)
    bad_at = 2985                                   # 2985 % 60 = 45: a base of order r, on which k P = (k mod r) P
    assert bad_at % 60 >= 30
    vals[bad_at] = m.bad_scalar(3)
    return bases, vals, _oracle(oracle, 0, bases, vals)


@pytest.mark.parametrize("chunk", [0, 1500])
@pytest.mark.parametrize("c", [12, 18])
def test_wide_repeat_together_with_the_edwards_repeat(ea, outside_subgroup, c, chunk):
    """The run with the wide window is void (a scalar has bit 253 set) AND the Edwards law fails on the repeat: a lone chunk and a carried
    batch both end on the XYZZ path without the wide window, with one fallback of each kind; a second such run demotes the context twice."""
    bases, vals, exp = outside_subgroup
    ctx = ea.MultiScalarMultContext("bls12_377_g1")
    ctx.set_option("anchor", 2)
    ctx.set_option("window_bits", c)
    ctx.set_option("max_chunk", chunk)
    ctx.set_bases(bases)
    q = ctx.query
    try:
        assert q("twisted_edwards") == 1 and q("anchor_wide") == 1
        sc = _to_np(vals)
        assert ctx.run(sc)[0] == exp, (c, chunk)
        assert (q("anchor_wide_fallbacks"), q("twisted_edwards_fallbacks")) == (1, 1)
        assert (q("anchor_wide_demotions"), q("twisted_edwards_demotions")) == (0, 0)
        assert q("anchor_wide_active") == 0 and ctx.last_timings()["twisted_edwards"] is False
        assert ctx.run(sc)[0] == exp, (c, chunk)
        assert (q("anchor_wide_fallbacks"), q("twisted_edwards_fallbacks")) == (2, 2)
        assert (q("anchor_wide_demotions"), q("twisted_edwards_demotions")) == (1, 1)
        assert q("anchor_wide") == 0 and q("twisted_edwards") == 0
        assert ctx.run(sc)[0] == exp, (c, chunk)
        assert (q("anchor_wide_fallbacks"), q("twisted_edwards_fallbacks")) == (2, 2)
    finally:
        ctx.close()
