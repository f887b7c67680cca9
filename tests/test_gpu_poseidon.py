"""GPU: Poseidon sponges and Merkle trees over Fr (csrc/poseidon.hpp, csrc/msm_poseidon.hpp) through the Python layer, element for
element against Python big integers (tests/poseidon_cases.py, which reproduces snarkVM's recorded results): the 100 recorded
transcripts, every shape at which a sponge takes another path at batch sizes around a wave and a block, rates 2, 4 and 8 on both fields,
other parameters, hash_many, Merkle trees with every node, root(depth) and path(i); the dense form of the partial rounds, host against
device pointers, out=, the refusal of an overlap; and the stream order of flag bit 1, pinned with late producers as
tests/test_gpu_mle.py pins it."""
import random

import numpy as np
import pytest

import poseidon_cases as pc
import stream_cases as st

pytestmark = pytest.mark.gpu

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
DOMAIN = "AleoPoseidon2"


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def hashers(ea):
    """one domain per field and one handle per (field, rate, parameter set) for the whole module: (handle, model)"""
    doms, made = {}, {}

    def get(field, rate, alt=False):
        if field not in doms:
            doms[field] = ea.Radix2EvaluationDomain(16, CURVE_OF[field])
        key = (field, rate, alt)
        if key not in made:
            kw = dict(pc.ALT_381) if alt else dict(pc.SNARKVM)
            m = pc.Model.generated(field, rate, **kw)
            if field == "bls12_377" and not alt:
                h = ea.Poseidon(doms[field], rate, domain=DOMAIN)                     # snarkVM's defaults, from the package's generator
            else:
                h = ea.Poseidon(doms[field], rate, parameters=dict(kw, ark=m.ark, mds=m.mds), domain=DOMAIN)
            made[key] = (h, m)
        h, m = made[key]
        h.set_option("sparse", 1)
        return h, m

    yield get
    for h, _ in made.values():
        h.close()
    for d in doms.values():
        d.close()


def dev(torch, raw, shape):
    return torch.frombuffer(bytearray(raw) if len(raw) else bytearray(1), dtype=torch.uint8)[:len(raw)].cuda().reshape(shape)


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else (t.tobytes() if hasattr(t, "tobytes") else bytes(t))


def rows_of(field, raw, n, width, montgomery):
    v = pc.decode(field, raw, montgomery)
    assert len(v) == n * width
    return [v[i * width:(i + 1) * width] for i in range(n)]


def test_the_recorded_transcripts(hashers, torch_):
    """absorb_a_squeeze_s for a, s < 10 at rate 2 on BLS12-377 with the handle's default parameters: each of the hundred shapes as a
    batch of three equal rows, device pointers"""
    h, m = hashers("bls12_377", 2)
    assert (h.query("rate"), h.query("state"), h.query("rounds")) == (2, 3, 39)
    for absorb in range(10):
        raw = pc.encode("bls12_377", [pc.SPONGE_INPUT] * (3 * absorb), True)
        t = dev(torch_, raw, (3, absorb, 32))
        for squeeze in range(10):
            want = pc.snapshot("test_sponge", "absorb_%d_squeeze_%d.snap" % (absorb, squeeze))
            got = h.sponge(t, squeeze)
            assert tuple(got.shape) == (3, squeeze, 32)
            assert rows_of("bls12_377", raw_of(got), 3, squeeze, True) == [want] * 3, (absorb, squeeze)


@pytest.mark.parametrize("rate", [2, 4, 8])
@pytest.mark.parametrize("field", FIELDS)
def test_every_shape_against_the_model(hashers, torch_, field, rate):
    """in_len in {0, 1, rate - 1, rate, rate + 1, 2 rate + 1} by n_out in {1, rate, rate + 1, 2 rate + 1}, both forms; the model hashes
    three distinct rows per shape, which a batch of n rows repeats: n in {1, 63, 64, 65, 257} and one block and one lane more than a
    block, every row compared; the dense form and host pointers give the same bytes"""
    h, m = hashers(field, rate)
    lanes = h.query("block_lanes")
    sizes = sorted({1, 63, 64, 65, 257, lanes, lanes + 1})
    rng = random.Random(0x6B0 + rate)
    for k, in_len in enumerate(pc.in_lens(rate)):
        for j, n_out in enumerate(pc.out_lens(rate)):
            montgomery = (k + j) % 2 == 0
            base = [[rng.randrange(m.p) for _ in range(in_len)] for _ in range(3)]
            want3 = [m.sponge(r, n_out) for r in base]
            n = sizes[(k * 4 + j) % len(sizes)]
            rows = [base[i % 3] for i in range(n)]
            raw = pc.encode(field, pc.flat(rows), montgomery)
            got = h.sponge(dev(torch_, raw, (n, in_len, 32)), n_out, montgomery=montgomery)
            got_raw = raw_of(got)
            assert rows_of(field, got_raw, n, n_out, montgomery) == [want3[i % 3] for i in range(n)], (in_len, n_out, n)
            if j == k % 4:
                assert raw_of(h.sponge(raw, n_out, in_len=in_len, montgomery=montgomery)) == got_raw            # host pointers
                h.set_option("sparse", 0)
                assert raw_of(h.sponge(dev(torch_, raw, (n, in_len, 32)), n_out, montgomery=montgomery)) == got_raw
                h.set_option("sparse", 1)
    # every batch size at one shape that crosses a rate block on both sides
    in_len, n_out = rate + 1, rate + 1
    base = [[rng.randrange(m.p) for _ in range(in_len)] for _ in range(3)]
    want3 = [m.sponge(r, n_out) for r in base]
    for n in sizes:
        rows = [base[i % 3] for i in range(n)]
        got = h.sponge(dev(torch_, pc.encode(field, pc.flat(rows), True), (n, in_len, 32)), n_out)
        assert rows_of(field, raw_of(got), n, n_out, True) == [want3[i % 3] for i in range(n)], n


@pytest.mark.parametrize("field", FIELDS)
def test_edge_inputs_and_products(hashers, torch_, field):
    """0, r - 1, r and 2^256 - 1 as they are, in both forms and both forms of the rounds; the product counts of the handle"""
    for rate in (2, 8):
        h, m = hashers(field, rate)
        t = rate + 1
        words = pc.edge_words(field)
        rows = [[w] * t for w in words] + [[words[(i + j) % 4] for j in range(t)] for i in range(2)]
        raw = pc.raw_words(pc.flat(rows))
        for montgomery in (True, False):
            meant = rows_of(field, raw, len(rows), t, montgomery)
            want = pc.encode(field, pc.flat([m.sponge(r, t) for r in meant]), montgomery)
            for sparse in (1, 0):
                h.set_option("sparse", sparse)
                assert raw_of(h.sponge(dev(torch_, raw, (len(rows), t, 32)), t, montgomery=montgomery)) == want, (rate, montgomery, sparse)
        h.set_option("sparse", 0)
        dense = h.query("products_per_permutation")
        h.set_option("sparse", 1)
        sparse_ = h.query("products_per_permutation")
        assert dense >= 8 * (5 * t + t * t) + 31 * (5 + t * t) and 8 * (5 * t + t * t) + 31 * (5 + 2 * t - 1) <= sparse_ < dense
        assert h.query("lds_bytes") == 2 * t * 36 * h.query("block_lanes") and h.query("work_bytes") > 0


def test_other_parameters_on_bls12_381(hashers, torch_):
    h, m = hashers("bls12_381", 4, alt=True)
    assert h.query("rounds") == 17
    rng = random.Random(0xA5)
    rows = [[rng.randrange(m.p) for _ in range(9)] for _ in range(67)]
    want = [m.sponge(r, 5) for r in rows[:4]]
    rows = [rows[i % 4] for i in range(67)]
    raw = pc.encode("bls12_381", pc.flat(rows), True)
    for sparse in (1, 0):
        h.set_option("sparse", sparse)
        got = rows_of("bls12_381", raw_of(h.sponge(dev(torch_, raw, (67, 9, 32)), 5)), 67, 5, True)
        assert got == [want[i % 4] for i in range(67)]


@pytest.mark.parametrize("field", FIELDS)
def test_hash_many_and_hash_against_the_preimage_form(hashers, torch_, field):
    h, m = hashers(field, 4)
    dom = pc.domain_element(DOMAIN, m.p)
    assert h.domain == dom
    rng = random.Random(0x4A5)
    for in_len in (0, 1, 4, 7):
        rows = [[rng.randrange(m.p) for _ in range(in_len)] for _ in range(3)]
        for montgomery in (True, False):
            raw = pc.encode(field, pc.flat(rows), montgomery)
            got = h.hash_many(dev(torch_, raw, (3, in_len, 32)), 3, montgomery=montgomery)
            # the preimage [domain, length, 0, 0] || row through the raw sponge of the model
            assert rows_of(field, raw_of(got), 3, 3, montgomery) == [m.sponge([dom, in_len, 0, 0] + r, 3) for r in rows]
            one = h.hash(raw, in_len=in_len, montgomery=montgomery) if in_len else h.hash(np.zeros((3, 0, 32), np.uint8), montgomery=montgomery)
            assert tuple(one.shape) == (3, 32)
            assert pc.decode(field, raw_of(one), montgomery) == [m.hash(dom, r) for r in rows]


@pytest.mark.parametrize("leaf_len", [1, 4])
@pytest.mark.parametrize("field", FIELDS)
def test_merkle_trees_against_the_model(hashers, torch_, field, leaf_len):
    """1, 2, 3, 5, 64, 65 and 1000 leaves: every node, the padding leaves, root(depth) and path(i); host pointers and the dense form
    give the same bytes"""
    h, m = hashers(field, 4 if leaf_len == 4 else 2)
    dom = pc.domain_element(DOMAIN, m.p)
    rng = random.Random(0x7EE + leaf_len)
    for n in (1, 2, 3, 5, 64, 65, 1000):
        montgomery = n % 2 == 1
        # the model hashes at most 16 distinct leaves and the nodes above them; equal subtrees are hashed once
        distinct = [[rng.randrange(m.p) for _ in range(leaf_len)] for _ in range(min(n, 16))]
        leaves = [distinct[(i * 7) % len(distinct)] if n > 16 else distinct[i] for i in range(n)]
        want, empty = merkle_cached(m, dom, leaves)
        raw = pc.encode(field, pc.flat(leaves), montgomery)
        tree = h.merkle_tree(dev(torch_, raw, (n, leaf_len, 32)), montgomery=montgomery)
        got = pc.decode(field, raw_of(tree.nodes), montgomery)
        assert got == want, n
        P = (len(want) + 1) // 2
        assert got[P - 1 + n:] == [empty] * (P - n)
        assert pc.decode(field, tree.empty_hash(), montgomery) == [empty]
        depth = tree.levels + 3
        assert pc.decode(field, tree.root(), montgomery) == [want[0]]
        assert pc.decode(field, tree.root(depth), montgomery) == [m.merkle_root(dom, want, empty, depth)]
        for i in sorted({0, n // 2, n - 1}):
            assert pc.decode(field, b"".join(tree.path(i)), montgomery) == m.merkle_path(want, i), (n, i)
        if n in (3, 65):
            assert raw_of(h.merkle_tree(raw, leaf_len=leaf_len, montgomery=montgomery).nodes) == raw_of(tree.nodes)
            h.set_option("sparse", 0)
            assert raw_of(h.merkle_tree(dev(torch_, raw, (n, leaf_len, 32)), montgomery=montgomery).nodes) == raw_of(tree.nodes)
            h.set_option("sparse", 1)


def merkle_cached(m, dom, leaves):
    """Model.merkle with every distinct hash computed once: a tree of 1000 leaves drawn from 16 has few distinct subtrees"""
    memo = {}

    def hash_(x):
        x = tuple(x)
        if x not in memo:
            memo[x] = m.hash(dom, list(x))
        return memo[x]

    n = len(leaves)
    P = 1
    while P < n:
        P *= 2
    empty = hash_([1, 0, 0])
    tree = [empty] * (2 * P - 1)
    for i, leaf in enumerate(leaves):
        tree[P - 1 + i] = hash_([0] + list(leaf))
    for i in range(P - 2, -1, -1):
        tree[i] = hash_([1, tree[2 * i + 1], tree[2 * i + 2]])
    assert n > 8 or (tree, empty) == m.merkle(dom, leaves)
    return tree, empty


def test_out_and_overlap(hashers, torch_, ea):
    torch = torch_
    h, m = hashers("bls12_381", 2)
    rng = random.Random(9)
    rows = [[rng.randrange(m.p) for _ in range(3)] for _ in range(5)]
    raw = pc.encode("bls12_381", pc.flat(rows), True)
    t = dev(torch, raw, (5, 3, 32))
    out = torch.zeros((5, 2, 32), dtype=torch.uint8, device="cuda")
    assert h.sponge(t, 2, out=out) is out
    assert rows_of("bls12_381", raw_of(out), 5, 2, True) == [m.sponge(r, 2) for r in rows]
    with pytest.raises(ValueError, match="out: a contiguous uint8 GPU tensor of 5 x 2"):
        h.sponge(t, 2, out=torch.zeros((5, 3, 32), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out= goes with GPU tensors"):
        h.sponge(raw, 2, in_len=3, out=out)
    whole = torch.zeros((5 * 3 + 5 * 2, 32), dtype=torch.uint8, device="cuda")
    whole[:15] = t.reshape(15, 32)
    with pytest.raises(ea.MsmError, match="overlaps the input"):
        h.sponge(whole[:15].reshape(5, 3, 32), 2, out=whole[14:24].reshape(5, 2, 32))
    assert h.sponge(whole[:15].reshape(5, 3, 32), 2, out=whole[15:25].reshape(5, 2, 32)) is not None      # adjacent is fine
    assert raw_of(whole[15:25]) == raw_of(out)
    leaves = torch.zeros((4 + 7, 32), dtype=torch.uint8, device="cuda")
    with pytest.raises(ea.MsmError, match="overlaps the leaves"):
        h.merkle_tree(leaves[:4].reshape(4, 1, 32), out=leaves[3:10])
    tree = h.merkle_tree(leaves[:4].reshape(4, 1, 32), out=leaves[4:11])
    assert tree.nodes.data_ptr() == leaves[4:11].data_ptr()


def test_rate_one_hashes_and_builds_no_tree(hashers, torch_, ea):
    import ctypes

    par = dict(alpha=5, full_rounds=8, partial_rounds=20)
    m1 = pc.Model.generated("bls12_381", 1, **par)
    h, _ = hashers("bls12_381", 2)
    rng = random.Random(11)
    rows = [[rng.randrange(m1.p) for _ in range(3)] for _ in range(5)]
    raw = pc.encode("bls12_381", pc.flat(rows), True)
    with ea.Poseidon(h.dom, 1, parameters=par, domain=1) as h1:
        assert rows_of("bls12_381", raw_of(h1.sponge(dev(torch_, raw, (5, 3, 32)), 2)), 5, 2, True) == [m1.sponge(r, 2) for r in rows]
        with pytest.raises(ValueError, match="rate of at least 2"):
            h1.merkle_tree(raw, leaf_len=3)
        tree = np.zeros((1, 32), np.uint8)
        err = ea.load_library().mi355_msm_poseidon_merkle(h1.handle, tree.ctypes.data, raw, 1, 3, bytes(32), 0, None)
        assert err.code == -1 and b"rate of at least 2" in ctypes.string_at(err.message)
        ctypes.CDLL(None).free(ctypes.c_void_p(err.message))


# ---- the stream order of flag bit 1 ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def side(torch_):
    """(stream, calibrated delay) for the late producers of this module, once.  The stream comes from torch's high-priority pool, as in
    tests/test_gpu_mle.py: on HIP torch creates a pool stream when it is first handed out and the runtime gives it the least loaded
    hardware queue of its priority, so a stream drawn here from the default pool would move every later module's side stream to
    another queue -- and tests/test_gpu_sparse.py's late_out, which synchronises the default stream with a delay already enqueued, onto
    the default stream's own.  A producer is no less late at a higher priority."""
    stream = torch_.cuda.Stream(priority=-1)
    return stream, st.Delay(torch_, stream)


def _late_call(torch, stream, delay, raw, shape, out_shape, call):
    """the input and the out= tensor behind ONE late producer on a side stream, which fills the output with OUT_POISON before it hands
    over the input (a result written on any other stream is overwritten afterwards): the window is open immediately before the call
    and the producer took its time"""
    out = st.poisoned(torch, out_shape)
    t = st.late(torch, raw, stream, delay, shape=shape, fill=[out])
    with torch.cuda.stream(stream):
        assert st.window_open(t.produced) and st.window_open(out.produced), "invalid: the producer had finished before the call was made"
        got = call(t, out)
    stream.synchronize()
    assert st.closed(t, out), "invalid: the producer took %s ms" % st.delay_ms(t)
    return got


def _no_poison(raw):
    rows = [raw[i:i + 32] for i in range(0, len(raw), 32)]
    assert bytes([st.POISON]) * 32 not in rows and bytes([st.OUT_POISON]) * 32 not in rows


def test_hash_after_a_late_producer_on_a_side_stream(hashers, torch_, side):
    h, m = hashers("bls12_377", 2)
    stream, delay = side
    rng = random.Random(0x1A7E)
    rows = [[rng.randrange(m.p) for _ in range(5)] for _ in range(70)]
    want = [m.hash_many(h.domain, r, 2) for r in rows[:3]]
    rows = [rows[i % 3] for i in range(70)]
    raw = pc.encode("bls12_377", pc.flat(rows), True)
    got = _late_call(torch_, stream, delay, raw, (70, 5, 32), (70, 2, 32), lambda t, out: h.hash_many(t, 2, out=out))
    _no_poison(raw_of(got))
    assert rows_of("bls12_377", raw_of(got), 70, 2, True) == [want[i % 3] for i in range(70)]


def test_merkle_after_a_late_producer_on_a_side_stream(hashers, torch_, side):
    h, m = hashers("bls12_381", 2)
    stream, delay = side
    rng = random.Random(0x1A7F)
    leaves = [[rng.randrange(m.p)] for _ in range(5)]
    want, _ = m.merkle(h.domain, leaves)
    raw = pc.encode("bls12_381", pc.flat(leaves), True)
    tree = _late_call(torch_, stream, delay, raw, (5, 1, 32), (15, 32), lambda t, out: h.merkle_tree(t, out=out))
    _no_poison(raw_of(tree.nodes))
    assert pc.decode("bls12_381", raw_of(tree.nodes), True) == want
