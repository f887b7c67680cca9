"""GPU: the segmented MSM (mi355_msm_segments, csrc/seg_msm.hpp) against the expectations of tests/segments_cases.py -- bytes at the
smallest shapes, tile edges, every window size and chunking, digit and law edges inside a bucket, isolation of a segment from its
neighbours, the shared form against the general one and against the big engine, the Montgomery entry, 2^18 / 2^16 points through the
discrete-log oracle and through linearity, chaining into the other calls, stream ordering, refusals, and a speed guard."""
import ctypes
import os
import re
import statistics
import time

import numpy as np
import pytest

import distinct_cases as dc
import pymodel as pm
import segments_cases as sc
import stream_cases as st
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def delay():
    import torch

    return st.Delay(torch, torch.cuda.Stream())


@pytest.fixture(scope="module")
def ctxs(ea):
    made = {}

    def get(name):
        if name not in made:
            made[name] = ea.MultiScalarMultContext(name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


def rows(out, size, stride=None):
    if hasattr(out, "cpu"):
        out = out.cpu().numpy()
    raw = out if isinstance(out, (bytes, bytearray)) else np.ascontiguousarray(out).tobytes()
    stride = stride or size
    return [bytes(raw[i:i + size]) for i in range(0, len(raw), stride)]


def mismatches(got, want):
    return [i for i, (g, e) in enumerate(zip(got, want)) if g != e] + ([-1] if len(got) != len(want) else [])


def want_rows(curve, values, projective=False):
    enc = curve.encode_projective_normalized if projective else curve.encode_affine
    return [enc(v) for v in values]


def options(ctx, **kw):
    for k, v in kw.items():
        ctx.set_option(k, v)
        assert ctx.query(k) == (v if v or k != "seg_tile" else 1024)


# ---- 1. bytes at the smallest shapes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CURVE_NAMES)
def test_bytes_small(ea, ctxs, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    logs, imgs, scalars, offsets, want = sc.small_case(name)
    raw = sc.scalar_bytes(scalars)
    A, P = curve.affine_stride, curve.projective_bytes
    got_a = ctx.msm_segments(imgs, raw, offsets)
    got_p = ctx.msm_segments(imgs, raw, offsets, projective=True)
    assert isinstance(got_a, bytes) and len(got_a) == len(sc.SMALL_LENGTHS) * A
    bad = mismatches(rows(got_a, A), want_rows(curve, want))
    assert not bad, (name, "affine", bad)
    bad = mismatches(rows(got_p, P), want_rows(curve, want, projective=True))
    assert not bad, (name, "projective", bad)
    # device pointers: the same bytes, as a GPU tensor; lengths= in place of offsets
    d_pts, d_s = torch.frombuffer(bytearray(imgs), dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    dev = ctx.msm_segments(d_pts, d_s, lengths=np.array(sc.SMALL_LENGTHS))
    assert dev.is_cuda and tuple(dev.shape) == (len(sc.SMALL_LENGTHS), A) and dev.cpu().numpy().tobytes() == got_a
    assert ctx.msm_segments(d_pts, d_s, torch.tensor(offsets), projective=True).cpu().numpy().tobytes() == got_p
    # a non-minimal stride and out_stride, host and device: the bytes between two images stay as they were
    wide = np.full((len(scalars), A + 24), 0x6B, dtype=np.uint8)
    wide[:, :A] = np.frombuffer(imgs, dtype=np.uint8).reshape(-1, A)
    got_w = ctx.msm_segments(wide, np.frombuffer(raw, dtype=np.uint8), offsets, stride=A + 24, out_stride=A + 16)
    assert isinstance(got_w, np.ndarray) and rows(got_w, A, A + 16) == rows(got_a, A) and not got_w[:, A:].any()
    o = torch.full((len(sc.SMALL_LENGTHS), P + 8), 0x44, dtype=torch.uint8, device="cuda")
    ctx.msm_segments(torch.from_numpy(wide).cuda(), d_s, offsets, stride=A + 24, out_stride=P + 8, projective=True, out=o)
    assert rows(o, P, P + 8) == rows(got_p, P) and bool((o[:, P:] == 0x44).all())
    # nothing in, nothing out; the module-level call on a throwaway context
    assert ctx.msm_segments(b"", b"", [0]) == b""
    assert ea.msm_segments(imgs, raw, offsets, curve=name) == got_a


# ---- 2. tile edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_tile_edges(ea, ctxs, name):
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    T = 64
    lengths = [T - 1, T, T + 1, 2 * T + 3, 5 * T]
    offsets = sc.offsets_of(lengths)
    logs, _, imgs = sc.base_set(name, "planted", offsets[-1], seed=2)
    scalars = sc.random_scalars(offsets[-1], 0x71E + curve.curve_id)
    want = want_rows(curve, sc.expected_dlog(curve, logs, scalars, offsets))
    try:
        for window in (0, 5):
            options(ctx, seg_tile=T, seg_window=window)
            got = rows(ctx.msm_segments(imgs, sc.scalar_bytes(scalars), offsets), curve.affine_stride)
            assert not mismatches(got, want), (name, window)
    finally:
        options(ctx, seg_tile=0, seg_window=0)


# ---- 3. every window size, every chunking ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g2"])
def test_every_window_size_and_chunking(ea, ctxs, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    lengths = [300, 0, 1, 65, 700, 2, 129, 0, 33]          # three classes of the automatic table, empty segments between them
    offsets = sc.offsets_of(lengths)
    n = offsets[-1]
    pts = torch.from_numpy(ea.generate_points(n, distinct=n, seed=31, curve=name)).cuda()
    s = torch.from_numpy(np.random.RandomState(31).randint(0, 256, size=32 * n, dtype=np.uint8)).cuda()
    auto = ctx.msm_segments(pts, s, offsets)
    try:
        for c in range(1, 10):
            options(ctx, seg_window=c)
            assert torch.equal(ctx.msm_segments(pts, s, offsets), auto), (name, c)
        options(ctx, seg_window=0, seg_chunk=3)                 # three chunks of three segments
        assert torch.equal(ctx.msm_segments(pts, s, offsets), auto), name
        options(ctx, seg_chunk=1, seg_tile=128)
        assert torch.equal(ctx.msm_segments(pts, s, offsets), auto), name
        assert ctx.msm_segments(pts.cpu().numpy(), s.cpu().numpy(), offsets).tobytes() == auto.cpu().numpy().tobytes()
    finally:
        options(ctx, seg_window=0, seg_chunk=0, seg_tile=0)


# ---- 4. digit and law edges inside a bucket --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CURVE_NAMES)
@pytest.mark.parametrize("kind", ["same", "pairs", "planted"])
def test_digit_and_law_edges(ea, ctxs, name, kind):
    """every edge scalar on a segment of equal bases (acc == P: the doubling inside a bucket, bucket + bucket doublings in the
    reduction), of P, -P pairs (acc == -P: sums to infinity) and with infinities planted; three segments, the scalars rotated"""
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    edges = sc.edge_scalars(curve)
    m = len(edges)
    offsets = sc.offsets_of([m, m, 2])
    logs, _, imgs = sc.base_set(name, kind, offsets[-1], seed=3)
    scalars = edges + edges[5:] + edges[:5] + [curve.r - 1, curve.r - 1]
    want = want_rows(curve, sc.expected_dlog(curve, logs, scalars, offsets))
    got = rows(ctx.msm_segments(imgs, sc.scalar_bytes(scalars), offsets), curve.affine_stride)
    assert not mismatches(got, want), (name, kind)


# ---- 5. isolation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_isolation_from_neighbours(ea, ctxs, name):
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    A = curve.affine_stride
    L = 97
    pts = ea.generate_points(3 * L + 40, distinct=3 * L + 40, seed=5, curve=name)
    rs = np.random.RandomState(5)
    s = rs.randint(0, 256, size=(3 * L + 40, 32), dtype=np.uint8)
    mine_p, mine_s = pts[:L], s[:L]
    alone = ctx.msm_segments(mine_p, mine_s, [0, L])
    for place, (before, after) in enumerate(((0, 2), (2, 0), (1, 1), (1, 1))):
        lens = [L + 20 * (place % 2)] * before + [L] + [L - 30 + place] * after
        ps, ss = [], []
        at = L + place
        for k, n in enumerate(lens):
            if k == before:
                ps.append(mine_p), ss.append(mine_s)
            else:
                ps.append(pts[at:at + n]), ss.append(s[at:at + n] ^ np.uint8(place))
                at += 7
        got = ctx.msm_segments(np.concatenate(ps), np.concatenate(ss), sc.offsets_of(lens))
        assert got[before].tobytes() == alone[0].tobytes(), (name, place)
    assert len(alone[0].tobytes()) == A


# ---- 6. the shared form ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_shared_form(ea, ctxs, name):
    import torch

    curve = pm.CURVES[name]
    ctx = ctxs(name)
    S, L = 33, 100
    pts = ea.generate_points(L, distinct=L, seed=6, curve=name)
    s = np.random.RandomState(6).randint(0, 256, size=(S, L, 32), dtype=np.uint8)
    shared = ctx.msm_segments(pts, s, shared=True, projective=True)
    assert isinstance(shared, np.ndarray) and shared.shape == (S, curve.projective_bytes)
    general = ctx.msm_segments(np.tile(pts, (S, 1)), s.reshape(-1, 32), sc.offsets_of([L] * S), projective=True)
    assert shared.tobytes() == general.tobytes()
    dev = ctx.msm_segments(torch.from_numpy(pts).cuda(), torch.from_numpy(s).cuda(), shared=True, projective=True)
    assert dev.cpu().numpy().tobytes() == shared.tobytes()
    # the big engine as a second witness: S batches over the same bases
    ctx.set_bases(pts)
    outs = ea.multi_scalar_mult(ctx, None, s.reshape(-1))
    assert len(outs) == S and b"".join(outs) == shared.tobytes()


# ---- 7. the Montgomery entry -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_377_g1", "bls12_381_g1"])
def test_montgomery_entry_on_ifft_output(ea, ctxs, name):
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    r = curve.r
    n = 256
    rs = np.random.RandomState(7)
    evals = [int.from_bytes(rs.bytes(32), "little") % r for _ in range(n)]
    dom = ea.Radix2EvaluationDomain(n, curve=name)
    try:
        coeffs = dom.ifft(pm.encode_scalars([e * (1 << 256) % r for e in evals]))
    finally:
        dom.close()
    rinv = pow(1 << 256, -1, r)
    ints = [a * rinv % r for a in pm.decode_scalars(bytes(coeffs))]
    pts = ea.generate_points(n, distinct=n, seed=77, curve=name)
    offsets = [0, 64, 64, 200, 256]
    assert ctx.msm_segments(pts, coeffs, offsets, montgomery=True).tobytes() == ctx.msm_segments(pts, pm.encode_scalars(ints), offsets).tobytes()


# ---- 8. at size: the discrete-log oracle on samples, linearity on everything -------------------------------------------------------

@pytest.mark.parametrize("name,logn", [("bls12_381_g1", 18), ("bls12_377_g2", 16)])
def test_at_size(ea, ctxs, oracle, name, logn):
    import torch

    curve = pm.CURVES[name]
    cid = curve.curve_id
    ctx = ctxs(name)
    n = 1 << logn
    r = curve.r
    rs = np.random.RandomState(80 + cid)
    lengths = []
    while sum(lengths) < n:
        lengths.append(min(int(rs.randint(1, 4097)), n - sum(lengths)))
    offsets = np.array(sc.offsets_of(lengths), dtype=np.uint64)
    S = len(lengths)
    logs, _ = dc.make_logs(cid, n, 0x5E6)
    s = dc.make_scalars(cid, n, 0x5E6, "any256")
    bases = dc.device_bases(ea, name, logs)
    out = ctx.msm_segments(bases, torch.from_numpy(dc.as_bytes(s).reshape(-1)).cuda(), offsets)
    assert out.is_cuda and tuple(out.shape) == (S, curve.affine_stride)
    host = out.cpu().numpy()
    # 64 sampled segments, each by one oracle multiplication
    pick = sorted(rs.choice(S, size=min(64, S), replace=False).tolist())
    ks = [dc.weighted_sum256(logs[int(offsets[k]):int(offsets[k + 1])], s[int(offsets[k]):int(offsets[k + 1])]) % r for k in pick]
    want = [dc.affine_of_projective(curve, img) for img in dc.oracle_mul(oracle, curve, dc.generator_image(curve), ks)]
    bad = [k for k, w in zip(pick, want) if host[k].tobytes() != w]
    assert not bad, (name, bad[:8])
    # all of them at once: sum_s rho_s out[s] by the big engine, against ((sum_s rho_s sum_i s_i h_i) mod r) G
    rho = dc.make_scalars(cid, S, 0x5E7, "uniform")
    seg_of = np.repeat(np.arange(S), lengths)
    rho_int = [dc.row_int(row) for row in rho]
    s_raw = dc.as_bytes(s)
    w = np.zeros((n, 4), dtype=np.uint64)
    for i in range(n):
        w[i] = dc.int_row(rho_int[seg_of[i]] * int.from_bytes(s_raw[i].tobytes(), "little") % r)
    ctx.set_bases(out)
    got = ctx.run(torch.from_numpy(dc.as_bytes(rho).reshape(-1)).cuda())[0]
    assert got == dc.expected(oracle, curve, logs, w), name


# ---- 9. chaining -----------------------------------------------------------------------------------------------------------------

def test_output_feeds_the_other_calls(ea, ctxs, oracle):
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    S, L = 16, 40
    logs, _, imgs = sc.base_set(name, "planted", S * L, seed=9)
    scalars = sc.random_scalars(S * L, 0x99)
    offsets = sc.offsets_of([L] * S)
    vals = sc.expected_dlog(curve, logs, scalars, offsets)
    out = ctx.msm_segments(torch.frombuffer(bytearray(imgs), dtype=torch.uint8).cuda(), torch.frombuffer(bytearray(sc.scalar_bytes(scalars)), dtype=torch.uint8).cuda(),
                           offsets)
    assert rows(out, curve.affine_stride) == want_rows(curve, vals)
    # (the rows above ARE the oracle's bytes, so the two legs below compare the GPU's own functions on equal bytes: what they pin is
    # that the result tensor is taken as it stands, without a copy or a restride; the oracle itself speaks in the set_bases + run leg)
    # compress_points: the records of the model points
    comp = ctx.compress_points(out)
    assert comp.ok
    want_c = ctx.compress_points(sc.images(curve, vals))
    assert comp.points.cpu().numpy().tobytes() == want_c.points
    # set_bases + run: sum_s rho_s out[s]
    rho = sc.random_scalars(S, 0x9A, curve)
    ctx.set_bases(out)
    got = ctx.run(sc.scalar_bytes(rho))[0]
    k = sum(a * b for a, b in zip(rho, sc.segment_logs(curve, logs, scalars, offsets))) % curve.r
    assert got == dc.oracle_mul(oracle, curve, dc.generator_image(curve), [k])[0]
    # fft_points over the 16 sums: the same transform of the model images
    dom = ea.Radix2EvaluationDomain(S, curve=name)
    try:
        a = ctx.fft_points(dom, out)
        b = ctx.fft_points(dom, torch.frombuffer(bytearray(sc.images(curve, vals)), dtype=torch.uint8).cuda())
        assert torch.equal(a, b)
    finally:
        dom.close()


# ---- 10. stream ordering ---------------------------------------------------------------------------------------------------------

def test_stream_ordering(ea, ctxs, delay):
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    A = curve.affine_stride
    logs, imgs, scalars, offsets, want = sc.small_case(name)
    raw = sc.scalar_bytes(scalars)
    ref = ctx.msm_segments(imgs, raw, offsets)
    S = len(offsets) - 1
    stream = torch.cuda.Stream()
    # late points and late scalars behind one producer on a side stream
    d_pts, d_s = st.late_many(torch, [imgs, raw], stream, delay)
    assert st.window_open(d_pts.produced) and st.window_open(d_s.produced)
    with torch.cuda.stream(stream):
        got = ctx.msm_segments(d_pts, d_s, offsets)
    stream.synchronize()
    assert st.closed(d_pts, d_s)
    assert got.cpu().numpy().tobytes() == ref
    # a late out=: its producer overwrites it after the delay; the result must land behind that
    d_pts2 = torch.frombuffer(bytearray(imgs), dtype=torch.uint8).cuda()
    d_s2 = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    o = st.late_out(torch, (S, A), stream, delay)
    assert st.window_open(o.produced)
    with torch.cuda.stream(stream):
        ctx.msm_segments(d_pts2, d_s2, offsets, out=o)
    stream.synchronize()
    assert st.closed(o)
    assert o.cpu().numpy().tobytes() == ref


# ---- 11. errors and lifetime -----------------------------------------------------------------------------------------------------

def test_errors_and_lifetime(ea):
    import torch

    name = "bls12_381_g1"
    lib = ea.load_library()
    n = 100
    pts = ea.generate_points(n, distinct=n, seed=11, curve=name)
    raw = np.random.RandomState(11).randint(0, 256, size=32 * n, dtype=np.uint8)
    ctx = ea.MultiScalarMultContext(name)
    offsets = [0, 10, 10, 60, 100]
    good = ctx.msm_segments(pts, raw, offsets)
    pbuf = ctypes.create_string_buffer(pts.tobytes(), n * 104)
    sbuf = ctypes.create_string_buffer(raw.tobytes(), 32 * n)
    out = ctypes.create_string_buffer(144 * n)
    P, S, O = ctypes.addressof(pbuf), ctypes.addressof(sbuf), ctypes.addressof(out)
    U = ctypes.c_uint64
    offs = lambda *v: (U * len(v))(*v)
    ok = offs(*offsets)
    fake_stream = ctypes.c_void_p(8)
    bad_calls = [
        ((None, n, 104, S, n, ok, 4, 0, O, 104, None), b"null points"),
        ((P, n, 104, None, n, ok, 4, 0, O, 104, None), b"null scalars"),
        ((P, n, 104, S, n, ok, 4, 0, None, 104, None), b"null output"),
        ((P, n, 104, S, n, None, 4, 0, O, 104, None), b"null offsets"),
        ((P, n, 96, S, n, ok, 4, 0, O, 104, None), b"stride 96"),
        ((P, n, 106, S, n, ok, 4, 0, O, 104, None), b"stride 106"),
        ((P, n, 104, S, n, ok, 4, 0, O, 100, None), b"out_stride 100"),
        ((P, n, 104, S, n, ok, 4, 0, O, 106, None), b"out_stride 106"),
        ((P, n, 104, S, n, ok, 4, 8, O, 104, None), b"out_stride 104"),
        ((P, n, 104, S, n, offs(1, 10, 10, 60, 100), 4, 0, O, 104, None), b"offsets[0] = 1"),
        ((P, n, 104, S, n, offs(0, 10, 9, 60, 100), 4, 0, O, 104, None), b"offsets[2] = 9 is smaller"),
        ((P, n, 104, S, n, offs(0, 10, 10, 60, 99), 4, 0, O, 104, None), b"offsets[4] = 99"),
        ((P, n, 104, S, n - 1, ok, 4, 0, O, 104, None), b"nscalars 99"),
        ((P, n, 104, S, n, ok, 4, 4, O, 104, None), b"offsets must be NULL"),
        ((P, 25, 104, S, 99, None, 4, 4, O, 104, None), b"nscalars 99"),
        ((P, 1 << 32, 104, S, 1 << 32, None, 1, 4, O, 104, None), b"npoints"),
        ((P, n, 104, S, n, ok, 4, 16, O, 104, None), b"flag bits 0x10"),
        ((P, n, 104, S, n, ok, 4, 0x80000000, O, 104, None), b"flag bits"),
        ((P, n, 104, S, n, ok, 4, 0, P + 208, 104, None), b"out overlaps points"),
        ((P, n, 104, S, n, ok, 4, 0, S + 64, 104, None), b"out overlaps scalars"),
        ((P, n, 104, S, n, ok, 4, 0, O, 104, fake_stream), b"stream"),
        ((P + 1, n, 104, S, n, ok, 4, 2, O, 104, None), b"4-byte aligned"),
    ]
    free = ctypes.CDLL(None).free
    for args, phrase in bad_calls:
        err = lib.mi355_msm_segments(ctx.context, *args)
        assert err.code == -1 and err.message, args
        msg = ctypes.string_at(err.message)
        free(ctypes.c_void_p(err.message))
        assert phrase in msg, (phrase, msg)
        assert np.array_equal(ctx.msm_segments(pts, raw, offsets), good)       # a valid call works after each refusal
    err = lib.mi355_msm_segments(None, P, n, 104, S, n, ok, 4, 0, O, 104, None)
    assert err.code == -1 and b"null context" in ctypes.string_at(err.message)
    free(ctypes.c_void_p(err.message))
    # nsegments = 0 succeeds and writes nothing
    assert lib.mi355_msm_segments(ctx.context, None, 0, 104, None, 0, offs(0), 0, 0, None, 104, None).code == 0
    for key, value in (("seg_window", 10), ("seg_window", -1), ("seg_tile", 96), ("seg_tile", 32), ("seg_tile", 8192), ("seg_chunk", -1)):
        with pytest.raises(ea.MsmError):
            ctx.set_option(key, value)
    with pytest.raises(ValueError, match=r"offsets\[2\]"):
        ctx.msm_segments(pts, raw, [0, 10, 9, 60, 100])
    # a sharded context refuses, with a message
    sharded = ea.MultiScalarMultContext(name, devices=[0, 0])
    try:
        with pytest.raises(ea.MsmError) as ei:
            sharded.msm_segments(pts, raw, offsets)
        assert ei.value.code == -1 and "sharded" in ei.value.message
    finally:
        sharded.close()
    assert np.array_equal(ctx.msm_segments(pts, raw, offsets), good)
    assert ctx.query("last_segments_us") > 0 and ctx.query("seg_work_bytes") > 0
    # the context remains usable for run
    ctx.set_bases(pts)
    one = ctx.run(raw)[0]
    assert one == ctx.msm_segments(pts, raw, [0, n], projective=True).tobytes()
    ctx.close()
    torch.cuda.synchronize()


# ---- 12. speed guard -------------------------------------------------------------------------------------------------------------

def speed_bound():
    """(bound, source): 1.5 x the ratio profiles/segments.txt measured for BLS12-381 G1, S = 256, L = 1024, general form, against
    mul_points on the same pairs; without that file the call must simply not be slower: 1.0"""
    path = os.path.join(ROOT, "profiles", "segments.txt")
    if os.path.exists(path):
        m = re.search(r"^bls12_381_g1 guard ratio msm_segments S=256 L=1024 / mul_points: ([0-9.]+)", open(path).read(), flags=re.M)
        if m:
            return 1.5 * float(m.group(1)), "profiles/segments.txt"
    return 1.0, "no profile"


def test_speed_guard_against_mul_points(ea):
    """BLS12-381 G1, S = 256 segments of L = 1024 pairs, device-resident, warmed up, median of 5, host clock around calls that end
    synchronised: msm_segments against mul_points on the same 2^18 pairs (which never sums).  The bound is never taken from this
    test's own timing."""
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    S, L = 256, 1024
    n = S * L
    bound, source = speed_bound()
    d_pts = torch.from_numpy(ea.generate_points(n, seed=12, curve=name)).cuda()
    d_s = torch.from_numpy(np.random.RandomState(12).randint(0, 256, size=32 * n, dtype=np.uint8)).cuda()
    offsets = np.arange(S + 1, dtype=np.uint64) * L
    ctx = ea.MultiScalarMultContext(name)
    try:
        def timed(call):
            def once():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            once()
            return statistics.median(once() for _ in range(5))

        t_mul = timed(lambda: ctx.mul_points(d_pts, d_s))
        t_seg = timed(lambda: ctx.msm_segments(d_pts, d_s, offsets))
    finally:
        ctx.close()
    print("S=256 L=1024: mul_points %.2f ms; msm_segments %.2f ms (ratio %.3f, bound %.3f from %s)" % (t_mul * 1e3, t_seg * 1e3, t_seg / t_mul, bound, source))
    assert t_seg <= bound * t_mul, (t_seg, t_mul, source)
