"""GPU: the stream-ordering contract of every device-pointer call of include/mi355_msm.h, with a producer that really is late
(tests/stream_cases.py).  The calls on the domain handle, mul_points, fixed_mul, fft_points and run_device enqueue their work on the
stream on which the input becomes ready; set_bases, check_bases and the codec synchronise the device first, whatever stream produced
their input.  Every input here holds poison until tens of milliseconds of device work have passed on a side stream, every test proves
on the host that the producer had not finished when the call was made, and the expected values come from the big-integer models of the
*_cases modules, computed on the CPU.  A launch on any other stream, a dropped producer synchronisation or a stream taken from the
wrong place reads the poison (or, with a late out=, has its result overwritten)."""
import ctypes
import random

import numpy as np
import pytest

import check_cases as cc
import codec_cases as cdc
import gfft_cases as gc
import ntt_cases as nc
import poly_cases as pc
import pymodel as pm
import quotient_cases as qc
import scan_cases as sc
import stream_cases as st

pytestmark = pytest.mark.gpu

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
# (poly_tile_log, n): a tile of 16 elements gives 257 three plan levels in the inversion, scan and division chains; the default tile
# of 1024 gives 1025 two, and runs the first call of each family alone
SHAPES = ((4, 257), (0, 1025))
CONTEXT_CURVES = ("bls12_377_g1", "bls12_381_g2")


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def lab(torch_):
    """the side stream, the calibrated delay and the bookkeeping of the late tensors of one call"""
    stream = torch_.cuda.Stream()
    return Lab(torch_, stream, st.Delay(torch_, stream))


@pytest.fixture(scope="module")
def domains(ea):
    """one domain per (field, k) for the whole module"""
    made = {}

    def get(field, k, tile_log=0):
        if (field, k) not in made:
            made[(field, k)] = ea.Radix2EvaluationDomain(1 << k, CURVE_OF[field])
        d = made[(field, k)]
        d.set_option("poly_tile_log", tile_log)
        return d

    yield get
    for d in made.values():
        d.close()


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


class Lab:
    def __init__(self, torch, stream, delay):
        self.torch, self.stream, self.delay = torch, stream, delay
        self.pending, self.deferred = [], []

    def _fill(self):
        fill, self.deferred = self.deferred, []
        return fill

    def late(self, *raws):
        """the byte strings as views of ONE late tensor (one delay in front of all of them, and of the fill of the late outputs asked
        for since the last call), each of shape (-1, 32)"""
        whole = st.late(self.torch, b"".join(raws), self.stream, self.delay, fill=self._fill())
        self.pending.append(whole)
        views, at = [], 0
        for raw in raws:
            views.append(whole[at:at + len(raw)].reshape(len(raw) // 32, 32))
            at += len(raw)
        return views[0] if len(views) == 1 else views

    def late_bytes(self, raw, width):
        """one late tensor of shape (-1, width)"""
        t = st.late(self.torch, raw, self.stream, self.delay, shape=(-1, width), fill=self._fill())
        self.pending.append(t)
        return t

    def out(self, *shape):
        """a late output whose producer is the one of the next late input: one delay in front of both, so that neither is produced
        while the other is still being enqueued"""
        t = st.poisoned(self.torch, shape)
        self.deferred.append(t)
        return t

    def out_alone(self, *shape):
        """a late output with a producer of its own, for a call without tensor inputs"""
        t = st.late_out(self.torch, shape, self.stream, self.delay)
        self.pending.append(t)
        return t

    def call(self, fn, current=True):
        """fn() with every producer still at work -- asserted, or the test is invalid -- under the side stream (current=False: under
        the default stream, for the calls that promise to wait for any producer); then the stream is synchronised and every producer
        must have taken its 10 ms"""
        torch, stream = self.torch, self.stream
        made, self.pending = self.pending, []
        assert not self.deferred, "a late output without a producer"
        assert made and all(st.window_open(t.produced) for t in made), "invalid: a producer had finished before the call was made"
        if current:
            with torch.cuda.stream(stream):
                res = fn()
        else:
            res = fn()
        stream.synchronize()
        assert st.closed(*made), "invalid: a producer took %s ms" % [st.delay_ms(t) for t in made]
        return res

    def upload(self, raw):
        """synchronously, on the default stream"""
        t = self.torch.frombuffer(bytearray(raw), dtype=self.torch.uint8).cuda().reshape(-1, 32)
        self.torch.cuda.synchronize()
        return t


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else (t.tobytes() if hasattr(t, "tobytes") else bytes(t))


def enc(field, vals):
    return nc.encode(field, vals, False)


def vals_of(field, raw_ints):
    return pc.values(field, raw_ints, False)


def outs(lab, n):
    """the two out= variants of a call: a fresh result, a late output"""
    return (lambda: None, lambda: lab.out(n, 32))


# ---- the control: this machine shows a mis-ordered read -------------------------------------------------------------------------------

def test_control_a_read_on_another_stream_sees_poison(lab):
    """a clone on a second stream that never waits for the first reads the poison and nothing else: the harness detects a mis-ordered
    read here.  (Defined memory is read; nothing faults.)"""
    torch = lab.torch
    t = lab.late(bytes(range(256)) * 64)
    other = torch.cuda.Stream()

    def read():
        with torch.cuda.stream(other):
            c = t.clone()
        other.synchronize()
        return c

    c = lab.call(read, current=False)
    assert bool((c == st.POISON).all())
    assert raw_of(t) == bytes(range(256)) * 64            # and the producer did deliver afterwards


# ---- the domain handle: stream-ordered ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_transforms(domains, lab, field):
    k = 10
    dom = domains(field, k)
    x = nc.random_values(field, 1 << k, 0x57A + k)
    raw = enc(field, x)
    for kind, name in ((nc.FORWARD, "fft"), (nc.INVERSE, "ifft"), (nc.COSET_FORWARD, "coset_fft"), (nc.COSET_INVERSE, "coset_ifft")):
        want = enc(field, nc.transform(field, k, kind, x))
        for make_out in outs(lab, 1 << k):
            out, d = make_out(), lab.late(raw)
            got = lab.call(lambda: getattr(dom, name)(d, out=out))
            assert raw_of(got) == want, (name, out is not None)
            assert raw_of(d) == raw


@pytest.mark.parametrize("tile_log,n", SHAPES)
@pytest.mark.parametrize("field", FIELDS)
def test_mul_and_vec_ops(domains, lab, field, tile_log, n):
    r = nc.modulus(field)
    dom = domains(field, 4, tile_log)
    pats = [pc.vector(field, n, tile_log or 10, 0x5E0 + j) for j in range(3)]
    a, b, c = (vals_of(field, p) for p in pats)
    s = random.Random(0x5E3).randrange(2, r)
    ops = [("mul", 2, (), [x * y % r for x, y in zip(a, b)]),
           ("add", 2, (), [(x + y) % r for x, y in zip(a, b)]),
           ("sub", 2, (), [(x - y) % r for x, y in zip(a, b)]),
           ("mul_sub", 3, (), [(x * y - z) % r for x, y, z in zip(a, b, c)]),
           ("scale", 1, (s,), [s * x % r for x in a])]
    for name, arity, tail, want in ops if tile_log else ops[:1]:
        for make_out in outs(lab, n):
            out = make_out()
            ins = lab.late(*[pc.to_raw(p) for p in pats[:arity]])
            ins = ins if arity > 1 else [ins]
            got = lab.call(lambda: getattr(dom, name)(*ins, *tail, out=out))
            assert raw_of(got) == enc(field, want), (name, out is not None)


@pytest.mark.parametrize("tile_log,n", SHAPES)
@pytest.mark.parametrize("field", FIELDS)
def test_batch_inversion(domains, lab, field, tile_log, n):
    r = nc.modulus(field)
    dom = domains(field, 4, tile_log)
    pat = pc.vector(field, n, tile_log or 10, 0x1B0)
    coeff = random.Random(0x1B1).randrange(2, r)
    want = enc(field, pc.ref_inverse(vals_of(field, pat), coeff, r))
    for make_out in outs(lab, n):
        out, v = make_out(), lab.late(pc.to_raw(pat))
        got = lab.call(lambda: dom.batch_inversion_and_mul(v, coeff, out=out))
        assert raw_of(got) == want, out is not None


@pytest.mark.parametrize("tile_log,n", SHAPES)
@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_and_divide_by_linear(domains, lab, field, tile_log, n):
    r = nc.modulus(field)
    dom = domains(field, 4, tile_log)
    pat = pc.vector(field, n, tile_log or 10, 0xE7A)
    vals = vals_of(field, pat)
    z = random.Random(0xE7B).randrange(2, r)
    v = lab.late(pc.to_raw(pat))
    assert lab.call(lambda: dom.evaluate(v, z)) == pc.ref_evaluate(vals, z, r)
    if not tile_log:
        return
    want_q, want_rem = pc.ref_divide(vals, z, r)
    for make_out in outs(lab, n - 1):
        out, v = make_out(), lab.late(pc.to_raw(pat))
        q, rem = lab.call(lambda: dom.divide_by_linear(v, z, out=out))
        assert raw_of(q) == enc(field, want_q) and rem == want_rem == pc.ref_evaluate(vals, z, r), out is not None


@pytest.mark.parametrize("field", FIELDS)
def test_lagrange_and_vanishing(domains, lab, field):
    """2^9 rows under a tile of 16: three levels in the inversion behind the Lagrange coefficients"""
    r = nc.modulus(field)
    k = 9
    dom = domains(field, k, 4)
    tau = random.Random(0x1A6).randrange(2, r)
    out = lab.out_alone(1 << k, 32)
    got = lab.call(lambda: dom.evaluate_all_lagrange_coefficients(tau, device=True, out=out))
    assert got is out and raw_of(out) == enc(field, pc.ref_lagrange(field, k, tau))
    pat = pc.vector(field, 257, 4, 0x1A7)
    zg_inv = pow((pow(nc.generator(field), 1 << k, r) - 1) % r, -1, r)
    want = enc(field, [x * zg_inv % r for x in vals_of(field, pat)])
    for make_out in outs(lab, 257):
        out, v = make_out(), lab.late(pc.to_raw(pat))
        got = lab.call(lambda: dom.divide_by_vanishing_poly_on_coset(v, out=out))
        assert raw_of(got) == want, out is not None


@pytest.mark.parametrize("tile_log,n", SHAPES)
@pytest.mark.parametrize("field", FIELDS)
def test_scans(domains, lab, field, tile_log, n):
    """prefix_product and prefix_sum, exclusive and inclusive, into a fresh result, a late output and in place; the total comes back
    as a host scalar after the chain"""
    r = nc.modulus(field)
    dom = domains(field, 4, tile_log)
    cases = [(name, op, inclusive) for name, op in (("prefix_product", sc.PRODUCT), ("prefix_sum", sc.SUM)) for inclusive in (False, True)]
    for name, op, inclusive in cases if tile_log else cases[:1]:
        pat = sc.vector(field, n, tile_log or 10, 0x5CA + op, zeros=op == sc.SUM)
        want, want_total = sc.ref_scan(vals_of(field, pat), op, inclusive, r)
        assert op == sc.SUM or want_total != 0
        for variant in ("fresh", "late out", "in place"):
            out = lab.out(n, 32) if variant == "late out" else None
            v = lab.late(pc.to_raw(pat))
            got, total = lab.call(lambda: getattr(dom, name)(v, inclusive=inclusive, out=v if variant == "in place" else out))
            assert raw_of(got) == enc(field, want) and total == want_total, (name, inclusive, variant)


@pytest.mark.parametrize("tile_log", [4, 0])
@pytest.mark.parametrize("field", FIELDS)
def test_permutation_product(domains, lab, field, tile_log):
    k, m = 9, 3
    dom = domains(field, k, tile_log)
    p = sc.permutation(field, k, m, 0x9E59)
    z, total = p.model()
    assert total == 1
    for make_out in outs(lab, p.n):
        out = make_out()
        w, s = lab.late(p.columns(p.wires, False, p.n), p.columns(p.sigmas, False, p.n))
        got, got_total = lab.call(lambda: dom.permutation_product(w.reshape(m, p.n, 32), s.reshape(m, p.n, 32), p.beta, p.gamma, p.ks, out=out))
        assert raw_of(got) == enc(field, z) and got_total == 1, out is not None


@pytest.mark.parametrize("field", FIELDS)
def test_plonk_quotient(domains, lab, field):
    """every vector late; a late output; only z late (the binding takes the stream from z); only the wires late"""
    for name, c, tile_logs in qc.row_cases(field):
        if name not in ("K5_n4", "nosel_m3"):
            continue
        want = enc(field, c.model(False))
        raws = dict(wires=c.columns(c.wires, c.M), sigmas=c.columns(c.sigmas, c.M), z=pc.to_raw(c.raw_z(False)), pi=pc.to_raw(c.pi))
        if c.selectors is not None:
            raws["selectors"] = c.columns(c.selectors, c.M)
        cols = lambda key, t: t if key in ("z", "pi") else t.reshape(-1, c.M, 32)
        for tile_log in tile_logs:
            dom = domains(field, c.K, 0 if tile_log == 10 else tile_log)
            for variant in ("all late", "late out", "only z late", "only wires late"):
                out = lab.out(c.M, 32) if variant == "late out" else None
                if variant.startswith("only"):
                    which = variant.split()[1]
                    v = {key: lab.upload(raw) for key, raw in raws.items() if key != which}
                    v[which] = lab.late(raws[which])
                else:
                    v = dict(zip(raws, lab.late(*raws.values())))
                v = {key: cols(key, t) for key, t in v.items()}
                got = lab.call(lambda: dom.plonk_quotient(v["wires"], v["sigmas"], v["z"], c.alpha, c.beta, c.gamma, c.ks, c.n,
                                                          selectors=v.get("selectors"), pi=v["pi"], offset=c.offset, out=out))
                assert raw_of(got) == want, (name, tile_log, variant)


@pytest.mark.parametrize("field", FIELDS)
def test_linear_combination(domains, lab, field):
    """m = 15 with the lengths mixed: into a fresh result, and with out= the first column (the longest moved there)"""
    r = nc.modulus(field)
    dom = domains(field, 4)
    cases = [case for case in qc.lincomb_cases(field) if len(case[0]) == 15]
    assert cases
    for cols, coeffs in cases:
        first = max(range(15), key=lambda j: len(cols[j]))
        order = [first] + [j for j in range(15) if j != first]
        cols, coeffs = [cols[j] for j in order], [coeffs[j] for j in order]
        want = enc(field, qc.ref_lincomb([vals_of(field, col) for col in cols], coeffs, r))
        for in_place in (False, True):
            tens = lab.late(*[pc.to_raw(col) for col in cols])
            got = lab.call(lambda: dom.linear_combination(tens, coeffs, out=tens[0] if in_place else None))
            assert raw_of(got) == want, ([len(col) for col in cols], in_place)
            assert not in_place or got.data_ptr() == tens[0].data_ptr()


@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_fft_points(ea, ctxs, domains, lab, name):
    """2^6 points h_j G late, the inverse transform (a monomial SRS into a Lagrange SRS): (the transform of the logs) G from the Python
    model, into a fresh result and a late output"""
    curve = pm.CURVES[name]
    n = 64
    ctx, dom = ctxs(name), domains(gc.field(name), 6)
    logs = gc.random_logs(name, n, 0x6FF7)
    pts = gc.model_images(name, logs)
    want = gc.model_images(name, gc.transform_logs(name, n, nc.INVERSE, logs))
    for late_out in (False, True):
        out = lab.out(n, curve.affine_stride) if late_out else None
        d = lab.late_bytes(pts, curve.affine_stride)
        got = lab.call(lambda: ctx.fft_points(dom, d, inverse=True, out=out))
        assert raw_of(got) == want, late_out


# ---- the context: ordered after any producer ------------------------------------------------------------------------------------------

N_CTX = 300


@pytest.mark.parametrize("name", CONTEXT_CURVES)
def test_check_bases_after_a_late_producer_on_any_stream(ctxs, lab, name):
    """the producer's stream is NOT current: the call promises to wait for whatever wrote the buffer"""
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    cases, statuses = cc.placed(name, N_CTX, seed=5)
    raw = cc.encode_all(curve, cases, False)
    host = ctx.check_bases(raw)
    assert host.status.tolist() == statuses
    d = lab.late_bytes(raw, curve.affine_stride)
    dev = lab.call(lambda: ctx.check_bases(d), current=False)
    assert dev.status.tolist() == statuses and dev.counts == host.counts and dev.first_invalid == host.first_invalid


@pytest.mark.parametrize("name", CONTEXT_CURVES)
def test_codec_after_a_late_producer_on_any_stream(ctxs, lab, name):
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    recs, statuses = cdc.placed(name, N_CTX, seed=6)
    raw = b"".join(recs)
    host = ctx.decompress_points(raw)
    assert host.status.tolist() == statuses
    d = lab.late_bytes(raw, curve.coord_bytes)
    dev = lab.call(lambda: ctx.decompress_points(d), current=False)
    assert dev.points.is_cuda and raw_of(dev.points) == host.points
    assert dev.status.tolist() == statuses and dev.counts == host.counts and dev.first_invalid == host.first_invalid
    back = ctx.compress_points(host.points)
    d = lab.late_bytes(host.points, curve.affine_stride)
    dev = lab.call(lambda: ctx.compress_points(d), current=False)
    assert raw_of(dev.points) == back.points and dev.status.tolist() == back.status.tolist() and dev.counts == back.counts


def msm_inputs(ea, oracle, name, seed):
    """(bases, scalars, the oracle's MSM) of N_CTX pairs"""
    cid = ea.CURVE_IDS[name]
    bases = ea.generate_points(N_CTX, distinct=N_CTX, seed=seed, curve=name)
    scalars = np.random.default_rng(seed).integers(0, 256, size=(N_CTX, 32), dtype=np.uint8)
    scalars[:, 31] &= 0x0F
    exp = ctypes.create_string_buffer(ea.projective_bytes(name))
    assert oracle.oracle_msm(cid, bases.ctypes.data, ea.affine_stride(name), scalars.ctypes.data, N_CTX, exp, 0) == 0
    return bases, scalars, exp.raw


@pytest.mark.parametrize("name", CONTEXT_CURVES)
def test_set_bases_after_a_late_producer_on_any_stream(ea, oracle, lab, name):
    bases, scalars, want = msm_inputs(ea, oracle, name, 0x5B)
    ctx = ea.MultiScalarMultContext(name)
    try:
        d = lab.late_bytes(bases, ea.affine_stride(name))
        lab.call(lambda: ctx.set_bases(d), current=False)
        assert ctx.run(scalars)[0] == want
    finally:
        ctx.close()


@pytest.mark.parametrize("name", CONTEXT_CURVES)
def test_run_with_late_scalars(ea, oracle, lab, name):
    """the scalars late on the current side stream, which is the stream the run is handed"""
    bases, scalars, want = msm_inputs(ea, oracle, name, 0x5C)
    ctx = ea.multi_scalar_mult_init(bases, name)
    try:
        assert ctx.run(scalars)[0] == want
        d = lab.late_bytes(scalars, 32)
        assert lab.call(lambda: ctx.run(d))[0] == want
    finally:
        ctx.close()


@pytest.mark.parametrize("name", CONTEXT_CURVES)
def test_mul_points_and_window_table_with_late_inputs(ea, ctxs, lab, name):
    """k_i P_i and k_i G with points and scalars late on the current side stream, against the same calls from host memory"""
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    pts = ea.generate_points(N_CTX, distinct=N_CTX, seed=0x5D, curve=name)
    ks = np.random.default_rng(0x5D).integers(0, 256, size=(N_CTX, 32), dtype=np.uint8)
    want = ctx.mul_points(pts, ks)
    d_p, d_k = st.late_many(lab.torch, [pts.tobytes(), ks.tobytes()], lab.stream, lab.delay)      # (one producer in front of both)
    lab.pending.append(d_p)
    got = lab.call(lambda: ctx.mul_points(d_p, d_k))
    assert got.is_cuda and (got.cpu().numpy() == want).all()
    with ea.FixedBase.get_window_table(bytes(pts[0]), curve=name) as table:
        want = table.msm(ks)
        d_k = lab.late_bytes(ks, 32)
        got = lab.call(lambda: table.msm(d_k))
        assert got.is_cuda and (got.cpu().numpy() == want).all()


# ---- the prover on a side stream ------------------------------------------------------------------------------------------------------

class Watched:
    """a domain whose every call first proves that the input uploaded last is still being produced"""

    def __init__(self, dom, lab, seen):
        self._dom, self._lab, self._seen = dom, lab, seen

    def __getattr__(self, name):
        fn = getattr(self._dom, name)
        if not callable(fn):
            return fn

        def checked(*a, **kw):
            made, self._lab.pending = self._lab.pending, []
            if made:
                assert st.window_open(made[-1].produced), "invalid: the producer had finished before %s was called" % name
                self._seen.extend(made)
            return fn(*a, **kw)

        return checked


def test_the_prover_on_a_side_stream(domains, lab, monkeypatch):
    """rounds two and three of tests/test_gpu_quotient.py's prover at k = 6, K = 9 over BLS12-381: every upload late, every call under
    the side stream, nothing synchronised between the calls but what they do themselves.  The rows and the coefficients of the
    quotient are the bytes of a second prover on the default stream with synchronous uploads, and the grand product closes"""
    import test_gpu_quotient as tq

    torch = lab.torch
    field, k, K = "bls12_381", 6, 9
    dom_n, dom_M = domains(field, k), domains(field, K)
    c = qc.Circuit(field, k, 0x3A + len(field))
    plain = tq.Round3(torch, dom_n, dom_M, c, 0x3B)
    want_t, want_rows = plain.quotient()
    torch.cuda.synchronize()
    assert plain.total == 1
    seen = []
    monkeypatch.setattr(tq, "dev", lambda torch, raw: lab.late(raw))
    with torch.cuda.stream(lab.stream):
        rd = tq.Round3(torch, Watched(dom_n, lab, seen), Watched(dom_M, lab, seen), c, 0x3B)
        t, rows = rd.quotient()
    lab.stream.synchronize()
    assert len(seen) == 5 + 5 + 13 + 1 + 5 + 1 and not lab.pending and st.closed(*seen)
    assert rd.total == 1 and rows == want_rows and t == want_t
