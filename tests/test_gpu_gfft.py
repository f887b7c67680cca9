"""GPU: transforms of vectors of curve points (mi355_msm_fft_points[_device], csrc/group_fft.hpp) against the discrete-log oracle of
tests/gfft_cases.py: inputs h_j * G, expected output (the transform of h over Fr) * G, byte-equal on EVERY output.  The Fr transform
is ntt_cases.transform (Python integers) up to 2^12 points and the CPU oracle's oracle_ntt above; the multiples of G come from the
fixed-base entry on the GPU."""
import ctypes
import os
import re
import statistics
import time

import numpy as np
import pytest

import gfft_cases as gc
import ntt_cases as nc
import pymodel as pm
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctxs(ea):
    """one context per curve for the whole module"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = ea.MultiScalarMultContext(name)
        return made[name]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def doms(ea):
    """one domain per (family, size) for the whole module"""
    made = {}

    def get(name, n):
        key = (gc.field(name), n)
        if key not in made:
            made[key] = ea.Radix2EvaluationDomain(n, curve=name)
        return made[key]

    yield get
    for d in made.values():
        d.close()


def rows(t):
    """(n, stride) uint8 GPU tensor / array / bytes -> NumPy array on the host"""
    if hasattr(t, "is_cuda"):
        return t.cpu().numpy()
    return np.asarray(t)


def mismatches(got, want):
    got, want = rows(got), rows(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.flatnonzero((got != want).any(axis=1))[:8].tolist()


def batch_images(ea, name, log_lists, projective=False):
    """[images of h * G for each list of logs], ONE fixed-base call for all of them"""
    all_img = gc.device_images(ea, name, np.concatenate([gc.words(logs) for logs in log_lists]), projective)
    out, at = [], 0
    for logs in log_lists:
        out.append(all_img[at:at + len(logs)])
        at += len(logs)
    return out


# ---- 1. bytes, small ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gc.CURVE_NAMES)
def test_small_sizes_every_kind(ea, ctxs, doms, name):
    """n = 1 .. 512 (G2: .. 64; 512 is two blocks of butterflies and nine stages), kinds 0 - 3, the default offset and another, device
    and host pointers, Projective images once"""
    curve = pm.CURVES[name]
    ctx = ctxs(name)
    sizes = (1, 2, 4, 32, 64) if curve.ext == 2 else (1, 2, 4, 32, 512)
    cases, lists = [], []
    for n in sizes:
        logs = gc.random_logs(name, n, 0xA0 + n)
        lists.append(logs)
        for kind in gc.KINDS:
            for offset in ((None, gc.OTHER_OFFSET) if kind & 2 else (None,)):
                cases.append((n, kind, offset, len(lists) - 1))
                lists.append(gc.transform_logs(name, n, kind, logs, offset))
    imgs = batch_images(ea, name, lists)
    # (the lists alternate: the inputs of a size, then its expected outputs in the order of `cases`)
    pos = {}
    j = 0
    for n in sizes:
        pos[n] = j
        j += 1 + sum(1 for c in cases if c[0] == n)
    seen = {n: 0 for n in sizes}
    for n, kind, offset, _ in cases:
        seen[n] += 1
        pts, want = imgs[pos[n]], imgs[pos[n] + seen[n]]
        dom = doms(name, n)
        got = ctx.fft_points(dom, pts, kind=kind, offset=offset)
        assert got.is_cuda and tuple(got.shape) == (n, curve.affine_stride)
        assert not mismatches(got, want), (name, n, kind, offset, mismatches(got, want))
        if n <= 32:
            got_h = ctx.fft_points(dom, pts.cpu().numpy(), kind=kind, offset=offset)
            assert isinstance(got_h, np.ndarray) and not mismatches(got_h, want), (name, n, kind, offset, "host")
    # Projective images: the coset inverse at the second largest size
    n = sizes[-2]
    logs = lists[pos[n]]
    want_p = gc.device_images(ea, name, gc.transform_logs(name, n, nc.COSET_INVERSE, logs), projective=True)
    got = ctx.fft_points(doms(name, n), imgs[pos[n]], inverse=True, coset=True, projective=True)
    assert tuple(got.shape) == (n, curve.projective_bytes) and not mismatches(got, want_p)
    assert ctx.fft_points(doms(name, n), imgs[pos[n]].cpu().numpy().tobytes(), kind=3, projective=True) == rows(want_p).tobytes()


# ---- 2. degenerate inputs --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gc.CURVE_NAMES)
def test_degenerate_inputs(ea, ctxs, doms, name):
    import torch

    curve = pm.CURVES[name]
    r = curve.r
    ctx = ctxs(name)
    n = 64
    dom = doms(name, n)
    st = curve.affine_stride
    h = gc.random_logs(name, 1, 0xD0)[0]
    full = gc.random_logs(name, n, 0xD1)
    half = gc.random_logs(name, n // 2, 0xD2)
    inputs = {
        "all equal": [h] * n,
        "every second point at infinity": [v if i % 2 == 0 else 0 for i, v in enumerate(full)],
        "first stage cancels": [r - v for v in half] + half,        # h_j = r - h_(j + n/2)
        "first stage doubles": half + half,
    }
    lists = [full]
    for logs in inputs.values():
        lists.append(logs)
        lists += [gc.transform_logs(name, n, kind, logs) for kind in gc.KINDS]
    in_lens = (0, 1, 33)
    for m in in_lens:
        lists += [gc.transform_logs(name, n, kind, full[:m]) for kind in gc.KINDS]
    lists.append([n * h % r])
    imgs = batch_images(ea, name, lists)
    at = 1
    for label in inputs:
        pts = imgs[at]
        for kind in gc.KINDS:
            got = ctx.fft_points(dom, pts, kind=kind)
            assert not mismatches(got, imgs[at + 1 + kind]), (name, label, kind)
        at += 5
    # all points equal: out[0] = 64 P, the rest infinity
    got = rows(ctx.fft_points(dom, imgs[1]))
    assert got[0].tobytes() == rows(imgs[-1])[0].tobytes()
    assert got[1:].tobytes() == gc.infinity_image(curve) * (n - 1)
    # in_len: the bytes past it are stale (0xFF) and never read, on the device and from the host
    stale = torch.full((n, st), 0xFF, dtype=torch.uint8, device="cuda")
    for m in in_lens:
        buf = stale.clone()
        buf[:m] = imgs[0][:m]
        for kind in gc.KINDS:
            want = imgs[at + kind]
            assert not mismatches(ctx.fft_points(dom, buf, kind=kind, in_len=m), want), (name, m, kind)
        assert not mismatches(ctx.fft_points(dom, buf.cpu().numpy(), kind=3, in_len=m), imgs[at + 3]), (name, m, "host")
        at += 4
    got = rows(ctx.fft_points(dom, stale, in_len=0))
    assert got.tobytes() == gc.infinity_image(curve) * n
    # an infinity is what the flag byte says, whatever the coordinates hold
    pts = imgs[1 + 5].clone()          # every second point at infinity
    junk = imgs[0].clone()
    junk[:, 2 * curve.coord_bytes] = 1
    pts[1::2] = junk[1::2]
    assert not mismatches(ctx.fft_points(dom, pts, kind=2), imgs[1 + 5 + 1 + 2])


# ---- 3. independence ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bls12_381_g1", "bls12_377_g2"])
def test_results_do_not_depend_on_chunks_window_pointers_or_strides(ea, doms, name):
    import torch

    curve = pm.CURVES[name]
    n = 512
    st = curve.affine_stride
    dom = doms(name, n)
    logs = gc.random_logs(name, n, 0x1DE)
    pts, want_f, want_ci = batch_images(ea, name, [logs, gc.transform_logs(name, n, nc.FORWARD, logs), gc.transform_logs(name, n, nc.COSET_INVERSE, logs)])
    ctx = ea.MultiScalarMultContext(name)
    try:
        ref = {kind: ctx.fft_points(dom, pts, kind=kind) for kind in (nc.FORWARD, nc.COSET_FORWARD, nc.COSET_INVERSE)}
        assert not mismatches(ref[nc.FORWARD], want_f) and not mismatches(ref[nc.COSET_INVERSE], want_ci)
        assert ctx.query("fft_points_chunk") == (1 << 18 if curve.ext == 2 else 1 << 19)
        for chunk in (64, 256):
            ctx.set_option("fft_points_chunk", chunk)
            assert ctx.query("fft_points_chunk") == chunk
            for kind, want in ref.items():
                assert torch.equal(ctx.fft_points(dom, pts, kind=kind), want), (name, chunk, kind)
        for window in (3, 5):
            ctx.set_option("mul_window", window)
            for kind, want in ref.items():
                assert torch.equal(ctx.fft_points(dom, pts, kind=kind), want), (name, window, kind)
        ctx.set_option("mul_window", 0)
        ctx.set_option("fft_points_chunk", 0)
        host = pts.cpu().numpy()
        for kind, want in ref.items():
            assert np.array_equal(ctx.fft_points(dom, host, kind=kind), rows(want)), (name, kind, "host")
            # in place
            buf = pts.clone()
            assert ctx.fft_points(dom, buf, kind=kind, out=buf) is buf
            assert torch.equal(buf, want), (name, kind, "in place")
        # a stride of its own on both sides: the bytes between two images stay as they were
        wide, owide = st + 12, st + 20
        spread = torch.full((n, wide), 0x3C, dtype=torch.uint8, device="cuda")
        spread[:, :st] = pts
        out = torch.full((n, owide), 0xC3, dtype=torch.uint8, device="cuda")
        ctx.fft_points(dom, spread, kind=nc.COSET_INVERSE, stride=wide, out_stride=owide, out=out)
        assert torch.equal(out[:, :st], ref[nc.COSET_INVERSE]) and bool((out[:, st:] == 0xC3).all())
        got = ctx.fft_points(dom, spread.cpu().numpy(), kind=nc.COSET_INVERSE, stride=wide, out_stride=owide)
        assert np.array_equal(got[:, :st], rows(ref[nc.COSET_INVERSE])) and (got[:, st:] == 0).all()    # (the wrapper's own zeros)
        # in place with the same wide stride
        buf = spread.clone()
        ctx.fft_points(dom, buf, kind=nc.FORWARD, stride=wide, out_stride=wide, out=buf)
        assert torch.equal(buf[:, :st], ref[nc.FORWARD]) and bool((buf[:, st:] == 0x3C).all())
        assert ctx.query("fft_points_work_bytes") > 0 and ctx.query("last_fft_points_us") > 0 and ctx.query("last_fft_points_device_us") > 0
    finally:
        ctx.close()


# ---- 4. round trip and every output at size ------------------------------------------------------------------------------------------

def test_round_trip_and_forward_at_2_14(ea, ctxs, doms, oracle):
    import torch

    name = "bls12_381_g1"
    n = 1 << 14
    ctx, dom = ctxs(name), doms(name, n)
    logs = gc.random_logs(name, n, 0x214)
    want_logs = gc.transform_logs(name, n, nc.FORWARD, logs, oracle=oracle)
    pts = gc.device_images(ea, name, logs)
    want = gc.device_images(ea, name, want_logs)
    t0 = time.perf_counter()
    got = ctx.fft_points(dom, pts)
    back = ctx.ifft_points(dom, got)
    torch.cuda.synchronize()
    print("2^14 forward + inverse: %.1f ms (device %.1f ms for the inverse)" % ((time.perf_counter() - t0) * 1e3, ctx.query("last_fft_points_device_us") / 1e3))
    assert not mismatches(got, want)
    assert torch.equal(back, pts)


def test_forward_at_2_16_bls12_377(ea, ctxs, doms, oracle):
    name = "bls12_377_g1"
    n = 1 << 16
    ctx, dom = ctxs(name), doms(name, n)
    logs = gc.random_logs(name, n, 0x216)
    want = gc.device_images(ea, name, gc.transform_logs(name, n, nc.FORWARD, logs, oracle=oracle))
    got = ctx.fft_points(dom, gc.device_images(ea, name, logs))
    print("2^16 forward: device %.1f ms" % (ctx.query("last_fft_points_device_us") / 1e3))
    assert not mismatches(got, want)


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------

def test_lagrange_srs_commits_to_evaluations(ea, doms):
    """a monomial SRS [tau^j] G -> ifft_points -> the Lagrange SRS [L_i(tau)] G: the MSM of a polynomial's evaluations on it equals the
    MSM of its coefficients on the monomial SRS, byte for byte"""
    name = "bls12_381_g1"
    n = 1 << 10
    r = pm.CURVES[name].r
    dom = doms(name, n)
    tau = gc.random_logs(name, 1, 0x7A0)[0]
    powers, t = [], 1
    for _ in range(n):
        powers.append(t)
        t = t * tau % r
    monomial = gc.device_images(ea, name, powers)
    evals = gc.random_logs(name, n, 0xE7A)
    e_raw = nc.encode(gc.field(name), evals, normal=True)
    c_raw = dom.ifft(e_raw, montgomery=False)
    assert nc.decode(gc.field(name), c_raw, True) == nc.transform(gc.field(name), 10, nc.INVERSE, evals)
    ctx = ea.MultiScalarMultContext(name)
    try:
        lagrange = ctx.ifft_points(dom, monomial)
        ctx.set_bases(monomial)
        by_coefficients = ctx.run(c_raw)[0]
        ctx.set_bases(lagrange)
        by_evaluations = ctx.run(e_raw)[0]
    finally:
        ctx.close()
    assert by_evaluations == by_coefficients
    # and both are p(tau) * G
    p_tau = sum(c * pw for c, pw in zip(nc.decode(gc.field(name), c_raw, True), powers)) % r
    assert by_coefficients == rows(gc.device_images(ea, name, [p_tau], projective=True)).tobytes()


# ---- 6. errors and lifetime --------------------------------------------------------------------------------------------------------

def test_refusals_with_live_handles_and_lifetimes(ea):
    import torch

    name = "bls12_381_g1"
    lib = ea.load_library()
    n = 16
    logs = gc.random_logs(name, n, 0xE44)
    pts = gc.device_images(ea, name, logs)
    host = pts.cpu().numpy()
    want = gc.device_images(ea, name, gc.transform_logs(name, n, nc.INVERSE, logs))
    want32 = gc.device_images(ea, name, gc.transform_logs(name, 32, nc.INVERSE, logs))
    ctx = ea.MultiScalarMultContext(name)
    dom = ea.Radix2EvaluationDomain(n, curve=name)
    other_family = ea.Radix2EvaluationDomain(n, curve="bls12_377_g1")
    out = np.zeros((n, 144), dtype=np.uint8)
    P, O = host.ctypes.data, out.ctypes.data
    zero = ctypes.create_string_buffer(32)
    one = ctypes.create_string_buffer(((1 << 256) % pm.CURVES[name].r).to_bytes(32, "little"), 32)
    bad = [
        ((O, 104, P, n, 104, 4, 0, None), b"kind 4"), ((O, 104, P, n, 104, 0, 1, None), b"flag bits"), ((O, 104, P, n, 104, 0, 4, None), b"flag bits"),
        ((O, 104, P, n, 104, 0, 0, ctypes.addressof(one)), b"not over a coset"), ((O, 104, P, n, 104, 1, 0, ctypes.addressof(one)), b"not over a coset"),
        ((O, 104, P, n, 104, 2, 0, ctypes.addressof(zero)), b"offset is zero"),
        ((O, 104, P, n + 1, 104, 0, 0, None), b"exceeds the domain size"),
        ((O, 104, P, n, 96, 0, 0, None), b"stride 96"), ((O, 104, P, n, 106, 0, 0, None), b"stride 106"),
        ((O, 100, P, n, 104, 0, 0, None), b"out_stride 100"), ((O, 104, P, n, 104, 0, 2, None), b"out_stride 104"),
        ((None, 104, P, n, 104, 0, 0, None), b"null input or output"), ((O, 104, None, n, 104, 0, 0, None), b"null input or output"),
        ((P + 104, 104, P, n, 104, 0, 0, None), b"overlap in part"), ((P, 112, P, n, 104, 0, 0, None), b"overlap in part"),
    ]
    try:
        for args, word in bad:
            for fn, extra in ((lib.mi355_msm_fft_points, ()), (lib.mi355_msm_fft_points_device, (None,))):
                err = fn(ctx.context, dom.handle, *args, *extra)
                assert err.code == -1 and err.message, args
                msg = ctypes.string_at(err.message)
                ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
                assert word in msg, (args, msg)
        for c, d, word in ((None, dom.handle, b"null context"), (ctx.context, None, b"null domain"), (ctx.context, other_family.handle, b"curve families")):
            err = lib.mi355_msm_fft_points(c, d, O, 104, P, n, 104, 0, 0, None)
            assert err.code == -1 and word in ctypes.string_at(err.message)
            ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
        err = lib.mi355_msm_fft_points_device(ctx.context, dom.handle, pts.data_ptr() + 2, 104, pts.data_ptr() + 2, n, 104, 0, 0, None, None)
        assert err.code == -1 and b"aligned" in ctypes.string_at(err.message)
        ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
        with pytest.raises(ea.MsmError):
            ctx.set_option("fft_points_chunk", -1)
        sharded = ea.MultiScalarMultContext(name, devices=[0, 0])
        try:
            with pytest.raises(ea.MsmError) as ei:
                sharded.fft_points(dom, host)
            assert ei.value.code == -1 and "sharded" in ei.value.message
        finally:
            sharded.close()
        # after all that the handles still work; two domains of different sizes take turns on one context
        dom32 = ea.Radix2EvaluationDomain(32, curve=name)
        for _ in range(2):
            assert not mismatches(ctx.ifft_points(dom, pts), want)
            assert not mismatches(ctx.ifft_points(dom32, pts), want32)
        # a domain destroyed before the context ...
        dom32.close()
        assert not mismatches(ctx.ifft_points(dom, pts), want)
        with pytest.raises(ea.MsmError, match="closed"):
            ctx.ifft_points(dom32, pts)
        # ... and a context destroyed before the domain, which goes on serving another context and its own transforms
        ctx.close()
        ctx = ea.MultiScalarMultContext(name)
        assert not mismatches(ctx.ifft_points(dom, pts), want)
        vals = nc.encode(gc.field(name), logs, normal=True)
        assert nc.decode(gc.field(name), dom.ifft(vals, montgomery=False), True) == nc.transform(gc.field(name), 4, nc.INVERSE, logs)
    finally:
        ctx.close()
        dom.close()
        other_family.close()
    torch.cuda.synchronize()


# ---- 7. speed guard ----------------------------------------------------------------------------------------------------------------

MODELLED_FORWARD = 7.5     # (k - 1) / 2 multiplications per point at k = 16, against mul_points' one
MODELLED_INVERSE = 8.5     # one more per point, by n^-1


def speed_bounds():
    """(forward bound, inverse bound, source): 1.5 x the ratios profiles/gfft.txt measured on BLS12-381 G1 at 2^16 points (the margin
    covers box-to-box spread and clocks under the power limit), or 2 x the modelled ratios when there is no such file"""
    path = os.path.join(ROOT, "profiles", "gfft.txt")
    if os.path.exists(path):
        txt = open(path).read()
        mf = re.search(r"^bls12_381_g1 n=2\^16 ratio forward / mul_points: ([0-9.]+)", txt, flags=re.M)
        mi = re.search(r"^bls12_381_g1 n=2\^16 ratio inverse / mul_points: ([0-9.]+)", txt, flags=re.M)
        if mf and mi:
            return 1.5 * float(mf.group(1)), 1.5 * float(mi.group(1)), "profiles/gfft.txt"
    return 2 * MODELLED_FORWARD, 2 * MODELLED_INVERSE, "model"


def test_speed_guard_against_mul_points(ea, doms):
    """BLS12-381 G1, 2^16 device-resident subgroup points, warmed up, median of 5, host clock: the forward and the inverse transform
    against pairwise mul_points on the same points.  The count gives (k - 1) / 2 = 7.5 and 8.5 multiplications per point against one;
    the per-stage normalisations and table builds cost about what mul_points' own do per multiplication.  Bound: 1.5 x the `ratio`
    lines tools/gfft_bench.py wrote into profiles/gfft.txt on the MI355X; without that file 2 x the modelled ratios.  The bounds
    never come from this test's own timing of the code under test.  The file says 14.309 and 15.441 (bounds 21.46 and 23.16); this
    test measured on an MI355X: mul_points 6.21 ms, forward 88.95 ms (ratio 14.33), inverse 95.62 ms (ratio 15.41).  At 2^16 points a
    stage of 2^15 butterflies no longer fills the device and costs what a whole mul_points costs, so the ratio tends to k - 1 = 15, not
    to (k - 1) / 2; at 2^20 the file has 9.02 and 10.12 against 9.5 and 10.5."""
    import torch

    name = "bls12_381_g1"
    curve = pm.CURVES[name]
    n = 1 << 16
    bound_f, bound_i, source = speed_bounds()
    dom = doms(name, n)
    rs = np.random.RandomState(16)
    scal = rs.randint(0, 256, size=(n, 32), dtype=np.uint8)
    scal[:, 31] &= 0x3F                                   # below r
    d_s = torch.from_numpy(scal.reshape(-1)).cuda()
    with ea.FixedBase.get_window_table(gc.dc.generator_image(curve), curve=name, expected_scalars=n) as table:
        d_pts = table.msm(d_s)
    out = torch.zeros((n, curve.affine_stride), dtype=torch.uint8, device="cuda")
    ctx = ea.MultiScalarMultContext(name)
    try:
        def timed(call):
            def once():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                return time.perf_counter() - t0
            once()
            return statistics.median(once() for _ in range(5))

        t_mul = timed(lambda: ctx.mul_points(d_pts, d_s))
        t_fwd = timed(lambda: ctx.fft_points(dom, d_pts, out=out))
        t_inv = timed(lambda: ctx.fft_points(dom, d_pts, inverse=True, out=out))
    finally:
        ctx.close()
    print("2^16 points: mul_points %.2f ms; forward %.2f ms (ratio %.2f, bound %.2f); inverse %.2f ms (ratio %.2f, bound %.2f); bounds from %s"
          % (t_mul * 1e3, t_fwd * 1e3, t_fwd / t_mul, bound_f, t_inv * 1e3, t_inv / t_mul, bound_i, source))
    assert t_fwd <= bound_f * t_mul, (t_fwd, t_mul, source)
    assert t_inv <= bound_i * t_mul, (t_inv, t_mul, source)
