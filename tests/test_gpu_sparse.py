"""GPU: resident sparse matrices over Fr and y = M z (csrc/sparse.hpp, csrc/msm_sparse.hpp) through the Python layer, byte for byte
against Python big integers (tests/sparse_cases.py) at every edge the kernels have -- lane and block boundaries, the levels of the
prefix sum over the lanes, empty rows, one row that holds everything, the worst case of the lazy sums --; the stream order of the
device-pointer form of apply, pinned with a late producer as tests/test_gpu_stream_order.py pins the _device calls; Groth16's witness
map from the assignment to the coefficients of h in device memory, judged by an identity at a random point; and a speed guard against
the forward transform."""
import ctypes
import os
import random
import re
import statistics
import time

import numpy as np
import pytest

import ntt_cases as nc
import sparse_cases as sp
import stream_cases as st
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


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
def consts(ea):
    """E entries per lane and L lanes per block, as the library states them"""
    lib = ea.load_library()
    v = ctypes.c_uint64()
    out = []
    for key in (b"entries_per_lane", b"block_lanes"):
        assert lib.mi355_msm_sparse_query(None, key, ctypes.byref(v)).code == 0
        out.append(int(v.value))
    return tuple(out)


def dev(torch, raw):
    return torch.frombuffer(bytearray(raw) if len(raw) else bytearray(32), dtype=torch.uint8).cuda()[:len(raw)].reshape(-1, 32)


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else (t.tobytes() if hasattr(t, "tobytes") else bytes(t))


def matrix_of(dom, c, create_normal):
    return dom.sparse_matrix(c.rows, c.cols, np.array(c.row_ptr, dtype=np.uint64), np.array(c.col_idx, dtype=np.uint32), c.values_raw(),
                             montgomery=not create_normal)


def report_mismatches(got_raw, want_raw, what):
    got = np.frombuffer(got_raw, dtype=np.uint8).reshape(-1, 32)
    want = np.frombuffer(want_raw, dtype=np.uint8).reshape(-1, 32)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        pytest.fail("%s: %d of %d rows differ; first at %s" % (what, bad.size, got.shape[0], bad[:8].tolist()))


# ---- y = M z against the model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_apply_against_the_model(domains, torch_, consts, field):
    """every case of the generator, the coefficients given in both forms, the call in both forms, host and device pointers: the bytes of
    the model, and the same bytes on both paths; the handle reports what it was given"""
    E, L = consts
    for c in sp.cases(field, E, L):
        dom = domains(field, 4, 4 if c.tile4 else 0)
        for create_normal in (0, 1):
            with matrix_of(dom, c, create_normal) as M:
                assert (M.rows, M.cols, M.nnz) == (c.rows, c.cols, c.nnz)
                assert (M.query("entries_per_lane"), M.query("block_lanes")) == (E, L)
                assert M.query("work_bytes") >= 32 * (c.nnz + c.cols)
                for normal in (0, 1):
                    want = c.expected(create_normal, normal)
                    what = (c.name, field, create_normal, normal)
                    host = M.apply(c.z_raw(), montgomery=not normal)
                    assert isinstance(host, np.ndarray) and host.shape == (c.rows, 32)
                    report_mismatches(raw_of(host), want, what + ("host",))
                    got = M.apply(dev(torch_, c.z_raw()), montgomery=not normal)
                    assert got.is_cuda and tuple(got.shape) == (c.rows, 32)
                    report_mismatches(raw_of(got), want, what + ("device",))


def test_the_scan_levels_are_reached(ea, consts):
    """with tiles of 16 the prefix sum over the lanes of 16 E + 1 entries has two levels and that of 256 E + 3 entries three: the work
    memory of the scan on the domain says so"""
    E, L = consts
    cs = {c.name: c for c in sp.cases("bls12_381", E, L)}
    sizes = []
    for n in (E + 1, 16 * E + 1, 256 * E + 3):
        c = cs["one row of %d" % n]
        with ea.Radix2EvaluationDomain(16, CURVE_OF["bls12_381"]) as dom:
            dom.set_option("poly_tile_log", 4)
            with matrix_of(dom, c, 0) as M:
                M.apply(c.z_raw())
            sizes.append(dom.query("scan_work_bytes"))
    assert sizes[0] < sizes[1] < sizes[2], sizes


@pytest.mark.parametrize("field", FIELDS)
def test_equal_residues_give_equal_results_and_calls_repeat(ea, domains, torch_, consts, field):
    """a matrix created from plain integers and one created from the arkworks images of the same residues; apply twice; two matrices
    on one domain, used in turn, do not disturb each other"""
    E, L = consts
    r = nc.modulus(field)
    rng = random.Random(0xA11CE)
    dom = domains(field, 4)
    c = sp.Case("residues", field, sp.lengths_with_ends([E, 3 * E], 5 * E + 3, rng), 9, rng)
    other = sp.Case("other", field, [3 * E + 1, 0, 2], 9, rng)
    ints = nc.decode(field, c.values_raw(), True)
    rp, ci = np.array(c.row_ptr, dtype=np.uint64), np.array(c.col_idx, dtype=np.uint32)
    z = dev(torch_, c.z_raw())
    want = c.expected(True, False)
    with dom.sparse_matrix(c.rows, c.cols, rp, ci, nc.encode(field, ints, True), montgomery=False) as plain, \
            dom.sparse_matrix(c.rows, c.cols, rp, ci, nc.encode(field, ints, False), montgomery=True) as mont, \
            matrix_of(dom, other, 0) as second:
        first = raw_of(plain.apply(z))
        assert first == want
        assert raw_of(mont.apply(z)) == want
        assert raw_of(second.apply(dev(torch_, other.z_raw()))) == other.expected(False, False)
        assert raw_of(plain.apply(z)) == want and raw_of(plain.apply(c.z_raw())) == want
        assert raw_of(second.apply(other.z_raw())) == other.expected(False, False)
    # arkworks' Matrix<F> as lists of (coefficient, column): the same matrix again, integers of any size
    rows_list = [[(ints[k] + (k % 3) * r, c.col_idx[k]) for k in range(a, b)] for a, b in zip(c.row_ptr, c.row_ptr[1:])]
    with ea.SparseMatrix.from_rows(dom, rows_list, c.cols) as M:
        assert M.dom is dom and (M.rows, M.cols, M.nnz) == (c.rows, c.cols, c.nnz)
        assert raw_of(M.apply(z)) == want
    with pytest.raises(ea.MsmError, match="closed"):
        M.apply(z)


def test_refusals_on_the_handle(ea, domains, torch_, consts):
    """what needs a matrix to be judged: an output that overlaps z in part, shapes, another device's memory is not at hand here; and
    what create refuses reaches the caller as MsmError with the row named"""
    torch = torch_
    dom = domains("bls12_381", 4)
    rng = random.Random(7)
    c = sp.Case("square", "bls12_381", [2, 3, 1, 0, 2, 1], 6, rng)
    with matrix_of(dom, c, 0) as M:
        buf = torch.zeros((16, 32), dtype=torch.uint8, device="cuda")
        for lo in (0, 3, 5):
            with pytest.raises(ea.MsmError, match="overlaps z"):
                M.apply(buf[2:8], out=buf[lo:lo + 6])
        got = M.apply(buf[0:6], out=buf[6:12])                                 # neighbours do not overlap
        assert got.data_ptr() == buf[6:12].data_ptr()
        with pytest.raises(ValueError, match="z: 6 32-byte elements"):
            M.apply(buf[0:5])
        with pytest.raises(ValueError, match="out: a contiguous uint8 GPU tensor of shape"):
            M.apply(buf[0:6], out=buf[6:11])
        with pytest.raises(ValueError, match="out= goes with GPU tensors"):
            M.apply(bytes(6 * 32), out=buf[6:12])
        err = ea.load_library().mi355_msm_sparse_apply(M.handle, buf[6:12].data_ptr(), buf.data_ptr(), 0, ctypes.c_void_p(64))
        assert err.code == -1
        ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
    rp = np.array([0, 2, 1, 3], dtype=np.uint64)
    with pytest.raises(ea.MsmError, match="row 1: row_ptr decreases"):
        dom.sparse_matrix(3, 5, rp, np.zeros(3, np.uint32), bytes(96))
    with pytest.raises(ea.MsmError, match="row 2: column index 5"):
        dom.sparse_matrix(3, 5, np.array([0, 2, 2, 3], np.uint64), np.array([0, 4, 5], np.uint32), bytes(96))


# ---- stream order ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", FIELDS)
def test_apply_after_late_producers_on_a_side_stream(domains, torch_, consts, field):
    """flag bit 1 promises what the _device calls promise: the work is enqueued on the stream on which z becomes ready.  z has a producer
    that is late on a side stream and fills out= behind the same delay (a result written on any other stream is overwritten afterwards);
    the window is open immediately before the call, the producer took its time, the result is the model's and no poison is left"""
    torch = torch_
    E, L = consts
    dom = domains(field, 4)
    rng = random.Random(0x57EA)
    c = sp.Case("late", field, sp.lengths_with_ends([E, 2 * E - 1, E * L], E * L + 2 * E + 5, rng), 33, rng)
    want = c.expected(False, False)
    assert bytes([st.POISON]) * 32 not in [want[i:i + 32] for i in range(0, len(want), 32)]
    stream = torch.cuda.Stream()
    delay = st.Delay(torch, stream)
    with matrix_of(dom, c, 0) as M:
        for with_out in (False, True):
            # (out= is allocated and poisoned BEFORE the delay is enqueued, as everywhere else: poisoned() synchronises the default stream,
            #  and a default-stream launch can queue up behind the delay -- which hardware queue a stream shares depends on how many streams
            #  the process has made -- so that z's producer would be through by the time the call is made)
            out = st.poisoned(torch, (c.rows, 32)) if with_out else None
            z = st.late(torch, c.z_raw(), stream, delay, shape=(c.cols, 32), fill=[out] if with_out else ())
            made = [z] + ([out] if with_out else [])
            with torch.cuda.stream(stream):
                assert all(st.window_open(t.produced) for t in made), "invalid: a producer had finished before the call was made"
                got = M.apply(z, out=out)
            stream.synchronize()
            assert st.closed(*made), "invalid: a producer took %s ms" % [st.delay_ms(t) for t in made]
            assert not with_out or got.data_ptr() == out.data_ptr()
            raw = raw_of(got)
            report_mismatches(raw, want, (field, with_out))
            rows = [raw[i:i + 32] for i in range(0, len(raw), 32)]
            assert bytes([st.POISON]) * 32 not in rows and bytes([st.OUT_POISON]) * 32 not in rows


# ---- Groth16's witness map -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k, slack", [(4, 0), (4, 5), (6, 0), (6, 9)])
@pytest.mark.parametrize("field", FIELDS)
def test_groth16_witness_map(ea, domains, torch_, field, k, slack):
    """n + num_inputs equal to the domain's size and below it; a satisfied instance and one whose C misses a row.  h has `size`
    coefficients, satisfies (sum L_i(tau) a_i)(sum L_i(tau) b_i) - sum L_i(tau) a_i b_i == h(tau)(tau^size - 1) at a random tau in
    Python integers, and its last coefficient is 0; the unsatisfied instance satisfies the identity too, because c is a o b by
    construction.  Device tensors and host bytes give the same coefficients, in both forms."""
    size, num_inputs = 1 << k, 3
    n = size - num_inputs - slack
    r = nc.modulus(field)
    dom = domains(field, k)
    rng = random.Random((k << 8) | slack)
    for satisfied in (True, False):
        inst = sp.R1cs(field, n, n + 5, num_inputs, rng, satisfied=satisfied)
        a, b = inst.padded(size)
        with ea.SparseMatrix.from_rows(dom, inst.A, inst.nvars) as A, ea.SparseMatrix.from_rows(dom, inst.B, inst.nvars) as B, \
                ea.SparseMatrix.from_rows(dom, inst.C, inst.nvars) as C:
            z = dev(torch_, nc.encode(field, inst.z, False))
            h = dom.groth16_witness_map(A, B, z, num_inputs)
            assert h.is_cuda and tuple(h.shape) == (size, 32)
            hs = nc.decode(field, raw_of(h), False)
            tau = rng.randrange(2, r)
            left, right = sp.witness_identity(field, k, a, b, hs, tau)
            assert left == right, (field, k, slack, satisfied)
            assert hs[size - 1] == 0
            # the instance is what it says: C z agrees with a o b in every row, or misses one
            cz = nc.decode(field, raw_of(C.apply(z)), False)
            ab = [x * y % r for x, y in zip(inst.a, inst.b)]
            assert (cz == ab) == satisfied and sum(x != y for x, y in zip(cz, ab)) == (0 if satisfied else 1)
            # host bytes, and plain integers: the same coefficients
            assert raw_of(dom.groth16_witness_map(A, B, nc.encode(field, inst.z, False), num_inputs)) == raw_of(h)
            plain = dom.groth16_witness_map(A, B, dev(torch_, nc.encode(field, inst.z, True)), num_inputs, montgomery=False)
            assert nc.decode(field, raw_of(plain), True) == hs
    with ea.SparseMatrix.from_rows(dom, inst.A, inst.nvars) as A:
        with pytest.raises(ValueError, match="do not fit a domain"):
            dom.groth16_witness_map(A, A, z, size - n + 1)


# ---- speed -------------------------------------------------------------------------------------------------------------------------------

# Modelled without a run, against the forward NN transform of 2^20 elements on the same handle (16 products an element,
# DESIGN.md 4e; 0.2 ms in profiles/quotient.txt).  With 4 entries a row, per entry: by products 1 1/16 in the totals, 1 1/16 + 1/4 in the
# rows, 1/4 for z and about 0.3 for the prefix sum over the lanes: 2.9, against the transform's 16 / 4 an entry: a ratio of 0.73.  By
# bytes two passes over 32 (coefficient) + 4 (column) + a 64-byte sector for the 32-byte gather of z, and 8 + 16 + 6 for the rows, z and
# the lanes: 230 an entry, 0.96 GB, at the 2.8 TB/s the device-to-device copy reaches at such a footprint 0.34 ms: a ratio of 1.7.  The
# scheme has no term for row lengths, so the one number stands for both matrices.
MODEL_RATIO = 1.7


def speed_bound(which):
    """(bound on apply / forward transform, source): 1.5 x the ratio profiles/sparse.txt recorded, or 2 x the modelled ratio"""
    path = os.path.join(ROOT, "profiles", "sparse.txt")
    if os.path.exists(path):
        m = re.search(r"^bls12_381 ratio apply %s 2\^20 / forward NN 2\^20: ([0-9.]+)" % which, open(path).read(), flags=re.M)
        if m:
            return 1.5 * float(m.group(1)), "profiles/sparse.txt"
    return 2 * MODEL_RATIO, "the model"


def speed_matrices(rows, nnz, seed):
    """(name, row lengths) of the two matrices of the guard: 4 entries a row; and one row of nnz / 2, 2^10 rows of 2^10, the rest spread
    evenly over the other rows, in a seeded order"""
    rng = np.random.default_rng(seed)
    uniform = np.full(rows, nnz // rows, dtype=np.int64)
    left = nnz - nnz // 2 - (1 << 20)
    others = rows - 1 - (1 << 10)
    rest = np.full(others, left // others, dtype=np.int64)
    rest[:left - int(rest.sum())] += 1
    skewed = np.concatenate([[nnz // 2], np.full(1 << 10, 1 << 10, dtype=np.int64), rest])
    rng.shuffle(skewed)
    assert uniform.sum() == nnz and skewed.sum() == nnz
    return ("uniform", uniform), ("skewed", skewed)


def test_speed_guard_against_the_transform(domains, torch_):
    """BLS12-381, rows = cols = 2^20, nnz = 2^22, device-resident random bytes, warmed up, median of 5: apply on a uniform and on a
    skewed matrix of the same nnz, each against the forward NN transform of 2^20 on the same handle, which this change does not touch,
    run in the same test on the same box.  Bound: 1.5 x the ratio profiles/sparse.txt recorded (tools/sparse_bench.py; the margin
    covers box-to-box spread and clock differences under the power limit), or 2 x the modelled ratio above without that
    file."""
    torch = torch_
    rows = cols = 1 << 20
    nnz = 1 << 22
    dom = domains("bls12_381", 20)
    g = torch.Generator(device="cuda")
    g.manual_seed(0x5EED)
    z = torch.randint(0, 256, (cols, 32), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((rows, 32), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(0x5BA25E)
    values = rng.integers(0, 256, size=(nnz, 32), dtype=np.uint8)
    col_idx = rng.integers(0, cols, size=nnz, dtype=np.uint32)

    def median5(fn):
        fn()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    t_ntt = median5(lambda: dom.fft(z, out=out))
    for which, lens in speed_matrices(rows, nnz, 0xD15C):
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        with dom.sparse_matrix(rows, cols, row_ptr, col_idx, values) as M:
            t = median5(lambda: M.apply(z, out=out))
        bound, source = speed_bound(which)
        print("apply %s: %.3f ms, forward NN 2^20 %.3f ms, ratio %.4f, bound %.4f from %s" % (which, 1e3 * t, 1e3 * t_ntt, t / t_ntt, bound, source))
        assert t / t_ntt <= bound, which
