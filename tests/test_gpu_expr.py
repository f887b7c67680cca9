"""GPU: compiled custom-gate expressions (ea.Expr, dom.compile_expression, ea.GateProgram) on both fields.  Parity with the big-integer
evaluator of tests/expr_cases.py at len = 1, 63, 64, 65, 1000 and 4096, every output compared: random DAGs, the chains that force
reductions, the program at the slot limit, a program of more than 10 000 instructions, 64 columns, rotations that wrap at both ends with
rot_step 8, periodic columns, edge-value inputs.  The oracle the project already trusts: the Jellyfish quotient row written as an Expr
equals dom.plonk_quotient byte for byte.  The contract: a late producer on a side stream, host pointers equal device pointers, out as a
column, len 0, one program with two sets of challenges, two programs on one domain, and what only a program can refuse."""
import ctypes
import random

import numpy as np
import pytest

import expr_cases as xc
import ntt_cases as nc
import poly_cases as pc
import quotient_cases as qc
import stream_cases as st

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
    """one domain per (field, size) for the whole module: a program takes its field and device from it, not its size"""
    made = {}

    def get(field, k=4):
        if (field, k) not in made:
            made[(field, k)] = ea.Radix2EvaluationDomain(1 << k, CURVE_OF[field])
        return made[(field, k)]

    yield get
    for d in made.values():
        d.close()


def dev(torch, raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda().reshape(-1, 32)


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else (t.tobytes() if hasattr(t, "tobytes") else bytes(t))


class RawProgram:
    """a program from the flat nodes of a case (the C ABI: the Python builder is tested on its own)"""

    def __init__(self, ea, dom, case, field):
        self.lib, self.dom, self.case, self.field = dom._lib, dom, case, field
        self.handle = ctypes.c_void_p()
        flat = (ctypes.c_uint32 * (3 * len(case.nodes)))(*case.flat())
        cb = b"".join((v % dom.modulus).to_bytes(32, "little") for v in case.consts)
        self.err = self.lib.mi355_msm_expr_create(ctypes.byref(self.handle), dom.handle, flat, len(case.nodes), cb or None, len(case.consts), case.n_chal,
                                                  case.n_cols, 1)

    def run(self, torch, cols, chals, length, normal, device=True, out=None):
        keep = [dev(torch, c) if device else np.frombuffer(c, dtype=np.uint8).copy() for c in cols]
        ptr = (lambda t: t.data_ptr()) if device else (lambda a: a.ctypes.data)
        if out is None:
            out = torch.full((max(length, 1), 32), 0xA5, dtype=torch.uint8, device="cuda") if device else np.full(max(length, 1) * 32, 0xA5, dtype=np.uint8)
        n = len(keep)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ptr(k) for k in keep])
        lens = (ctypes.c_size_t * max(n, 1))(*[len(c) // 32 for c in cols])
        cb = nc.encode(self.field, list(chals), normal)
        err = self.lib.mi355_msm_expr_run(self.handle, ptr(out), ptrs, lens, n, length, self.case.rot_step, cb or None, len(chals),
                                          (1 if normal else 0) | (2 if device else 0), torch.cuda.current_stream().cuda_stream if device else None)
        return err, out

    def query(self, key):
        v = ctypes.c_uint64()
        assert self.lib.mi355_msm_expr_query(self.handle, key.encode(), ctypes.byref(v)).code == 0
        return int(v.value)

    def close(self):
        if self.handle:
            assert self.lib.mi355_msm_expr_destroy(self.handle).code == 0
            self.handle = ctypes.c_void_p()


def message(err):
    msg = ctypes.string_at(err.message).decode() if err.message else ""
    if err.message:
        ctypes.CDLL(None).free(ctypes.c_void_p(err.message))
    return msg


def parity(ea, torch, dom, field, case, lengths, normals=(0, 1), device=True):
    prog = RawProgram(ea, dom, case, field)
    assert prog.err.code == 0, message(prog.err)
    try:
        for normal in normals:
            for length in lengths:
                raws, chals, want = xc.inputs(case, field, length, normal)
                err, out = prog.run(torch, raws, chals, length, normal, device)
                assert err.code == 0, message(err)
                got = raw_of(out)[:length * 32]
                if got != want:
                    bad = [i for i in range(length) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]]
                    raise AssertionError((case.name, field, normal, length, "rows", bad[:8], len(bad)))
        return {k: prog.query(k) for k in ("nodes", "instructions", "slots", "products", "reduces", "columns", "lds_bytes")}
    finally:
        prog.close()


@pytest.mark.parametrize("case", xc.dags(), ids=lambda c: c.name)
@pytest.mark.parametrize("field", FIELDS)
def test_random_dags(ea, domains, torch_, field, case):
    parity(ea, torch_, domains(field), field, case, xc.LENS)


@pytest.mark.parametrize("case", xc.chains(), ids=lambda c: c.name)
@pytest.mark.parametrize("field", FIELDS)
def test_forced_reduction_chains(ea, domains, torch_, field, case):
    info = parity(ea, torch_, domains(field), field, case, xc.LENS)
    if not case.name.startswith("add_chain") or field == "bls12_381":
        assert info["reduces"] > 0, info


@pytest.mark.parametrize("field", FIELDS)
def test_program_at_the_slot_limit_and_one_above(ea, domains, torch_, field):
    info = parity(ea, torch_, domains(field), field, xc.slot_program(xc.MAX_SLOTS - 1), xc.LENS, normals=(0,))
    assert info["slots"] == xc.MAX_SLOTS and info["lds_bytes"] == xc.MAX_SLOTS * 8 * 4 * 64
    over = RawProgram(ea, domains(field), xc.slot_program(xc.MAX_SLOTS), field)
    msg = message(over.err)
    assert over.err.code == -1 and not over.handle and "S = %d" % (xc.MAX_SLOTS + 1) in msg and "limit is %d" % xc.MAX_SLOTS in msg, msg


@pytest.mark.parametrize("field", FIELDS)
def test_more_than_10000_instructions(ea, domains, torch_, field):
    info = parity(ea, torch_, domains(field), field, xc.long_program(3400), xc.LENS, normals=(0,))
    assert info["instructions"] > 10000 and info["nodes"] > 20000


@pytest.mark.parametrize("field", FIELDS)
def test_64_columns(ea, domains, torch_, field):
    info = parity(ea, torch_, domains(field), field, xc.wide_program(64), xc.LENS, normals=(0,))
    assert info["columns"] == 64


@pytest.mark.parametrize("field", FIELDS)
def test_rotations_periodic_columns_and_edge_values(ea, domains, torch_, field):
    dom = domains(field)
    parity(ea, torch_, dom, field, xc.rotation_program(8), xc.LENS)          # rotations +-1, +-3 times 8: every length wraps at both ends
    parity(ea, torch_, dom, field, xc.periodic_program((1, 8)), xc.LENS)     # a scalar and a column of period 8 (1 where 8 does not divide)
    parity(ea, torch_, dom, field, xc.edge_program(), xc.LENS)
    parity(ea, torch_, dom, field, xc.sqr_tower(24), (65, 1000), normals=(0,))
    parity(ea, torch_, dom, field, xc.single_leaf(), (1, 65), normals=(1,))


# ---- the oracle the project already trusts --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,n,m,selectors", [(8, 32, 5, True), (8, 32, 3, False), (6, 32, 5, True), (6, 32, 3, False)])
@pytest.mark.parametrize("field", FIELDS)
def test_jellyfish_quotient_row_equals_plonk_quotient(ea, domains, torch_, field, K, n, m, selectors):
    torch = torch_
    r = nc.modulus(field)
    c = qc.Rows(field, K, n, m, 0xE9 + K + m, selectors=selectors)
    M, ratio = c.M, c.M // n
    dom = domains(field, K)
    g, om = nc.generator(field), nc.root_of_unity(field, K)
    xs = [g * pow(om, i, r) % r for i in range(M)]
    zh_inv = [pow((pow(xs[i], n, r) - 1) % r, -1, r) for i in range(ratio)]
    l1_den = [pow(n * (x - 1) % r, -1, r) for x in xs]
    t = lambda raw: dev(torch, pc.to_raw(raw))
    e = lambda vals: dev(torch, nc.encode(field, vals, False))
    wires, sigmas, z, pi = [t(w) for w in c.wires], [t(s) for s in c.sigmas], t(c.raw_z(False)), t(c.pi)
    sel = [t(q) for q in c.selectors] if selectors else None
    want = dom.plonk_quotient(wires, sigmas, z, c.alpha, c.beta, c.gamma, c.ks, n, selectors=sel, pi=pi)
    at = xc.jellyfish_columns(m, selectors)
    cols = wires + sigmas + [z, pi, e(xs), e(zh_inv), e(l1_den)] + (sel or [])
    assert len(cols) == at["ncols"] and zh_inv and len(zh_inv) == ratio
    with dom.compile_expression(xc.jellyfish_expr(ea, m, selectors, c.ks), at["ncols"]) as prog:
        got = prog.run(cols, challenges=(c.alpha, c.beta, c.gamma), rot_step=ratio)
        assert got.is_cuda and raw_of(got) == raw_of(want)
        assert prog.query("slots") <= 8 and prog.query("columns") == at["ncols"]
        print(field, K, m, selectors, {k: prog.query(k) for k in ("nodes", "instructions", "slots", "products", "reduces")})
    assert raw_of(want) == nc.encode(field, c.model(False), False)


# ---- the contract ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def side(torch_):
    stream = torch_.cuda.Stream(priority=-1)
    return stream, st.Delay(torch_, stream)


@pytest.mark.parametrize("field", FIELDS)
def test_run_after_a_late_producer_on_a_side_stream(ea, domains, torch_, side, field):
    """device pointers on a non-default stream, the columns produced on that stream by a producer that takes its time, out= poisoned by it"""
    torch = torch_
    stream, delay = side
    case, length = xc.rotation_program(8), 1000
    raws, chals, want = xc.inputs(case, field, length, 0)
    E = ea.Expr
    expr = None
    for rot in (1, -1, 3, -3, 0):
        term = E.col(0, rot) * E.col(1, -rot)
        expr = term if expr is None else expr + term
    with domains(field).compile_expression(expr, 2) as prog:
        outs = [st.poisoned(torch, (length, 32))]
        views = st.late_many(torch, raws, stream, delay, fill=outs)
        ins = []
        for v in views:
            t = v.reshape(length, 32)
            t.started, t.produced = v.started, v.produced
            ins.append(t)
        made = ins + outs
        with torch.cuda.stream(stream):
            assert all(st.window_open(t.produced) for t in made), "invalid: a producer had finished before the call was made"
            got = prog.run(ins, rot_step=8, out=outs[0])
        stream.synchronize()
        assert st.closed(*made), "invalid: a producer took %s ms" % [st.delay_ms(t) for t in made]
        assert got.data_ptr() == outs[0].data_ptr() and raw_of(got) == want


@pytest.mark.parametrize("field", FIELDS)
def test_host_pointers_equal_device_pointers(ea, domains, torch_, field):
    for case in (xc.random_dag(15, 150), xc.periodic_program((1, 8)), xc.edge_program()):
        parity(ea, torch_, domains(field), field, case, (1, 65, 1000), device=False)
    # the Python layer: bytes in, bytes out; NumPy in, NumPy out
    case, length = xc.periodic_program((1, 8)), 64
    raws, chals, want = xc.inputs(case, field, length, 1)
    E = ea.Expr
    expr = E.col(0)
    for j in (1, 2):
        expr = expr * E.col(j, 1) - E.col(j)
    with domains(field).compile_expression(expr, 3) as prog:
        assert prog.run(raws, montgomery=False) == want
        got = prog.run([np.frombuffer(c, dtype=np.uint8).reshape(-1, 32) for c in raws], montgomery=False)
        assert isinstance(got, np.ndarray) and got.shape == (length, 32) and got.tobytes() == want


@pytest.mark.parametrize("field", FIELDS)
def test_out_as_a_column_len_0_challenges_and_two_programs(ea, domains, torch_, field):
    torch = torch_
    dom = domains(field)
    r = nc.modulus(field)
    E = ea.Expr
    length = 1000
    rng = random.Random(0x0C7)
    a, b = ([rng.randrange(r) for _ in range(length)] for _ in range(2))
    ta, tb = dev(torch, nc.encode(field, a, False)), dev(torch, nc.encode(field, b, False))
    p0 = dom.compile_expression(E.col(0) * E.challenge(0) + E.col(1, 1) * E.challenge(1), 2)      # column 0 at rotation 0 only
    p1 = dom.compile_expression(E.col(0, 1) - E.col(0) * E.col(1) ** 3 + 7, 2)                     # column 0 at rotations 0 and 1
    with p0, p1:
        # the same program twice with different challenges; another program on the same domain between them
        for ch in ((3, 5), (r - 1, rng.randrange(r))):
            want = [(a[i] * ch[0] + b[(i + 1) % length] * ch[1]) % r for i in range(length)]
            assert raw_of(p0.run([ta, tb], challenges=ch)) == nc.encode(field, want, False)
            want1 = [(a[(i + 1) % length] - a[i] * pow(b[i], 3, r) + 7) % r for i in range(length)]
            assert raw_of(p1.run([ta, tb])) == nc.encode(field, want1, False)
        # out IS column 0, read at rotation 0 only: in place
        keep = ta.clone()
        want = [(a[i] * 3 + b[(i + 1) % length] * 5) % r for i in range(length)]
        got = p0.run([keep, tb], challenges=(3, 5), out=keep)
        assert got.data_ptr() == keep.data_ptr() and raw_of(keep) == nc.encode(field, want, False)
        # out is column 1 (read at rotation 1), or column 0 of the other program (rotations 0 and 1): refused, nothing written
        for prog, cols, which, ch in ((p0, [ta, tb], 1, (3, 5)), (p1, [ta, tb], 0, ())):
            before = raw_of(cols[which])
            with pytest.raises(ea.MsmError) as ei:
                prog.run(cols, challenges=ch, out=cols[which])
            assert ei.value.code == -1 and "rotation other than 0" in ei.value.message and raw_of(cols[which]) == before
        # an overlap in part
        big = torch.zeros((length + 8, 32), dtype=torch.uint8, device="cuda")
        with pytest.raises(ea.MsmError) as ei:
            p0.run([big[:length], tb], challenges=(3, 5), out=big[8:])
        assert "overlaps column 0" in ei.value.message
        # what only the program can judge: the counts it was created with
        lib = dom._lib
        ptrs = (ctypes.c_void_p * 2)(ta.data_ptr(), tb.data_ptr())
        lens = (ctypes.c_size_t * 2)(length, length)
        out = torch.empty((length, 32), dtype=torch.uint8, device="cuda")
        b64 = bytes(64)
        assert "1 columns, the program was created with 2" in message(lib.mi355_msm_expr_run(p0.handle, out.data_ptr(), ptrs, lens, 1, length, 1, b64, 2, 2, None))
        assert "1 challenges, the program was created with 2" in message(lib.mi355_msm_expr_run(p0.handle, out.data_ptr(), ptrs, lens, 2, length, 1, b64, 1, 2, None))
        # len = 0 succeeds and writes nothing
        lens0 = (ctypes.c_size_t * 2)(1, 1)
        out.fill_(0x77)
        err = lib.mi355_msm_expr_run(p0.handle, out.data_ptr(), ptrs, lens0, 2, 0, 1, b64, 2, 2, None)
        assert err.code == 0 and bool((out == 0x77).all())
        assert p0.query("last_device_us") >= 0 and p0.query("products") == 2 + 2 + 1 and p0.query("slots") <= 1
