"""GPU: resident lookup tables over Fr (ea.LookupTable: multiplicities, index, plookup's sorted vector) and the logUp running sum
(dom.logup_sum) against the integer model of tests/lookup_cases.py, byte for byte, on both fields and in both forms: the shapes at the
slot-sizing and block edges, duplicates, residues above r, missing values (sorted then writes nothing), skewed columns, 2^20 values
against numpy.unique, determinism, host pointers against device pointers, and the stream order of flag bit 1, pinned with late producers
as tests/test_gpu_mle.py pins it, one test each for create, count, sorted and logup_sum."""
import random

import numpy as np
import pytest

import lookup_cases as lc
import ntt_cases as nc
import stream_cases as st

pytestmark = pytest.mark.gpu

FIELDS = ("bls12_377", "bls12_381")
CURVE_OF = {"bls12_377": "bls12_377_g1", "bls12_381": "bls12_381_g1"}
PATTERN = 0xA5


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def domains(ea):
    """one (small) domain per field for the whole module: a table takes its field, device and stream from it, not its size"""
    made = {}

    def get(field, tile_log=0):
        if field not in made:
            made[field] = ea.Radix2EvaluationDomain(1 << 4, CURVE_OF[field])
        made[field].set_option("poly_tile_log", tile_log)
        return made[field]

    yield get
    for d in made.values():
        d.close()


def dev(torch, raw):
    return torch.frombuffer(bytearray(raw) if len(raw) else bytearray(32), dtype=torch.uint8).cuda().reshape(-1, 32)[:len(raw) // 32]


def raw_of(t):
    return t.cpu().numpy().tobytes() if hasattr(t, "cpu") else (t.tobytes() if hasattr(t, "tobytes") else bytes(t))


def index_of(idx):
    return (idx.cpu().numpy() if hasattr(idx, "cpu") else np.asarray(idx)).view(np.uint32).tolist()


def run_case(ea, torch, dom, c, device=True):
    """every output of one case: (mult, index, missing, first, s or None when sorted refused, the pattern-filled out tensor)"""
    wrap = (lambda raw: dev(torch, raw)) if device else (lambda raw: raw)
    with ea.LookupTable(dom, wrap(c.table_raw), montgomery=not c.normal) as lt:
        values = wrap(c.values_raw)
        mult, missing, first, idx = lt.multiplicities(values, index=True)
        out = torch.full((c.n_t + c.n_f, 32), PATTERN, dtype=torch.uint8, device="cuda") if device else None
        try:
            s = lt.sorted(values, out=out) if device else lt.sorted(values)
        except ea.MsmError as e:
            assert "first_missing = %d" % first in str(e)
            s = None
        assert lt.query("n") == c.n_t and lt.query("max_probe") >= 1 and lt.query("table_bytes") >= c.n_t * 32 + 4 * lt.query("slots")
        info = (lt.query("slots"), lt.query("distinct"))
    return raw_of(mult), index_of(idx), missing, first, None if s is None else raw_of(s), out, info


def check(got, c):
    mult, index, missing, first, s, out, info = got
    want = c.expected
    assert index == want["index"], c.name
    assert mult == want["mult"], c.name
    assert (missing, first) == (want["missing"], want["first"]), c.name
    if want["sorted"] is None:
        assert s is None, c.name
        if out is not None:
            assert raw_of(out) == bytes([PATTERN]) * ((c.n_t + c.n_f) * 32), c.name    # nothing was written
    else:
        assert s == want["sorted"], c.name
    slots = 2
    while slots < 2 * c.n_t:
        slots *= 2
    assert info == (slots, len(set(lc.model_count(c.field, c.table_raw, c.table_raw)[0]))), c.name


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_every_case_against_the_model(ea, domains, torch_, field, normal):
    dom = domains(field)
    for c in lc.cases(field, normal).values():
        check(run_case(ea, torch_, dom, c), c)


@pytest.mark.parametrize("field", FIELDS)
def test_host_pointers_equal_device_pointers(ea, domains, torch_, field):
    dom = domains(field)
    cs = lc.cases(field, 0)
    for name in ("nt1_nf0", "nt1_nf65", "nt33", "dup_scattered", "missing_many", "table_v_values_v_plus_r", "skew_half_padding"):
        host, device = run_case(ea, torch_, dom, cs[name], device=False), run_case(ea, torch_, dom, cs[name])
        check(host, cs[name])
        assert host[:5] == device[:5] and host[6] == device[6], name


@pytest.mark.parametrize("field", FIELDS)
def test_a_call_in_the_other_form_is_refused(ea, domains, torch_, field):
    c = lc.cases(field, 0)["nt32"]
    with ea.LookupTable(domains(field), c.table_raw, montgomery=True) as lt:
        lt._flags = 1
        with pytest.raises(ea.MsmError, match="flag bit 0"):
            lt.multiplicities(c.values_raw)
        with pytest.raises(ea.MsmError, match="flag bit 0"):
            lt.sorted(dev(torch_, c.values_raw))
        lt._flags = 0
        assert lt.multiplicities(c.values_raw)[1] == 0


@pytest.mark.parametrize("field", FIELDS)
def test_medium_against_numpy_unique(ea, domains, torch_, field):
    """2^20 uniform values into 2^16 entries: the counts of numpy.unique over the canonical rows, the index, and s as a repeat"""
    torch = torch_
    table, values, pick = lc.medium_case(field, 0)
    with ea.LookupTable(domains(field), torch.from_numpy(table.view(np.uint8)).cuda()) as lt:
        v = torch.from_numpy(values.view(np.uint8)).cuda()
        mult, missing, first, idx = lt.multiplicities(v, index=True)
        s = lt.sorted(v)
        assert lt.query("distinct") == 1 << 16 and lt.query("slots") == 1 << 17 and lt.query("max_probe") <= (1 << 16) // 16
    uniq, counts = np.unique(values, axis=0, return_counts=True)
    want = np.zeros(1 << 16, dtype=np.int64)
    order = {row.tobytes(): i for i, row in enumerate(table)}
    for row, c in zip(uniq, counts):
        want[order[row.tobytes()]] = c
    assert (missing, first) == (0, 1 << 20) and index_of(idx) == pick.tolist()
    assert raw_of(mult) == nc.encode(field, want.tolist(), False)
    assert np.array_equal(s.cpu().numpy().view(np.uint32).reshape(-1, 8), np.repeat(table, 1 + want, axis=0))


@pytest.mark.parametrize("field", FIELDS)
def test_every_output_byte_is_a_function_of_the_inputs(ea, domains, torch_, field):
    """atomics are used, yet the same calls twice and a handle built twice give identical bytes, index_out included"""
    dom = domains(field)
    cs = lc.cases(field, 1)
    for name in ("dup_1000_equal", "dup_scattered", "block_edges", "skew_half_padding", "missing_many"):
        c = cs[name]
        seen = []
        for _ in range(2):
            with ea.LookupTable(dom, dev(torch_, c.table_raw), montgomery=False) as lt:
                v = dev(torch_, c.values_raw)
                for _ in range(2):
                    mult, missing, first, idx = lt.multiplicities(v, index=True)
                    s = raw_of(lt.sorted(v)) if missing == 0 else None
                    seen.append((raw_of(mult), index_of(idx), missing, first, s))
        assert all(x == seen[0] for x in seen), name


# ---- the logUp running sum ----------------------------------------------------------------------------------------------------------------

def logup(dom, torch, case, m, stride, n, normal, helpers, device=True):
    wrap = (lambda raw: dev(torch, raw)) if device else (lambda raw: np.frombuffer(raw, dtype=np.uint8).reshape(-1, 32))
    vals = wrap(case["values"])
    if m > 1 or stride != n:
        if device:
            pad = torch.zeros((m * stride, 32), dtype=torch.uint8, device="cuda")
            pad[:vals.shape[0]] = vals
        else:
            pad = np.zeros((m * stride, 32), dtype=np.uint8)
            pad[:vals.shape[0]] = vals
        vals = pad.reshape(m, stride, 32)
    got = dom.logup_sum(wrap(case["table"]), wrap(case["mult"]), vals, nc.decode(case["field"], case["beta"], normal)[0],
                        helpers=helpers, montgomery=not normal)
    return (raw_of(got[0]), got[1]) + ((raw_of(got[2]),) if helpers else ())


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_logup_against_the_model(domains, torch_, field, normal):
    for n in (1, 8, 1025):
        for m in (1, 8):
            stride = n + 3 if m == 8 else n
            case = dict(lc.logup_case(field, normal, n, m, stride, 1), field=field)
            want = lc.model_logup(field, case["table"], case["mult"], case["values"], m, stride, n, case["beta"], normal)
            wtotal = nc.decode(field, want[1], normal)[0]
            assert wtotal == 0
            for tile_log in (4, 0):
                dom = domains(field, tile_log)
                assert logup(dom, torch_, case, m, stride, n, normal, True) == (want[0], wtotal, want[2]), (n, m, tile_log)
            assert logup(dom, torch_, case, m, stride, n, normal, False) == (want[0], wtotal)
            assert logup(dom, torch_, case, m, stride, n, normal, True, device=False) == (want[0], wtotal, want[2])
            counts = list(case["counts"])
            counts[0] += 1
            off = dict(case, mult=nc.encode(field, counts, normal))
            got = logup(dom, torch_, off, m, stride, n, normal, False)
            wt = nc.decode(field, lc.model_logup(field, off["table"], off["mult"], off["values"], m, stride, n, off["beta"], normal)[1], normal)[0]
            assert got[1] == wt != 0
    assert dom.query("logup_work_bytes") > 0
    # a zero denominator (beta = -table[3]) contributes 0 and is no error
    case = dict(lc.logup_case(field, normal, 8, 2, 8, 2, zero_den=True), field=field)
    want = lc.model_logup(field, case["table"], case["mult"], case["values"], 2, 8, 8, case["beta"], normal)
    assert want[2][(2 * 8 + 3) * 32:(2 * 8 + 4) * 32] == bytes(32)
    assert logup(dom, torch_, case, 2, 8, 8, normal, True) == (want[0], nc.decode(field, want[1], normal)[0], want[2])


@pytest.mark.parametrize("normal", [0, 1])
@pytest.mark.parametrize("field", FIELDS)
def test_end_to_end_total_is_zero_from_the_librarys_multiplicities(ea, domains, torch_, field, normal):
    """LookupTable -> multiplicities -> logup_sum, all in device memory"""
    dom = domains(field)
    rng = random.Random(21)
    n = 3000
    t = lc.distinct_small(n, 100, rng)
    f = [t[rng.randrange(40)] if rng.randrange(2) else t[rng.randrange(n)] for _ in range(n)]
    traw, fraw = dev(torch_, nc.encode(field, t, normal)), dev(torch_, nc.encode(field, f, normal))
    with ea.LookupTable(dom, traw, montgomery=not normal) as lt:
        mult, missing, _ = lt.multiplicities(fraw)
    assert missing == 0
    beta = rng.randrange(nc.modulus(field))
    phi, total = dom.logup_sum(traw, mult, fraw, beta, montgomery=not normal)
    assert total == 0 and raw_of(phi[:1]) == bytes(32)
    mult[7, 0] ^= 1                                   # one multiplicity changed by one (in either form the element changes)
    assert dom.logup_sum(traw, mult, fraw, beta, montgomery=not normal)[1] != 0


def test_logup_out_overlapping_an_input_is_refused(ea, domains, torch_):
    dom = domains("bls12_381")
    n = 64
    buf = torch_.zeros((3 * n, 32), dtype=torch_.uint8, device="cuda")
    table, mult, values = buf[:n], buf[n:2 * n], buf[2 * n:]
    for out in (table, mult, values, buf[n // 2:n // 2 + n]):
        with pytest.raises(ea.MsmError, match="overlaps"):
            dom.logup_sum(table, mult, values, 5, out=out)


# ---- the stream order of flag bit 1 ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def side(torch_):
    """(stream, calibrated delay) for the late producers of this module, once; from torch's high-priority pool, for the reason
    tests/test_gpu_mle.py gives"""
    stream = torch_.cuda.Stream(priority=-1)
    return stream, st.Delay(torch_, stream)


def _late_call(torch, stream, delay, raws, shapes, out_shapes, call):
    """inputs and out= tensors behind ONE late producer on a side stream, which fills the outputs with OUT_POISON before it hands over
    the inputs: the window is open immediately before the call and the producer took its time; returns what `call(inputs, outs)` returned"""
    outs = [st.poisoned(torch, s) for s in out_shapes]
    views = st.late_many(torch, raws, stream, delay, fill=outs)
    ins = []
    for v, shape in zip(views, shapes):
        t = v.reshape(shape)
        t.started, t.produced = v.started, v.produced
        ins.append(t)
    made = ins + outs
    with torch.cuda.stream(stream):
        assert all(st.window_open(t.produced) for t in made), "invalid: a producer had finished before the call was made"
        got = call(ins, outs)
    stream.synchronize()
    assert st.closed(*made), "invalid: a producer took %s ms" % [st.delay_ms(t) for t in made]
    return got


@pytest.mark.parametrize("field", FIELDS)
def test_create_after_a_late_producer_on_a_side_stream(ea, domains, torch_, side, field):
    c = lc.cases(field, 0)["dup_scattered"]
    stream, delay = side
    lt = _late_call(torch_, stream, delay, [c.table_raw], [(c.n_t, 32)], [], lambda ins, outs: ea.LookupTable(domains(field), ins[0]))
    with lt:
        mult, missing, first, idx = lt.multiplicities(dev(torch_, c.values_raw), index=True)
        assert (raw_of(mult), index_of(idx), missing, first) == (c.expected["mult"], c.expected["index"], 0, c.n_f)


@pytest.mark.parametrize("field", FIELDS)
def test_count_after_a_late_producer_on_a_side_stream(ea, domains, torch_, side, field):
    c = lc.cases(field, 0)["missing_many"]
    stream, delay = side
    with ea.LookupTable(domains(field), dev(torch_, c.table_raw)) as lt:
        mult, missing, first, idx = _late_call(torch_, stream, delay, [c.values_raw], [(c.n_f, 32)], [], lambda ins, outs: lt.multiplicities(ins[0], index=True))
    assert (raw_of(mult), index_of(idx), missing, first) == (c.expected["mult"], c.expected["index"], c.expected["missing"], c.expected["first"])


@pytest.mark.parametrize("field", FIELDS)
def test_sorted_after_a_late_producer_on_a_side_stream(ea, domains, torch_, side, field):
    c = lc.cases(field, 0)["dup_scattered"]
    stream, delay = side
    with ea.LookupTable(domains(field), dev(torch_, c.table_raw)) as lt:
        s = _late_call(torch_, stream, delay, [c.values_raw], [(c.n_f, 32)], [(c.n_t + c.n_f, 32)], lambda ins, outs: lt.sorted(ins[0], out=outs[0]))
    assert raw_of(s) == c.expected["sorted"]


@pytest.mark.parametrize("field", FIELDS)
def test_logup_sum_after_late_producers_on_a_side_stream(domains, torch_, side, field):
    n, m = 300, 2
    case = lc.logup_case(field, 0, n, m, n, 4)
    want = lc.model_logup(field, case["table"], case["mult"], case["values"], m, n, n, case["beta"], 0)
    beta = nc.decode(field, case["beta"], 0)[0]
    stream, delay = side
    phi, total = _late_call(torch_, stream, delay, [case["table"], case["mult"], case["values"]], [(n, 32), (n, 32), (m, n, 32)], [(n, 32)],
                            lambda ins, outs: domains(field).logup_sum(ins[0], ins[1], ins[2], beta, out=outs[0]))
    assert raw_of(phi) == want[0] and total == 0
