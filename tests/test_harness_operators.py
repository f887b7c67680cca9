"""include/mi355_msm.hpp EXECUTED, class by class: tests/harness_operators.cpp calls every wrapper of the header on the GPU, one process
per family and field, and every file it writes must equal, byte for byte, what the integer models give (tests/operator_cases.py).  The
header is the last layer in front of kernels that have their own tests, so the shapes are chosen for its marshalling: flags, strides,
lengths, output sizes, and the refusals of the wrappers and of the C ABI behind them.

Without a GPU: the program builds without a warning, every C entry point the header calls is reached by this harness or by
harness_msm_correctness.cpp (adding a wrapper without a case fails here), and every family's first constructor throws mi355::MsmError
with the no-device code."""
import os
import re
import subprocess

import pytest

import operator_cases as oc
from conftest import ROOT

PKG = os.path.join(ROOT, "2022-entries_amd")
SRC = os.path.join(ROOT, "tests", "harness_operators.cpp")
HPP = os.path.join(ROOT, "include", "mi355_msm.hpp")
EXE = os.path.join(ROOT, "tests", "harness_operators.bin")
LIMIT = 120      # seconds a process may take; one takes a few, most of it the start of the runtime

# C entry point -> (family of harness_operators.cpp, the `ran` line that proves a wrapper calling it returned)
ENTRY_POINTS = {
    "mi355_msm_create": ("points", "multi_scalar_mult_init"),
    "mi355_msm_set_bases": ("points", "multi_scalar_mult_init"),
    "mi355_msm_destroy": ("points", "multi_scalar_mult_init"),
    "mi355_msm_run": ("points", "multi_scalar_mult"),
    "mi355_msm_run_async": ("points", "multi_scalar_mult_async"),
    "mi355_msm_job_wait": ("points", "MsmJob::wait"),
    "mi355_msm_job_done": ("points", "MsmJob::done"),
    "mi355_msm_check_bases": ("points", "check_bases"),
    "mi355_msm_check_bases_device": ("points", "check_bases_device"),
    "mi355_msm_decompress_points": ("points", "decompress_points"),
    "mi355_msm_compress_points": ("points", "compress_points"),
    "mi355_msm_mul_points": ("points", "mul_points"),
    "mi355_msm_set_bases_compressed": ("points", "set_bases_compressed"),
    "mi355_msm_set_option": ("points", "msm_chunks"),
    "mi355_msm_fold": ("points", "msm_chunks"),
    "mi355_msm_fft_points": ("points", "fft_points"),
    "mi355_msm_fixed_create": ("fixed", "get_window_table"),
    "mi355_msm_fixed_destroy": ("fixed", "get_window_table"),
    "mi355_msm_fixed_query": ("fixed", "WindowTable::query"),
    "mi355_msm_fixed_window_size": ("fixed", "get_mul_window_size"),
    "mi355_msm_fixed_mul": ("fixed", "msm"),
    "mi355_msm_domain_create": ("transforms", "Radix2EvaluationDomain"),
    "mi355_msm_domain_destroy": ("transforms", "Radix2EvaluationDomain"),
    "mi355_msm_domain_query": ("transforms", "query"),
    "mi355_msm_domain_element": ("transforms", "element"),
    "mi355_msm_domain_transform": ("transforms", "fft"),
    "mi355_msm_domain_mul": ("vecops", "mul"),
    "mi355_msm_domain_vec_op": ("vecops", "add"),
    "mi355_msm_domain_batch_inverse": ("vecops", "batch_inversion_and_mul"),
    "mi355_msm_domain_linear_combination": ("vecops", "linear_combination"),
    "mi355_msm_domain_evaluate": ("polys", "evaluate"),
    "mi355_msm_domain_divide_by_linear": ("polys", "divide_by_linear"),
    "mi355_msm_domain_lagrange": ("polys", "evaluate_all_lagrange_coefficients"),
    "mi355_msm_domain_vanishing": ("polys", "evaluate_vanishing_polynomial"),
    "mi355_msm_domain_divide_by_vanishing_on_coset": ("polys", "divide_by_vanishing_poly_on_coset"),
    "mi355_msm_domain_scan": ("scans", "scan"),
    "mi355_msm_domain_permutation_product": ("scans", "permutation_product"),
    "mi355_msm_domain_plonk_quotient": ("quotient", "plonk_quotient"),
    "mi355_msm_sparse_create": ("sparse", "SparseMatrix"),
    "mi355_msm_sparse_destroy": ("sparse", "SparseMatrix"),
    "mi355_msm_sparse_query": ("sparse", "SparseMatrix::query"),
    "mi355_msm_sparse_apply": ("sparse", "apply"),
    "mi355_msm_lookup_create": ("lookup", "LookupTable"),
    "mi355_msm_lookup_destroy": ("lookup", "LookupTable"),
    "mi355_msm_lookup_query": ("lookup", "LookupTable::query"),
    "mi355_msm_lookup_count": ("lookup", "multiplicities"),
    "mi355_msm_lookup_sorted": ("lookup", "sorted"),
    "mi355_msm_domain_logup_sum": ("lookup", "logup_sum"),
    "mi355_msm_expr_create": ("expr", "GateProgram"),
    "mi355_msm_expr_destroy": ("expr", "GateProgram"),
    "mi355_msm_expr_query": ("expr", "GateProgram::query"),
    "mi355_msm_expr_run": ("expr", "run"),
    "mi355_msm_poseidon_create": ("poseidon", "Poseidon"),
    "mi355_msm_poseidon_destroy": ("poseidon", "Poseidon"),
    "mi355_msm_poseidon_query": ("poseidon", "Poseidon::query"),
    "mi355_msm_poseidon_hash": ("poseidon", "hash"),
    "mi355_msm_poseidon_merkle": ("poseidon", "merkle_tree"),
    "mi355_msm_pairing_create": ("pairing", "Pairing"),
    "mi355_msm_pairing_destroy": ("pairing", "Pairing"),
    "mi355_msm_pairing_query": ("pairing", "Pairing::query"),
    "mi355_msm_pairing_run": ("pairing", "pairing"),
    "mi355_msm_pairing_check": ("pairing", "check_groups"),
    "mi355_msm_h2c_create": ("h2c", "HashToCurve"),
    "mi355_msm_h2c_destroy": ("h2c", "HashToCurve"),
    "mi355_msm_h2c_query": ("h2c", "HashToCurve::query"),
    "mi355_msm_h2c_hash": ("h2c", "HashToCurve::hash"),
    "mi355_msm_h2c_field": ("h2c", "hash_to_field"),
    "mi355_msm_h2c_map": ("h2c", "map_to_curve"),
    "mi355_msm_domain_mle_fix": ("mle", "mle_fix_variables"),
    "mi355_msm_domain_mle_eq": ("mle", "eq_table"),
    "mi355_msm_domain_sumcheck_round": ("mle", "sumcheck_round"),
}
# wrappers that reach the C ABI through another wrapper, or not at all: they must have run as well
ALSO_RAN = {
    "transforms": ["size", "ifft", "coset_fft", "coset_ifft"],
    "vecops": ["sub", "mul_sub", "scale", "batch_inversion"],
    "scans": ["prefix_product", "prefix_sum"],
    "sparse": ["rows", "cols", "groth16_witness_map"],
    "mle": ["mle_evaluate"],
    "fixed": ["msm_affine"],
    "pairing": ["product_of_pairings"],
    "points": ["mul_points_by", "mul_by_cofactor", "msm", "ifft_points"],
}
CASES = [(family, field) for family in oc.FAMILIES for field in oc.fields_of(family)]


def _build():
    newest = max(os.path.getmtime(p) for p in (SRC, HPP, os.path.join(ROOT, "include", "mi355_msm.h")))
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < newest:
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE, "-L" + PKG,
                        "-lmi355msm", "-ldl", "-Wl,-rpath,$ORIGIN/../2022-entries_amd", "-Wl,-rpath," + PKG], check=True)


def _run(case, workdir, no_device=False):
    """write the inputs, run the one process of this case under its time limit; a process that a signal ends fails the test at once"""
    for name, data in case.inputs.items():
        with open(os.path.join(workdir, name), "wb") as f:
            f.write(data)
    with open(os.path.join(workdir, "case.txt"), "w") as f:
        f.write(case.case_txt(no_device))
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), EXE, case.family, str(workdir)], capture_output=True, text=True)
    # (timeout passes a signal on as 128 + its number, and gives 124 / 137 when the limit ran out)
    assert 0 <= r.returncode < 124, "the process was ended by a signal or by its time limit (%d):\n" % r.returncode + r.stdout + r.stderr
    return r


def test_the_harness_builds_without_a_warning(built):
    if os.path.exists(EXE):
        os.remove(EXE)
    _build()
    assert os.path.exists(EXE)


def test_every_entry_point_of_the_header_is_reached_by_a_harness():
    """the coverage pin: a wrapper added to the header without a case in one of the two harnesses fails here, on the CPU"""
    hpp = open(HPP).read()
    called = set(re.findall(r"\b(mi355_msm_\w+)\s*\(", hpp))
    assert len(called) > 60, called
    first_harness = open(os.path.join(ROOT, "tests", "harness_msm_correctness.cpp")).read()
    missing = sorted(name for name in called if name not in ENTRY_POINTS and not re.search(r"\b%s\b" % name, first_harness))
    assert not missing, "the header calls these and no harness runs them: %s" % missing
    stale = sorted(name for name in ENTRY_POINTS if name not in called)
    assert not stale, "the table names entry points the header no longer calls: %s" % stale
    source = open(SRC).read()
    for name, (family, wrapper) in ENTRY_POINTS.items():
        assert family in oc.FAMILIES and 'ran("%s")' % wrapper in source, (name, family, wrapper)
    for family, wrappers in ALSO_RAN.items():
        for wrapper in wrappers:
            assert 'ran("%s")' % wrapper in source, (family, wrapper)


def _wrappers(family):
    return sorted({w for f, w in ENTRY_POINTS.values() if f == family} | set(ALSO_RAN.get(family, [])))


@pytest.mark.parametrize("family,field", CASES)
def test_without_a_gpu_the_first_constructor_throws_no_device(built, tmp_path, family, field):
    """mi355::MsmError with the code tests/test_lookup_api.py::test_without_a_gpu_no_table_can_exist expects of the C ABI, and exit 0"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU; with one the constructor returns, which is test_family_on_the_gpu")
    _build()
    r = _run(oc.build(family, field), tmp_path, no_device=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refused create MsmError:%d |" % oc.NO_DEVICE in r.stdout and "ran " not in r.stdout, r.stdout
    assert ("%s: done" % family) in r.stdout


def _compare(case, workdir, got_names):
    want = case.expected()
    bad = []
    for name, exp in sorted(want.items()):
        path = os.path.join(workdir, name)
        if not os.path.exists(path):
            bad.append("%s: not written" % name)
            continue
        got = open(path, "rb").read()
        if name in case.partial:
            size, keep = case.partial[name]
            if len(got) != len(exp):
                bad.append("%s: %d bytes, expected %d" % (name, len(got), len(exp)))
            elif any(got[size * i:size * (i + 1)] != exp[size * i:size * (i + 1)] for i in keep):
                bad.append("%s: differs in a record that is compared" % name)
        elif got != exp:
            where = next((i for i, (x, y) in enumerate(zip(got, exp)) if x != y), min(len(got), len(exp)))
            bad.append("%s: %d bytes against %d expected, first difference at byte %d" % (name, len(got), len(exp), where))
    extra = sorted(set(got_names) - set(want) - set(case.inputs) - case.judged_apart - {"case.txt"})
    if extra:
        bad.append("written and never compared: %s" % extra)
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("family,field", CASES)
def test_family_on_the_gpu(built, tmp_path, family, field):
    _build()
    case = oc.build(family, field)
    r = _run(case, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    ran = {ln[4:] for ln in lines if ln.startswith("ran ")}
    assert set(_wrappers(family)) <= ran, sorted(set(_wrappers(family)) - ran)
    # every refusal of the case fired, as the type and with the code the case names, and with a message
    for label, want in case.expect.items():
        kind, _, phrase = want.partition(" | ")
        told = [ln.split(" | ", 1)[1] for ln in lines if ln.startswith("refused %s %s | " % (label, kind))]
        assert len(told) == 1 and told[0] and phrase in told[0], (label, want, r.stdout)
    assert sum(ln.startswith("refused ") for ln in lines) == len(case.expect), r.stdout
    bad = _compare(case, tmp_path, os.listdir(tmp_path))
    assert not bad, "\n".join(bad)
    if family == "sparse":
        _witness_identity(case, tmp_path)
    if family == "expr":
        _slots_of_the_host_build(case, tmp_path)
    if family == "fixed":
        chosen = int.from_bytes(open(os.path.join(tmp_path, "window_bits"), "rb").read()[:8], "little")
        assert 1 <= chosen <= 16, chosen          # the engine's own choice for a large batch on G1 (mi355_msm.h)


def _witness_identity(case, workdir):
    """the witness map judged as tests/test_gpu_sparse.py judges it: A(tau) B(tau) - C(tau) == h(tau) Z(tau) at a point that shares
    nothing with the transforms, in the model's arithmetic, on the bytes the header returned"""
    import ntt_cases as nc
    import sparse_cases as sp

    f, k, R = case.field, case.log_size, case.r1cs
    h = nc.decode(f, open(os.path.join(workdir, "witness_h"), "rb").read(), False)
    assert len(h) == 1 << k
    a, b = R.padded(1 << k)
    lhs, rhs = sp.witness_identity(f, k, a, b, h, 0xC0FFEE)
    assert lhs == rhs


def _slots_of_the_host_build(case, workdir):
    """query("nodes") and query("columns") against the case's own numbers.  query("slots") has no model of its own: it is what the
    compiler of csrc/expr.hpp decides, so all this can say is that the header hands through the number that compiler gives when it is
    built for the host (libmsm_hosttest.so, pinned by tests/test_expr_host.py), and that it lies within the DAG's size."""
    import ctypes

    import test_expr_host as host

    lib = ctypes.CDLL(os.path.join(PKG, "libmsm_hosttest.so"))
    vp, ci, cu, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint64
    lib.ht_expr.argtypes = [ci, cu, vp, U64, vp, U64, U64, U64, vp, vp, U64, U64, vp, vp, vp, vp, U64]
    rc, msg, info, _ = host.host_expr(lib, case.field, 0, case.gate)
    assert rc == 0, msg
    got = open(os.path.join(workdir, "query"), "rb").read()
    slots, nodes, columns = (int.from_bytes(got[8 * i:8 * i + 8], "little") for i in range(3))
    assert (nodes, columns) == (len(case.gate.nodes), case.gate.n_cols) == (20, 3), (nodes, columns)         # the case's own numbers
    assert slots == info["slots"] and 0 <= slots <= 20, (slots, info)
