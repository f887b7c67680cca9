"""The cases of tests/harness_operators.cpp: for every family of wrappers in include/mi355_msm.hpp the input files, the integers of
case.txt, what every guarded call must do, and the bytes every output file must hold.  Nothing here comes from the code under test:
the expected bytes are those of the integer models the kernel tests already use (ntt_cases, poly_cases, scan_cases, quotient_cases,
sparse_cases, mle_cases, lookup_cases, expr_cases, poseidon_cases, codec_cases, check_cases), of oracle/pymodel.py for points, of the
golden pairings and of the RFC 9380 vectors.  Shapes are chosen for the marshalling of the header -- strides, flags, lengths, output
sizes -- not for the kernels, which have their own tests.

build(family, field) -> Case; Case.expected() runs the models (a few seconds for the families that multiply points)."""
import functools
import random
import struct

import ntt_cases as nc

FAMILIES = ("transforms", "vecops", "polys", "scans", "quotient", "sparse", "lookup", "expr", "poseidon", "pairing", "h2c", "mle", "fixed", "points")
FR_FIELDS = ("bls12_377", "bls12_381")
CURVE_ID = {"bls12_377": 0, "bls12_381": 1, "g1": 1, "g2": 3}
NO_DEVICE = 100          # hipErrorNoDevice, what tests/test_lookup_api.py expects of the C ABI without a GPU
INVALID, RUNTIME, REFUSED = "invalid_argument", "runtime_error", "MsmError:-1"


def because(kind, phrases):
    """label -> `kind | phrase`: the exception and words its message must contain, so that a label is not satisfied by another branch"""
    return {label: "%s | %s" % (kind, phrase) for label, phrase in phrases.items()}
UNTOUCHED = (1 << 64) - 1


def fields_of(family):
    return ("g1", "g2") if family == "h2c" else FR_FIELDS


def u64s(*values):
    return struct.pack("<%dQ" % len(values), *values)


def u32s(values):
    return struct.pack("<%dI" % len(values), *values)


def raw(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


class Case:
    """cfg: the integers of case.txt; inputs: name -> bytes; expect: label -> what the guarded call does; expected(): name -> bytes;
    partial: name -> (record size, indices) for the files that are compared at those records only"""

    def __init__(self, family, field):
        self.family, self.field = family, field
        self.cfg = {"curve": CURVE_ID[field]}
        self.inputs, self.expect, self.partial = {}, {}, {}
        self.judged_apart = set()           # outputs the test judges by other means than these bytes
        self.model = lambda: {}

    def expected(self):
        return self.model()

    def case_txt(self, no_device=False):
        lines = ["%s %d" % kv for kv in sorted(self.cfg.items())]
        if no_device:
            lines.append("expect.create MsmError:%d" % NO_DEVICE)
        else:
            lines += ["expect.%s %s" % kv for kv in sorted(self.expect.items())]
        return "\n".join(lines) + "\n"


def _mont(field):
    return lambda ints: nc.encode(field, list(ints), False)


# ---- the domain ---------------------------------------------------------------------------------------------------------------------------

def _transforms(c):
    f, E = c.field, _mont(c.field)
    r = nc.modulus(f)
    v = nc.random_values(f, 40, 101)
    c.cfg.update(num_coeffs=50, element=5)           # 50 coefficients round up to a domain of 2^6
    c.inputs = {"v": E(v), "too_long": E(nc.random_values(f, 65, 102))}
    c.expect = {"transform_too_long": REFUSED, "query_unknown": REFUSED}

    def model():
        out = {"size": u64s(64, 6), "element": E([pow(nc.root_of_unity(f, 6), 5, r)])}
        for name, kind in (("fft", nc.FORWARD), ("ifft", nc.INVERSE), ("coset_fft", nc.COSET_FORWARD), ("coset_ifft", nc.COSET_INVERSE)):
            out[name] = E(nc.transform(f, 6, kind, v))
        out["fft_again"] = out["fft"]
        return out
    c.model = model


def _vecops(c):
    import poly_cases as pc
    import quotient_cases as qc

    f, E = c.field, _mont(c.field)
    r = nc.modulus(f)
    a, b, cc_, shorter = (nc.random_values(f, n, 110 + i) for i, n in enumerate((64, 64, 64, 40)))
    s, coeff = nc.random_values(f, 2, 115)
    inv_vals = nc.random_values(f, 50, 116)
    inv_vals[7] = 0
    inv_raw = bytearray(E(inv_vals))
    inv_raw[32 * 20:32 * 21] = r.to_bytes(32, "little")        # the byte pattern r is zero as well
    inv_vals[20] = 0
    cols = [nc.random_values(f, n, 120 + n) for n in (64, 40, 1)]
    lc = nc.random_values(f, 3, 117)
    c.inputs = {"a": E(a), "b": E(b), "c": E(cc_), "shorter": E(shorter), "s": E([s]), "coeff": E([coeff]), "inv_in": bytes(inv_raw),
                "lc0": E(cols[0]), "lc1": E(cols[1]), "lc2": E(cols[2]), "lc_coeffs": E(lc)}
    c.expect = because(INVALID, {"mul_unequal": "mul: a and b", "mul_unequal_first": "mul: a and b", "add_unequal": "vec_op: a and b",
                                 "sub_unequal": "vec_op: a and b", "mul_sub_unequal": "vec_op: c differs", "vec_op_needs_c": "needs c",
                                 "linear_combination_coeffs": "coeffs holds"})
    c.expect["vec_op_unknown"] = REFUSED

    def model():
        out = {"mul": E(x * y % r for x, y in zip(a, b)), "add": E((x + y) % r for x, y in zip(a, b)), "sub": E((x - y) % r for x, y in zip(a, b)),
               "mul_sub": E((x * y - z) % r for x, y, z in zip(a, b, cc_)), "scale": E(x * s % r for x in a),
               "batch_inversion": E(pc.ref_inverse(inv_vals, 1, r)), "batch_inversion_and_mul": E(pc.ref_inverse(inv_vals, coeff, r)),
               "linear_combination": E(qc.ref_lincomb(cols, lc, r))}
        out["mul_again"], out["mul_sub_again"] = out["mul"], out["mul_sub"]
        return out
    c.model = model


def _polys(c):
    import poly_cases as pc

    f, E = c.field, _mont(c.field)
    r, g = nc.modulus(f), nc.generator(f)
    coeffs, evals = nc.random_values(f, 50, 130), nc.random_values(f, 64, 131)
    z, tau = nc.random_values(f, 2, 132)
    offset = pow(g, 5, r)
    c.inputs = {"coeffs": E(coeffs), "evals": E(evals), "z": E([z]), "tau": E([tau]), "offset": E([offset]), "zero": E([0])}
    c.expect = {"dvc_zero_offset": REFUSED}

    def model():
        q, rem = pc.ref_divide(coeffs, z, r)
        by = lambda off: E(x * pow(pow(off, 64, r) - 1, -1, r) % r for x in evals)
        out = {"evaluate": E([pc.ref_evaluate(coeffs, z, r)]), "divide_by_linear": E(q), "rem": E([rem]), "divide_by_linear_norem": E(q),
               "lagrange": E(pc.ref_lagrange(f, 6, tau)), "vanishing": E([(pow(tau, 64, r) - 1) % r]), "dvc": by(g), "dvc_offset": by(offset)}
        out["dvc_again"] = out["dvc"]
        return out
    c.model = model


def _scans(c):
    import scan_cases as sc

    f, E = c.field, _mont(c.field)
    r = nc.modulus(f)
    rng = random.Random("operator scans " + f)
    v = [rng.randrange(1, r) for _ in range(70)]
    stride = 64 + 3
    perm = sc.permutation(f, 6, 3, 140)
    bad = sc.broken(perm, 141)
    c.cfg.update(stride=stride)
    c.inputs = {"v": E(v), "wires": perm.columns(perm.wires, False, stride), "wires_broken": bad.columns(bad.wires, False, stride),
                "sigmas": perm.columns(perm.sigmas, False, stride), "ks": E(perm.ks), "beta": E([perm.beta]), "gamma": E([perm.gamma])}
    c.expect = because(INVALID, {"permutation_short_wires": "wires holds", "permutation_short_sigmas": "sigmas holds",
                                 "permutation_small_stride": "stride is below", "permutation_no_columns": "ks is empty"})
    c.expect["permutation_nine_columns"] = REFUSED

    def model():
        out = {}
        for name, op in (("product", sc.PRODUCT), ("sum", sc.SUM)):
            for inclusive in (False, True):
                vals, total = sc.ref_scan(v, op, inclusive, r)
                key = "%s_%s" % (name, "inclusive" if inclusive else "exclusive")
                out[key], out[key + "_total"] = E(vals), E([total])
        out["sum_default"] = out["sum_exclusive"]
        z, total = perm.model()
        assert total == 1                                   # satisfied copy constraints: the image of one
        out["permutation"], out["permutation_total"] = E(z), E([total])
        z, total = bad.model()
        assert total != 1
        out["permutation_broken"], out["permutation_broken_total"] = E(z), E([total])
        out["permutation_again"], out["permutation_again_total"] = out["permutation"], out["permutation_total"]
        return out
    c.model = model


def _quotient(c):
    import poly_cases as pc
    import quotient_cases as qc

    f, E = c.field, _mont(c.field)
    r = nc.modulus(f)
    K, n, stride = 7, 32, 128 + 2
    rows = qc.Rows(f, K, n, 5, 150 + nc.FIELD_IDS[f])
    offset = pow(nc.generator(f), 5, r)
    c.cfg.update(M=1 << K, n=n, stride=stride)
    c.inputs = {"wires": rows.columns(rows.wires, stride), "sigmas": rows.columns(rows.sigmas, stride), "selectors": rows.columns(rows.selectors, stride),
                "z": pc.to_raw(rows.z), "pi": pc.to_raw(rows.pi), "ks": E(rows.ks), "alpha": E([rows.alpha]), "beta": E([rows.beta]),
                "gamma": E([rows.gamma]), "offset": E([offset])}
    c.expect = because(INVALID, {"short_wires": "wires holds", "short_sigmas": "sigmas holds", "short_selectors": "selectors holds", "short_z": "z holds",
                                 "short_pi": "pi holds", "small_stride": "stride is below", "no_columns": "ks is empty"})
    c.expect["bad_ratio"] = REFUSED

    def model():
        val = lambda x: pc.values(f, x, False)
        cols = lambda cs: [val(x) for x in cs]
        w, s, q, z, pi = cols(rows.wires), cols(rows.sigmas), cols(rows.selectors), val(rows.z), val(rows.pi)
        ref = lambda sel, p, g=None: E(qc.ref_quotient_rows(f, K, n, w, s, sel, z, p, rows.ks, rows.alpha, rows.beta, rows.gamma, g))
        out = {"full": ref(q, pi), "no_selectors": ref(None, pi), "no_pi": ref(q, None), "bare_offset": ref(None, None, offset)}
        out["full_again"] = out["full"]
        return out
    c.model = model


def _csr(field, matrix):
    """arkworks' Matrix<F> (rows of (coefficient, column)) as CSR files"""
    row_ptr, col_idx, values = [0], [], []
    for row in matrix:
        for coeff, col in row:
            col_idx.append(col)
            values.append(coeff)
        row_ptr.append(len(col_idx))
    return u64s(*row_ptr), u32s(col_idx), nc.encode(field, values, False)


def _sparse(c):
    import sparse_cases as sp

    f, E = c.field, _mont(c.field)
    r, g = nc.modulus(f), nc.generator(f)
    rng = random.Random("operator sparse " + f)
    m = sp.Case("an empty row and a long one", f, [2, 0, 40, 1, 3], 9, rng)
    k, constraints, nvars, num_inputs = 4, 8, 6, 2
    R = sp.R1cs(f, constraints, nvars, num_inputs, rng)
    c.cfg.update(domain=1 << k, rows=m.rows, cols=m.cols, constraints=constraints, nvars=nvars, num_inputs=num_inputs)
    c.inputs = {"row_ptr": u64s(*m.row_ptr), "col_idx": u32s(m.col_idx), "values": m.values_raw(), "z": m.z_raw(), "witness": E(R.z)}
    for name, mat in (("a", R.A), ("b", R.B)):
        c.inputs[name + "_row_ptr"], c.inputs[name + "_col_idx"], c.inputs[name + "_values"] = _csr(f, mat)
    c.expect = because(INVALID, {"apply_short_z": "z holds cols()", "apply_long_z": "z holds cols()", "create_short_row_ptr": "row_ptr holds",
                                 "create_empty_row_ptr": "row_ptr holds", "create_short_col_idx": "col_idx holds", "create_short_values": "values holds",
                                 "witness_map_inputs": "fewer than num_inputs", "witness_map_domain": "do not fit the domain"})
    c.expect["create_column_out_of_range"] = REFUSED
    c.r1cs, c.log_size = R, k

    def model():
        out = {"shape": u64s(m.rows, m.cols, m.nnz), "apply": m.expected(False, False), "witness_a": E(R.a), "witness_b": E(R.b)}
        out["apply_again"] = out["apply"]
        a, b = R.padded(1 << k)
        ab = [x * y % r for x, y in zip(a, b)]
        on_coset = lambda v: nc.transform(f, k, nc.COSET_FORWARD, nc.transform(f, k, nc.INVERSE, v))
        zinv = pow(pow(g, 1 << k, r) - 1, -1, r)
        h = nc.transform(f, k, nc.COSET_INVERSE, [(x * y - z) * zinv % r for x, y, z in zip(on_coset(a), on_coset(b), on_coset(ab))])
        lhs, rhs = sp.witness_identity(f, k, a, b, h, 0x5EED + k)
        assert lhs == rhs
        out["witness_h"] = E(h)
        return out
    c.model = model


def _lookup(c):
    import lookup_cases as lk

    f = c.field
    r = nc.modulus(f)
    rng = random.Random("operator lookup " + f)
    base = lk.distinct_table(f, 16, rng)
    table, outsider = base[:15] + [base[3]], base[15]                   # a duplicate of entry 3 at the end
    present = lk.draw(table[:15], 30, rng) + [table[2] % r + r, table[15]]
    values = present[:11] + [outsider] + present[11:]                   # one value the table does not hold, at index 11
    lc = lk.logup_case(f, False, 16, 2, 16, 160)
    c.inputs = {"table": lk.raw_bytes(table), "values": lk.raw_bytes(values), "values_present": lk.raw_bytes(present), "logup_table": lc["table"],
                "logup_mult": lc["mult"], "logup_beta": lc["beta"], "logup_col0": lc["values"][:512], "logup_col1": lc["values"][512:]}
    assert len(lc["values"]) == 1024
    c.expect = because(INVALID, {"logup_short_column": "columns holds", "logup_long_column": "columns holds", "logup_short_mult": "mult holds",
                                 "logup_no_columns": "columns is empty"})
    c.expect["create_empty_table"] = REFUSED

    def model():
        index, counts, missing, first = lk.model_count(f, c.inputs["table"], c.inputs["values"])
        assert (missing, first) == (1, 11) and counts[15] == 0 and counts[3] >= 1
        index2, counts2, missing2, _ = lk.model_count(f, c.inputs["table"], c.inputs["values_present"])
        assert missing2 == 0
        phi, total, _ = lk.model_logup(f, lc["table"], lc["mult"], lc["values"], 2, 16, 16, lc["beta"], False)
        assert total == bytes(32)
        out = {"query": u64s(16, 15), "mult": lk.model_mult(f, counts, False), "index": u32s(index), "stats": u64s(missing, first),
               "sorted_missing": b"", "sorted_missing_first": u64s(first), "sorted": lk.model_sorted(f, c.inputs["table"], counts2),
               "sorted_first": u64s(UNTOUCHED), "mult_present": lk.model_mult(f, counts2, False), "logup": phi, "logup_total": total, "logup_nototal": phi}
        out["logup_again"], out["mult_again"] = out["logup"], out["mult"]
        return out
    c.model = model


@functools.lru_cache(maxsize=None)
def gate_case():
    """a 20-node DAG whose RESULT depends on its rotations (+1 and -1 are among them), its constant, both challenges and the column of
    length 1: the first seed of expr_cases.random_dag at which changing any of them changes the value the model gives"""
    import expr_cases as xc

    f = "bls12_377"
    rng = random.Random("operator gate")
    cols = [[rng.getrandbits(200) for _ in range(n)] for n in (8, 8, 1)]
    chals = [rng.getrandbits(200), rng.getrandbits(200)]
    for seed in range(2000):
        case = xc.random_dag(seed, 20, n_cols=3, n_consts=1, n_chal=2)
        rots = {b for op, a, b in case.nodes if op == xc.COL}
        if case.nodes[-1][0] < xc.ADD or not {1, xc.u32(-1)} <= rots:
            continue
        base = xc.evaluate(f, case.nodes, case.consts, chals, cols, 8, 2)
        others = [xc.evaluate(f, case.nodes, case.consts, chals, cols, 8, 1), xc.evaluate(f, case.nodes, [case.consts[0] + 1], chals, cols, 8, 2),
                  xc.evaluate(f, case.nodes, case.consts, [chals[0] + 1, chals[1]], cols, 8, 2),
                  xc.evaluate(f, case.nodes, case.consts, [chals[0], chals[1] + 1], cols, 8, 2),
                  xc.evaluate(f, case.nodes, case.consts, chals, cols[:2] + [[cols[2][0] + 1]], 8, 2)]
        if all(o != base for o in others):
            return case
    raise AssertionError("no such DAG")


def _expr(c):
    import expr_cases as xc

    f, E = c.field, _mont(c.field)
    case = gate_case()
    rng = random.Random("operator expr " + f)
    r = nc.modulus(f)
    cols = [[rng.randrange(r) for _ in range(n)] for n in (64, 64, 1)]      # the third column is a scalar
    chals = [rng.randrange(r) for _ in range(2)]
    c.cfg.update(rot_step=2)
    c.inputs = {"nodes": u32s(case.flat()), "consts": E(case.consts), "challenges": E(chals), "col0": E(cols[0]), "col1": E(cols[1]), "col2": E(cols[2])}
    c.expect = {"run_column_missing": REFUSED, "run_challenge_missing": REFUSED, **because(INVALID, {"create_bad_nodes": "triples"})}
    c.gate = case
    c.judged_apart = {"query"}              # the slots: against the compiler built for the host

    def model():
        out = {"run": E(xc.evaluate(f, case.nodes, case.consts, chals, cols, 64, 2)), "run_step1": E(xc.evaluate(f, case.nodes, case.consts, chals, cols, 64, 1))}
        assert out["run"] != out["run_step1"]
        out["run_again"] = out["run"]
        return out
    c.model = model


def _poseidon(c):
    import poseidon_cases as ps

    f, E = c.field, _mont(c.field)
    m = ps.Model.generated(f, 2)
    rng = random.Random("operator poseidon " + f)
    in_len, n_out, leaf_len = 3, 2, 2
    rows = [[rng.randrange(m.p) for _ in range(in_len)] for _ in range(3)]
    leaves = [[rng.randrange(m.p) for _ in range(leaf_len)] for _ in range(5)]
    sep = ps.domain_element("OperatorHarness", m.p)
    header = m.header(sep, in_len)
    c.cfg.update(rate=2, alpha=m.alpha, full_rounds=m.full_rounds, partial_rounds=m.partial_rounds, in_len=in_len, n_out=n_out, leaf_len=leaf_len)
    c.inputs = {"ark": E(ps.flat(m.ark)), "mds": E(ps.flat(m.mds)), "in": E(ps.flat(rows)), "header": E(header), "leaves": E(ps.flat(leaves)),
                "domain_sep": E([sep])}
    c.expect = because(INVALID, {"create_short_ark": "ark: one row", "create_short_mds": "mds: rate + 1 rows", "hash_bad_header": "a header holds",
                                 "hash_ragged_rows": "whole rows", "merkle_ragged_leaves": "whole leaves", "merkle_no_leaves": "whole leaves"})
    c.expect["create_even_alpha"] = REFUSED

    def model():
        tree, _ = m.merkle(sep, leaves)
        assert len(tree) == 15
        out = {"query": u64s(2, 3, m.full_rounds + m.partial_rounds), "hash": E(ps.flat(m.sponge(row, n_out) for row in rows)),
               "hash_header": E(ps.flat(m.sponge(header + row, n_out) for row in rows)), "hash_one_out": E(ps.flat(m.sponge(header + row, 1) for row in rows)),
               "merkle_tree": E(tree)}
        out["hash_again"] = out["hash_header"]
        return out
    c.model = model


def _mle(c):
    import mle_cases as mc

    f, E = c.field, _mont(c.field)
    r = nc.modulus(f)
    rng = random.Random("operator mle " + f)
    evals = mc.raw_values(f, 32, rng)
    full_point = [rng.randrange(r) for _ in range(5)]
    fix_point, eq_point = full_point[:3], [rng.randrange(r) for _ in range(4)]         # a point shorter than num_vars
    rc = mc.RoundCase(f, "spartan", 4, rng)                                            # eq (a b - c): degree 3 over four tables
    c.cfg.update(tables=rc.m)
    c.inputs = {"evals": mc.raw_bytes(evals), "fix_point": E(fix_point), "full_point": E(full_point), "eq_point": E(eq_point),
                "term_coeffs": E(rc.coeffs), "term_n_factors": u32s([len(fs) for fs in rc.factors]),
                "term_factors": u32s([x for fs in rc.factors for x in fs + [0] * (5 - len(fs))]), "r_prev": mc.raw_bytes([rc.r_prev])}
    for k, t in enumerate(rc.tables):
        c.inputs["table%d" % k] = mc.raw_bytes(t)
    c.expect = because(INVALID, {"fix_not_a_power_of_two": "2^num_vars", "fix_long_point": "more values than variables",
                                 "evaluate_short_point": "one value per variable", "round_no_tables": "no tables", "round_ragged_tables": "differ in length",
                                 "round_no_place_for_folded": "r_prev needs", "round_six_factors": "1 .. 5 factors", "round_no_factors": "1 .. 5 factors"})
    c.expect["round_unknown_table"] = REFUSED

    def model():
        table = nc.decode(f, c.inputs["evals"], False)
        plain, _ = rc.expected(False, False)
        fused, folded = rc.expected(False, True)
        assert len(plain) == 4
        out = {"fix": E(mc.fix_variables(r, table, fix_point)), "evaluate": E([mc.evaluate(r, table, full_point)]), "eq": E(mc.eq_table(r, eq_point)),
               "round": E(plain), "round_fused": E(fused), "folded_count": u64s(rc.m), "round_again": E(plain)}
        for k, t in enumerate(folded):
            out["folded%d" % k] = t
        return out
    c.model = model


# ---- pairings and hash-to-curve ----------------------------------------------------------------------------------------------------------------

def _pairing(c):
    import pairing_cases as pg

    F = pg.FAMILIES[c.field]
    g1, g2, em, ec = pg.load_golden(F)
    pairs = [0, 1, 2, 3]                    # the generators and three random pairs
    chk = [1, 15, 2, 18]                    # (P, Q), (-P, Q): one; (P', Q'), (O, Q''): not one
    c.inputs = {"g1": b"".join(g1[i] for i in pairs), "g2": b"".join(g2[i] for i in pairs), "check_g1": b"".join(g1[i] for i in chk),
                "check_g2": b"".join(g2[i] for i in chk)}
    c.expect = because(INVALID, {"pairing_ragged_g1": "whole groups", "pairing_short_g2": "whole groups", "pairing_group_zero": "whole groups",
                                 "pairing_partial_group": "whole groups", "product_empty": "at least one pair", "check_partial_group": "whole groups",
                                 "check_short_g2": "whole groups"})
    c.expect["query_unknown"] = REFUSED

    def model():
        e = [pg.gt_from_image(F, em[i]) for i in pairs]
        assert pg.gt_image(F, e[0]) == em[0] and pg.gt_image(F, e[1], True) == ec[1]
        one = pg.f12_one()
        assert pg.f12_mul(F, pg.gt_from_image(F, em[1]), pg.gt_from_image(F, em[15])) == one and pg.gt_from_image(F, em[18]) == one
        lo, hi = pg.f12_mul(F, e[0], e[1]), pg.f12_mul(F, e[2], e[3])
        prod = pg.f12_mul(F, lo, hi)
        out = {"query": u64s(CURVE_ID[c.field]), "pairing": b"".join(em[i] for i in pairs), "pairing_canonical": b"".join(ec[i] for i in pairs),
               "pairing_group2": pg.gt_image(F, lo) + pg.gt_image(F, hi), "product": pg.gt_image(F, prod), "product_canonical": pg.gt_image(F, prod, True),
               "check_groups": bytes([1, 0]), "check_groups_single": bytes([0, 0, 0, 1])}
        out["pairing_again"] = out["pairing_group2"]
        return out
    c.model = model


def _h2c(c):
    import h2c_cases as hc

    group = c.field
    fx = hc.fixture("BLS12381%s_XMD-SHA-256_SSWU_RO_.json" % group.upper())
    dst = fx["dst"].encode()
    vectors = fx["vectors"]
    msgs = [v["msg"].encode() for v in vectors]
    assert len(msgs) == 5
    stride = hc.STRIDE[group]
    us = [hc.parse_el(group, u) for v in vectors for u in v["u"]]
    offsets = [0]
    for m in msgs:
        offsets.append(offsets[-1] + len(m))
    c.inputs = {"dst": dst, "messages": b"".join(msgs), "message_offsets": u64s(*offsets), "u": b"".join(hc.el_image(u) for u in us)}
    c.expect = {**because(INVALID, {"map_ragged": "whole pairs", "map_odd_pairs": "whole pairs"}), "field_count_three": REFUSED, "create_377": REFUSED,
                "create_empty_tag": REFUSED}

    def model():
        img = lambda P: hc.affine_image(group, P, stride)
        pt = lambda d: hc.parse_point(group, d)
        out = {"query": u64s(CURVE_ID[group], len(dst), stride // 100, stride), "hash": b"".join(img(pt(v["P"])) for v in vectors),
               "encode": b"".join(img(hc.encode_to_curve(group, m, dst)) for m in msgs), "field": c.inputs["u"],
               "field_one": b"".join(hc.el_image(hc.hash_to_field(group, m, dst, 1)[0]) for m in msgs),
               "map": b"".join(img(pt(v[q])) for v in vectors for q in ("Q0", "Q1")), "map_pairs": b"".join(img(pt(v["P"])) for v in vectors)}
        out["hash_again"] = out["hash"]
        return out
    c.model = model


# ---- points -------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _generator_multiples(name):
    import fixed_base_cases as fc
    import pymodel as pm

    curve = pm.CURVES[name]
    return fc.Expect(curve, curve.generator())


def _fixed(c):
    import pymodel as pm

    f, E = c.field, _mont(c.field)
    name = f + "_g1"
    curve = pm.CURVES[name]
    rng = random.Random("operator fixed " + f)
    ks = [0, 1, curve.r - 1] + [rng.randrange(curve.r) for _ in range(67)]
    c.cfg.update(window=5)
    c.inputs = {"g": curve.encode_affine(curve.generator()), "scalars": E(ks)}          # Fr values in Montgomery form, as FixedBase::msm takes them
    c.expect = {"window_too_wide": REFUSED, "unknown_curve": REFUSED, "query_unknown": REFUSED}
    c.partial = {"window_bits": (8, [1, 2])}                                              # the engine's own choice is not the model's to predict

    def model():
        exp = _generator_multiples(name)
        ark = lambda n: 3 if n < 32 else (n - 1).bit_length() * 69 // 100              # arkworks' get_mul_window_size
        out = {"window_bits": u64s(0, 5, -(-256 // 5)), "window_size": u64s(ark(10), ark(1000)), "msm": exp.projective(ks), "msm_affine": exp.affine(ks)}
        out["msm_forced"] = out["msm_again"] = out["msm"]
        out["msm_affine_moved"] = out["msm_affine"]
        return out
    c.model = model


def _check_counts(statuses, flags, method):
    import check_cases as cc

    s = cc.summary(statuses, flags)
    return u64s(*s, int(s[5] == len(statuses)), method)


def _points(c):
    import check_cases as cc
    import codec_cases as dc
    import point_mul_cases as pmc
    import pymodel as pm

    f, E = c.field, _mont(c.field)
    name = f + "_g1"
    curve = pm.CURVES[name]
    r = curve.r
    rng = random.Random("operator points " + f)
    mult = _generator_multiples(name)
    G = curve.generator()
    comps = lambda P: ((P[0],), (P[1],))

    # a dozen records of the check corpus: three of every status, a flagged infinity among the valid ones
    cases, statuses, labels = cc.corpus(name)
    pick = []
    for s in (0, 1, 2, 3):
        idx = [i for i, st in enumerate(statuses) if st == s]
        if s == 0:
            idx = idx[:2] + [i for i in idx if cases[i][0]][:1]
        pick.append(idx[:3])
    order = [pick[0][0]] + [pick[s][j] for j in range(3) for s in (3, 2, 1, 0) if (s, j) != (0, 0)]     # a valid point first: first_invalid is 1
    picked, want = [cases[i] for i in order], [statuses[i] for i in order]
    assert len(picked) == 12 and sorted(want) == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3] and any(p[0] for p in picked)
    flags = [p[0] for p in picked]

    # the codec: valid points and an infinity to compress, one record whose x is not canonical; records of every status to decode
    logs = [rng.randrange(1, r) for _ in range(4)]
    good = [mult(k) for k in logs] + [None]
    lifted = cc.encode(curve, cc._pt(curve, mult(logs[0]), lx=(1,)), False)
    recs, rstat, _, sub = dc.corpus(name)
    by = lambda s, in_sub=True: next(rec for rec, st, g in zip(recs, rstat, sub) if st == s and g == in_sub)
    to_decode = [dc.compress(curve, None if P is None else comps(P)) for P in good] + [by(dc.MALFORMED), by(dc.NO_POINT), by(dc.OK, False)]

    # point multiplication: subgroup points and a flagged infinity
    few_logs = [1] + [rng.randrange(1, r) for _ in range(3)]
    few = [mult(k) for k in few_logs] + [None]
    ks = [r - 1, 7, rng.getrandbits(256), (1 << 255) + 12345, rng.randrange(r)]
    k_one = 0xC0FFEE1122334455
    few_scalars = [rng.randrange(r) for _ in range(10)]                                    # two batches on the five bases of init

    # MSM on bases set from compressed records: 16 multiples of the generator, two batches
    msm_logs = [rng.randrange(1, r) for _ in range(16)]
    msm_pts = [mult(k) for k in msm_logs]
    msm_scalars = [rng.randrange(r) for _ in range(32)]
    msm_scalars[3], msm_scalars[20] = 0, r - 1

    # msm_chunks: 260 bases (eight distinct ones in turn), 256 Fr scalars that pair up with the LAST 256
    chunk_logs = [rng.randrange(1, r) for _ in range(8)]
    chunk_scalars = [rng.randrange(r) for _ in range(256)]
    fft_logs = [rng.randrange(1, r) for _ in range(3)]

    c.cfg.update(step=100, fft_size=4)
    c.inputs = {
        "corpus": cc.encode_all(curve, picked, False), "compress_points": curve.encode_affine_array(good) + lifted, "records": b"".join(to_decode),
        "mul_points": curve.encode_affine_array(few), "mul_scalars": raw(ks), "mul_scalars_montgomery": E(k % r for k in ks), "k": k_one.to_bytes(8, "little"),
        "few_scalars": raw(few_scalars), "msm_records": b"".join(dc.compress(curve, comps(P)) for P in msm_pts), "msm_points": curve.encode_affine_array(msm_pts),
        "msm_scalars": raw(msm_scalars), "chunk_bases": curve.encode_affine_array([mult(chunk_logs[i % 8]) for i in range(260)]),
        "chunk_scalars": E(chunk_scalars), "fft_points_in": curve.encode_affine_array([mult(k) for k in fft_logs])}
    c.expect = {"check_device_bad_stride": REFUSED, "mul_points_by_three_bytes": REFUSED, "set_bases_compressed_malformed": REFUSED,
                "fft_points_too_long": REFUSED, **because(RUNTIME, {"mul_points_ragged": "one 32-byte scalar per point"}),
                # MsmError -1 thrown by the wrappers themselves
                **because(REFUSED, {"msm_point_count": "different point count", "msm_partial_batch": "whole number of batches",
                                    "msm_chunks_more_scalars": "msm_chunks:", "msm_chunks_step_zero": "msm_chunks:"})}
    # a record that failed leaves unspecified bytes; which method a decode names is the engine's to say
    c.partial = {"compress_records": (48, list(range(5))), "decompress_validate_points": (104, list(range(7))), "decompress_counts": (8, list(range(7))),
                 "decompress_validate_counts": (8, list(range(7))), "compress_counts": (8, list(range(7)))}

    def model():
        out = {}
        for key, method in (("check", 1), ("check_exact", 0), ("check_device", 1), ("check_device_exact", 0)):
            out[key + "_status"], out[key + "_counts"] = bytes(want), _check_counts(want, flags, method)
        out["compress_status"] = bytes([0] * 5 + [1])
        out["compress_counts"] = u64s(5, 1, 1, 0, 0, 5, 0, 0)
        out["compress_records"] = b"".join(to_decode[:5]) + bytes(48)
        st, images = dc.expected(curve, b"".join(to_decode), False)
        infinities = [int(s == 0 and (rec[-1] >> 6) == 1) for s, rec in zip(st, to_decode)]
        out["decompress_status"], out["decompress_points"] = bytes(st), images
        out["decompress_counts"] = _check_counts(st, infinities, 0)
        stv = st[:7] + [3]
        out["decompress_validate_status"], out["decompress_validate_points"] = bytes(stv), images
        out["decompress_validate_counts"] = _check_counts(stv, infinities, 0)
        mul = lambda k, P: None if P is None else curve.mul(k, P)
        out["mul_points"] = out["mul_points_again"] = curve.encode_affine_array([mul(k, P) for k, P in zip(ks, few)])
        out["mul_points_montgomery"] = curve.encode_affine_array([mul(k % r, P) for k, P in zip(ks, few)])
        out["mul_points_by"] = curve.encode_affine_array([mul(k_one, P) for P in few])
        out["mul_by_cofactor"] = curve.encode_affine_array([mul(pmc.cofactor(curve), P) for P in few])
        fold = lambda logs_, scalars: curve.encode_projective_normalized(mult(sum(s * k for s, k in zip(scalars, logs_)) % r or r))
        init_logs = few_logs + [0]
        out["msm_init"] = fold(init_logs, few_scalars[:5]) + fold(init_logs, few_scalars[5:])
        both = fold(msm_logs, msm_scalars[:16]) + fold(msm_logs, msm_scalars[16:])
        out["msm_compressed"] = out["msm_compressed_again"] = out["msm_async"] = both
        out["msm_async_done"] = u64s(1, 1)
        out["msm_stateless"] = fold(msm_logs, msm_scalars[:16])                      # chopped to the shorter input: the 16 bases
        out["msm_chunks"] = out["msm_chunks_one_step"] = fold([chunk_logs[(4 + i) % 8] for i in range(256)], chunk_scalars)
        field = nc.FIELD_OF_CURVE[name]
        for key, kind in (("fft_points", nc.FORWARD), ("ifft_points", nc.INVERSE)):
            out[key] = curve.encode_affine_array([mult(k or r) for k in nc.transform(field, 2, kind, fft_logs)])
        out["fft_points_again"] = out["fft_points"]
        return out
    c.model = model


_BUILDERS = {"transforms": _transforms, "vecops": _vecops, "polys": _polys, "scans": _scans, "quotient": _quotient, "sparse": _sparse, "lookup": _lookup,
             "expr": _expr, "poseidon": _poseidon, "pairing": _pairing, "h2c": _h2c, "mle": _mle, "fixed": _fixed, "points": _points}


@functools.lru_cache(maxsize=None)
def build(family, field):
    c = Case(family, field)
    _BUILDERS[family](c)
    return c
