#!/usr/bin/env python3
"""Worst-case limbs, columns and values of the butterfly chain of csrc/ntt.hpp on the 9 x 29 scalar fields (csrc/fr.hpp).

A pass loads class-M values (normalised limbs, value < 2r), runs up to NTT_MAX_PASS_LOG = 10 levels of

    t = w * b (fr_mul, w canonical);  a' = a + t;  b' = a + BIAS4 - t;  one carry pass on each

and ends with products by canonical table entries.  This script carries an upper bound per limb and on the value through that chain
exactly as the code performs it and prints, per field and level, the margin of

  * every product-scanning column against 2^64:  col_k <= sum_{i+j=k} A_i W_j + (2^29 - 1) sum_{i+j=k, j>=1} r_j + (2^29 - 1) + carry,
  * every limb against the 2^31 that fr_mul accepts and every limb-wise sum against 2^32,
  * every limb of BIAS4 against the limb of t it meets,
  * the value of a product's first operand against R = 2^261 (what keeps the product below 2r), and 2r against the 2^256 of a stored
    element.

All margins must be positive (tests/test_fr_consts.py runs it); the host build checks the same sums on every product (MSM_CHECK).

    python tools/limb_bounds_fr.py
    python tools/limb_bounds_fr.py --poly     (the chains of csrc/poly.hpp: analyse_poly below)
    python tools/limb_bounds_fr.py --scan     (the sum scan and the permutation product of csrc/scan.hpp: analyse_scan below)
    python tools/limb_bounds_fr.py --quotient (the rows of the Plonk quotient and the linear combination of csrc/quotient.hpp: analyse_quotient below)
    python tools/limb_bounds_fr.py --sparse   (the lane sums of the sparse matrix-vector product of csrc/sparse.hpp: analyse_sparse below)
    python tools/limb_bounds_fr.py --mle      (the folds, extrapolations, products and sums of csrc/mle.hpp: analyse_mle below)
    python tools/limb_bounds_fr.py --poseidon (the rounds of csrc/poseidon.hpp with the reductions its schedule sets: analyse_poseidon below)
    python tools/limb_bounds_fr.py --expr     (the stored form and the bound rule of the expression programs of csrc/expr.hpp: analyse_expr below)
"""
import sys

N, B = 9, 29
MASK = (1 << B) - 1
R = 1 << (N * B)
LEVELS = 10
FIELDS = {
    "Bls12_377_Fr29": 8444461749428370424248824938781546531375899335154063827935233455917409239041,
    "Bls12_381_Fr29": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
}


def limbs(x):
    return [(x >> (B * i)) & MASK for i in range(N - 1)] + [x >> (B * (N - 1))]


def bias4(r):
    v = limbs(4 * r)
    return [v[0] + (1 << B)] + [v[i] + (1 << B) - 1 for i in range(1, N - 1)] + [v[N - 1] - 1]


def columns(a, w, rl):
    """the largest value every column of fr_mul can reach for first-operand limb bounds a and second-operand limb bounds w"""
    cols, carry = [], 0
    for k in range(2 * N - 1):
        c = carry + sum(a[i] * w[k - i] for i in range(N) if 0 <= k - i < N)
        c += MASK * sum(rl[k - i] for i in range(N) if 1 <= k - i < N)
        if k < N:
            c += MASK          # m_k * r_0, r_0 = 1
        cols.append(c)
        carry = c >> B
    return cols


def carry_pass(l):
    return [MASK] + [MASK + (l[i - 1] >> B) for i in range(1, N - 1)] + [l[N - 1] + (l[N - 2] >> B)]


def analyse(name, r, out):
    rl = limbs(r)
    ok = True
    margins = []

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        margins.append((what, m))
        ok &= m > 0
        out.append("  %-58s %s (limit 2^%.2f, margin %.3e)" % (what, "ok " if m > 0 else "BAD", __import__("math").log2(limit), m))

    out.append("%s: r = %.3f * 2^252, R / r = %.2f" % (name, r / 2**252, R / r))
    top_m = (2 * r) >> (B * (N - 1))                      # the top limb of a class-M value
    class_m = [MASK] * (N - 1) + [top_m]
    w = [MASK] * (N - 1) + [rl[N - 1]]                    # a canonical table entry
    bias = bias4(r)
    margin("2r against a stored element (2^256)", 2 * r, 1 << 256)
    for i in range(N):
        margin("BIAS4 limb %d covers the limb of t" % i, class_m[i], bias[i] + 1)
    # the conversion of any 256-bit input: value < 2^256, the product below r + 2^256 r / R
    margin("input conversion: 2^256 against R", 1 << 256, R)
    margin("pointwise product: (2^256)^2 / R against r", (1 << 512) // R, r)
    a_l, val = list(class_m), 2                            # limb bounds and the value in units of r
    for lvl in range(LEVELS + 1):
        # every element is a product's first operand at this level (as b) or at the store
        margin("level %2d: value %3dr against R" % (lvl, val), val * r, R)
        margin("level %2d: largest limb against 2^31" % lvl, max(a_l), 1 << 31)
        margin("level %2d: largest column against 2^64" % lvl, max(columns(a_l, w, rl)), 1 << 64)
        if lvl == LEVELS:
            break
        s = [a_l[i] + class_m[i] for i in range(N)]
        d = [a_l[i] + bias[i] for i in range(N)]
        margin("level %2d: limb-wise sums against 2^32" % lvl, max(max(s), max(d)), 1 << 32)
        a_l = [max(x, y) for x, y in zip(carry_pass(s), carry_pass(d))]
        val += 4
    return ok


POLY_SCAN_LEVELS = 8     # a tile of csrc/poly.hpp has at most 256 lanes


def analyse_poly(name, r, out):
    """The chains of csrc/poly.hpp (python tools/limb_bounds_fr.py --poly): products of products (the runs, trees and scans of the
    batch inversion, the powers), Horner steps (a product plus an element, fed into the next product) and the sums of the LDS tree
    and scan (one class-M product more per level, one carry pass after it), carried exactly as the code performs them."""
    import math

    rl = limbs(r)
    ok = True

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        ok &= m > 0
        out.append("  %-66s %s (limit 2^%.2f, margin %.3e)" % (what, "ok " if m > 0 else "BAD", math.log2(limit), m))

    def first_operand(what, l, val, second):
        """an element with limb bounds l and value < val r as the first operand of fr_mul; the product must be class M again"""
        margin(what + ": value %dr against R" % val, val * r, R)
        margin(what + ": largest limb against 2^31", max(l), 1 << 31)
        margin(what + ": largest column against 2^64", max(columns(l, second, rl)), 1 << 64)
        sec_val = 2 * r if second is class_m else r
        margin(what + ": product r + a b / R against 2r", r + val * r * sec_val // R + 1, 2 * r)

    out.append("%s: r = %.3f * 2^252, R / r = %.2f  (the chains of poly.hpp)" % (name, r / 2**252, R / r))
    top_m = (2 * r) >> (B * (N - 1))
    class_m = [MASK] * (N - 1) + [top_m]
    w = [MASK] * (N - 1) + [rl[N - 1]]
    bias = bias4(r)
    margin("second operand: limbs of a class-M value against 2^29 + 8", max(class_m), (1 << B) + 8)
    # the batch inversion: nothing but class-M values multiplied together, to any depth (runs, trees, scans, x^(r - 2))
    first_operand("product of class-M by class-M", class_m, 2, class_m)
    # Horner: acc' = acc * z + c with z canonical and c class M, no carry pass in between
    horner = [class_m[i] + class_m[i] for i in range(N)]
    margin("Horner step: limb-wise sum against 2^32", max(horner), 1 << 32)
    first_operand("Horner step acc z + c as the next first operand", horner, 4, w)
    # the sums of the tree (evaluation) and of the suffix scan (division): v' = v + (a product), then one carry pass
    a_l, val = list(horner), 4
    for lvl in range(POLY_SCAN_LEVELS + 1):
        first_operand("tree / scan level %d: the element times a power of z" % lvl, a_l, val, w)
        if lvl == POLY_SCAN_LEVELS:
            break
        sm = [a_l[i] + class_m[i] for i in range(N)]
        margin("tree / scan level %d: limb-wise sum against 2^32" % lvl, max(sm), 1 << 32)
        margin("tree / scan level %d: top limb into the carry pass against 2^31" % lvl, sm[N - 1] + (sm[N - 2] >> B), 1 << 31)
        a_l = carry_pass(sm)
        val += 2
    # the division's last step: S = s_j (a Horner value) + z^(4 - j) * (scan value), carried, then converted or brought to class M
    fin = [horner[i] + class_m[i] for i in range(N)]
    margin("division finish: limb-wise sum against 2^32", max(fin), 1 << 32)
    first_operand("division finish S as the first operand of the conversion", carry_pass(fin), 6, w)
    # differences: tau - w^i (Lagrange), a - b, a*b - c: a class-M value + BIAS4 - a class-M value, one carry pass
    for i in range(N):
        margin("BIAS4 limb %d covers the limb of a class-M value" % i, class_m[i], bias[i] + 1)
    diff = [class_m[i] + bias[i] for i in range(N)]
    margin("difference: limb-wise sum against 2^32", max(diff), 1 << 32)
    first_operand("difference a + 4r - b as a first operand", carry_pass(diff), 7, w)
    # the element-wise sum
    first_operand("sum a + b as a first operand", carry_pass(horner), 4, w)
    return ok


def analyse_scan(name, r, out):
    """The chains of csrc/scan.hpp (python tools/limb_bounds_fr.py --scan).  The product scan multiplies class-M values only.  The sum
    scan adds limb-wise with one carry pass per step: a lane's run of four class-M elements, then tree or Hillis-Steele steps that
    each double the bound, with one product by 1 after every odd step; an offset (the carry into the tile plus a scan value) meets a
    prefix of the lane's run, and the result is converted.  The factors of the permutation product are sums of three, not carried."""
    import math

    rl = limbs(r)
    ok = True

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        ok &= m > 0
        out.append("  %-74s %s (limit 2^%.2f, margin %.3e)" % (what, "ok " if m > 0 else "BAD", math.log2(limit), m))

    top_m = (2 * r) >> (B * (N - 1))
    class_m = [MASK] * (N - 1) + [top_m]
    w = [MASK] * (N - 1) + [rl[N - 1]]

    def first_operand(what, l, val, second):
        margin(what + ": value %dr against R" % val, val * r, R)
        margin(what + ": largest limb against 2^31", max(l), 1 << 31)
        margin(what + ": largest column against 2^64", max(columns(l, second, rl)), 1 << 64)
        sec_val = 2 * r if second is class_m else r
        margin(what + ": product r + a b / R against 2r", r + val * r * sec_val // R + 1, 2 * r)

    def add(what, a, b):
        sm = [x + y for x, y in zip(a, b)]
        margin(what + ": limb-wise sum against 2^32", max(sm), 1 << 32)
        margin(what + ": top limb into the carry pass against 2^31", sm[N - 1] + (sm[N - 2] >> B), 1 << 31)
        return carry_pass(sm)

    out.append("%s: r = %.3f * 2^252, R / r = %.2f  (the chains of scan.hpp)" % (name, r / 2**252, R / r))
    margin("second operand: limbs of a class-M value against 2^29 + 8", max(class_m), (1 << B) + 8)
    first_operand("product scan: class-M by class-M, to any depth", class_m, 2, class_m)
    # the lane's run: three sums of a running value and a class-M element; prefix[j] is what the way down keeps
    run_l, run_v = list(class_m), 2
    for j in range(1, 4):
        run_l = add("sum scan, lane run element %d" % j, run_l, class_m)
        run_v += 2
    # tree (way up) and Hillis-Steele (way down) steps: both operands carry the bound of the step before
    a_l, a_v = run_l, run_v
    worst_l, worst_v = a_l, a_v
    for s in range(POLY_SCAN_LEVELS):
        a_l = add("sum scan step %d" % s, a_l, a_l)
        a_v *= 2
        if s & 1:
            first_operand("sum scan step %d: the product by 1 of an odd step" % s, a_l, a_v, w)
            a_l, a_v = list(class_m), 2
        if a_v > worst_v:
            worst_l, worst_v = a_l, a_v
        worst_l = [max(x, y) for x, y in zip(worst_l, a_l)]
    # what the scan leaves after any number of steps, as the tile total (a product by 1) and as the lane to the left
    first_operand("sum scan: a total brought to class M", worst_l, worst_v, w)
    off_l = add("sum scan offset: carry into the tile + scan value", class_m, worst_l)
    off_v = 2 + worst_v
    y_l = add("sum scan output: offset + prefix of the run", off_l, run_l)
    first_operand("sum scan output as the first operand of the conversion", y_l, off_v + run_v, w)
    # the permutation product: (w + gamma) + beta * id, two class-M values and a canonical one, no carry pass
    t = [class_m[i] + class_m[i] + w[i] for i in range(N)]
    margin("permutation product factor: limb-wise sum against 2^32", max(t), 1 << 32)
    first_operand("permutation product factor w + beta id + gamma times the running product", t, 5, class_m)
    return ok


LINCOMB_COLUMNS = 32    # LINCOMB_MAX_COLUMNS of csrc/quotient.hpp


def analyse_quotient(name, r, out):
    """The chains of csrc/quotient.hpp (python tools/limb_bounds_fr.py --quotient), carried exactly as quot_row performs them.  The gate
    accumulator starts as q_c + pi; every iteration of the column loop adds two class-M products (q_lc w, q_hash w^5) and at odd columns a
    third (q_mul w w'), then one carry pass; the fifth column adds q_ecc w0..w4, carries, subtracts q_o w4 (+ 4r) and carries; t_perm1,
    one class-M product, is added and the sum is the first operand of the product by 1 / Z_H.  The linear combination adds one class-M
    product per column with a carry pass after each.  The largest column of every product must stay below 2^64."""
    import math

    rl = limbs(r)
    ok = True
    worst_col = 0

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        ok &= m > 0
        out.append("  %-78s %s (limit 2^%.2f, margin %.3e)" % (what, "ok " if m > 0 else "BAD", math.log2(limit), m))

    top_m = (2 * r) >> (B * (N - 1))
    class_m = [MASK] * (N - 1) + [top_m]
    w = [MASK] * (N - 1) + [rl[N - 1]]
    bias = bias4(r)

    def first_operand(what, l, val, second):
        nonlocal worst_col
        col = max(columns(l, second, rl))
        worst_col = max(worst_col, col)
        margin(what + ": value %dr against R" % val, val * r, R)
        margin(what + ": largest limb against 2^31", max(l), 1 << 31)
        margin(what + ": largest column against 2^64", col, 1 << 64)
        sec_val = 2 * r if second is class_m else r
        margin(what + ": product r + a b / R against 2r", r + val * r * sec_val // R + 1, 2 * r)

    def add(what, a, b, carry=True):
        sm = [x + y for x, y in zip(a, b)]
        margin(what + ": limb-wise sum against 2^32", max(sm), 1 << 32)
        if not carry:
            return sm
        margin(what + ": top limb into the carry pass against 2^31", sm[N - 1] + (sm[N - 2] >> B), 1 << 31)
        return carry_pass(sm)

    out.append("%s: r = %.3f * 2^252, R / r = %.2f  (the chains of quotient.hpp)" % (name, r / 2**252, R / r))
    margin("second operand: limbs of a class-M value against 2^29 + 8", max(class_m), (1 << B) + 8)
    first_operand("products of loaded values, wires and their powers: class-M by class-M", class_m, 2, class_m)
    for i in range(N):
        margin("BIAS4 limb %d covers the limb of a class-M value" % i, class_m[i], bias[i] + 1)
    # x - 1 (the first kernel) and z[i] - 1: a class-M value + BIAS4 - a class-M value, one carry pass, then a product
    diff = add("difference x - 1, z - 1, num - den", class_m, bias)
    first_operand("difference as a first operand (conversion, alpha^2 / (n (x - 1)), alpha)", diff, 6, class_m)
    # the permutation factors, as in scan.hpp
    t = [class_m[i] + class_m[i] + w[i] for i in range(N)]
    margin("permutation factor: limb-wise sum against 2^32", max(t), 1 << 32)
    first_operand("permutation factor w + beta k x + gamma times the running product", t, 5, class_m)
    # the gate
    acc, val = add("gate: q_c + pi", class_m, class_m, carry=False), 4
    for j in range(4):
        acc = add("gate column %d: + q_lc w" % j, acc, class_m, carry=False)
        acc = add("gate column %d: + q_hash w^5" % j, acc, class_m, carry=j % 2 == 0)
        val += 4
        if j % 2:
            acc = add("gate column %d: + q_mul w w'" % j, acc, class_m)
            val += 2
    acc = add("gate column 4: + q_ecc w0 w1 w2 w3 w4", acc, class_m)
    val += 2
    acc = add("gate column 4: - q_o w4 (+ 4r)", acc, bias)
    val += 4
    acc = add("gate + t_perm1", acc, class_m, carry=False)
    val += 2
    first_operand("gate + t_perm1 times 1 / Z_H", acc, val, w)
    fin = add("(..) / Z_H + t_perm2", class_m, class_m, carry=False)
    first_operand("the row as the first operand of the conversion", fin, 4, w)
    # the linear combination
    acc, val = [0] * N, 0
    for j in range(LINCOMB_COLUMNS):
        acc = add("linear combination, column %2d" % j, acc, class_m)
        val += 2
    first_operand("linear combination of %d columns as the first operand of the conversion" % LINCOMB_COLUMNS, acc, val, w)
    margin("the chain's largest column against 2^64", worst_col, 1 << 64)
    return ok


SPARSE_ENTRIES = 16     # SPARSE_E of csrc/sparse.hpp: the entries a lane sums before it reduces


def analyse_sparse(name, r, out):
    """The chains of csrc/sparse.hpp (python tools/limb_bounds_fr.py --sparse), carried exactly as sparse_total and sparse_rows_lane
    perform them.  z is converted once (any 256-bit input times a canonical constant) and every entry is one product of that class-M
    value by a canonical coefficient.  A lane adds SPARSE_ENTRIES such products, with one carry pass after each: `loc` from zero, `run`
    from the class-M value of a canonical prefix.  Either sum is then the first operand of a product by a canonical constant (the
    conversion on the way out, the product by 1 into bstart / bend).  A row that crosses lanes is bend + BIAS4 - bstart, carried and
    converted.  The largest column of every product must stay below 2^64."""
    import math

    rl = limbs(r)
    ok = True
    worst_col = 0

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        ok &= m > 0
        out.append("  %-78s %s (limit 2^%.2f, margin %.3e)" % (what, "ok " if m > 0 else "BAD", math.log2(limit), m))

    top_m = (2 * r) >> (B * (N - 1))
    class_m = [MASK] * (N - 1) + [top_m]
    w = [MASK] * (N - 1) + [rl[N - 1]]
    any256 = [MASK] * (N - 1) + [(1 << (256 - B * (N - 1))) - 1]
    bias = bias4(r)

    def first_operand(what, l, val, second):
        nonlocal worst_col
        col = max(columns(l, second, rl))
        worst_col = max(worst_col, col)
        margin(what + ": value %dr against R" % val, val * r, R)
        margin(what + ": largest limb against 2^31", max(l), 1 << 31)
        margin(what + ": largest column against 2^64", col, 1 << 64)
        sec_val = 2 * r if second is class_m else r
        margin(what + ": product r + a b / R against 2r", r + val * r * sec_val // R + 1, 2 * r)

    def add(what, a, b):
        sm = [x + y for x, y in zip(a, b)]
        margin(what + ": limb-wise sum against 2^32", max(sm), 1 << 32)
        margin(what + ": top limb into the carry pass against 2^31", sm[N - 1] + (sm[N - 2] >> B), 1 << 31)
        return carry_pass(sm)

    out.append("%s: r = %.3f * 2^252, R / r = %.2f  (the chains of sparse.hpp, %d entries a lane)" % (name, r / 2**252, R / r, SPARSE_ENTRIES))
    margin("2r against a packed element (2^256)", 2 * r, 1 << 256)
    first_operand("z or a coefficient on the way in: any 256-bit value times a canonical constant", any256, -(-(1 << 256) // r), w)
    first_operand("an entry: z in class M times a canonical coefficient", class_m, 2, w)
    loc, run, lv, rv = [0] * N, list(class_m), 0, 2
    for e in range(SPARSE_ENTRIES):
        loc = add("loc, entry %2d" % e, loc, class_m)
        run = add("run, entry %2d (from a canonical prefix in class M)" % e, run, class_m)
        lv += 2
        rv += 2
    first_operand("a lane total or a row inside a lane as the first operand of the conversion", loc, lv, w)
    first_operand("the running sum as the first operand of the product by 1 (bstart, bend)", run, rv, w)
    for i in range(N):
        margin("BIAS4 limb %d covers the limb of bstart" % i, class_m[i], bias[i] + 1)
    diff = add("a crossing row: bend + 4r - bstart", class_m, bias)
    first_operand("a crossing row as the first operand of the conversion", diff, 6, w)
    margin("the chain's largest column against 2^64", worst_col, 1 << 64)
    out.append("  largest column: %d = 2^%.3f" % (worst_col, math.log2(worst_col)))
    return ok


MLE_POINTS, MLE_TERMS, MLE_FACTORS = 4, 8, 5     # MLE_PTS, MLE_MAX_TERMS, MLE_MAX_FACTORS of csrc/mle.hpp
MLE_TREE_LEVELS, MLE_TREE_REDUCE = 8, 4           # a block tree has at most 256 lanes and multiplies by 1 after its fourth level


def analyse_mle(name, r, out):
    """The chains of csrc/mle.hpp (python tools/limb_bounds_fr.py --mle), carried exactly as the code performs them.  The lazy value is
    always the FIRST operand of a product; the second is a canonical constant or, inside a term, the running product in class M
    (normalised, below 2r) -- so that product is judged with a class-M second operand: r + a b / R must stay below 2r.
      the fold            (1 - r) x + r y: two products by canonical constants, one limb-wise sum (below 4r, limbs below 2^30), which is
                          the first operand of the next level's products, of the conversion on the way out, or of nothing else.
      the extrapolation   lo, hi in class M; diff = hi + BIAS4 - lo, one carry pass; e_2 = hi + diff, e_3 = e_2 + diff, one carry
                          pass, e_4, e_5.
      a term              P starts as the canonical coefficient; factor by factor P = fr_mul(e_t, P).
      the sums            MLE_POINTS * MLE_TERMS class-M products into a lane accumulator, one carry pass each; the product by 1; the
                          block tree with a carry pass per level and the product by 1 after its fourth level."""
    import math

    rl = limbs(r)
    ok = True
    worst_col = 0

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        ok &= m > 0
        out.append("  %-86s %s (limit 2^%.2f, margin %.3e)" % (what, "ok " if m > 0 else "BAD", math.log2(limit), m))

    top_m = (2 * r) >> (B * (N - 1))
    class_m = [MASK] * (N - 1) + [top_m]
    w = [MASK] * (N - 1) + [rl[N - 1]]
    any256 = [MASK] * (N - 1) + [(1 << (256 - B * (N - 1))) - 1]
    bias = bias4(r)

    def first_operand(what, l, val, second):
        """val: the value bound in units of r (a fraction for a raw input); second: w (canonical) or class_m"""
        nonlocal worst_col
        col = max(columns(l, second, rl))
        worst_col = max(worst_col, col)
        margin(what + ": value %.1fr against R" % val, int(val * r), R)
        margin(what + ": largest limb against 2^31", max(l), 1 << 31)
        margin(what + ": largest column against 2^64", col, 1 << 64)
        sec_val = 2 * r if second is class_m else r
        margin(what + ": product r + a b / R against 2r", r + int(val * r) * sec_val // R + 1, 2 * r)

    def add(what, a, b, carry=True):
        sm = [x + y for x, y in zip(a, b)]
        margin(what + ": limb-wise sum against 2^32", max(sm), 1 << 32)
        if not carry:
            return sm
        margin(what + ": top limb into the carry pass against 2^31", sm[N - 1] + (sm[N - 2] >> B), 1 << 31)
        return carry_pass(sm)

    raw = (1 << 256) / r
    out.append("%s: r = %.3f * 2^252, R / r = %.2f  (the chains of mle.hpp: %d points a lane, %d terms of %d factors)"
               % (name, r / 2**252, R / r, MLE_POINTS, MLE_TERMS, MLE_FACTORS))
    margin("2r against a packed element (2^256)", 2 * r, 1 << 256)
    first_operand("an element or a pair on the way in: any 256-bit value times a canonical constant", any256, raw, w)
    # the fold
    lazy = add("the fold (1 - r) x + r y: two class-M products", class_m, class_m, carry=False)
    first_operand("the fold (1 - r) x + r y as the first operand of the next level or of the conversion", lazy, 4, w)
    # the extrapolation
    for i in range(N):
        margin("BIAS4 limb %d covers the limb of lo" % i, class_m[i], bias[i] + 1)
    diff = add("diff = hi + 4r - lo", class_m, bias)
    e, val = list(class_m), 2                     # e_1 = hi
    first_operand("e_0 = lo, e_1 = hi against the running product", e, val, class_m)
    for t in range(2, MLE_FACTORS + 1):
        e = add("e_%d = e_%d + diff" % (t, t - 1), e, diff, carry=False)
        val += 6
        first_operand("e_%d against the running product" % t, e, val, class_m)
        if t == 3:
            margin("e_3: top limb into the carry pass against 2^31", e[N - 1] + (e[N - 2] >> B), 1 << 31)
            e = carry_pass(e)
    for k in range(1, MLE_FACTORS + 1):
        # every factor meets a class-M running product (the first one the canonical coefficient, which is smaller)
        first_operand("factor %d of a term at t = %d" % (k, MLE_FACTORS), e, val, class_m)
    # the sums
    acc, av = [0] * N, 0
    for i in range(1, MLE_POINTS * MLE_TERMS + 1):
        acc = add("the lane accumulator, add %2d" % i, acc, class_m)
        av += 2
    first_operand("the lane accumulator as the first operand of the product by 1", acc, av, w)
    node, nv = list(class_m), 2
    for lvl in range(1, MLE_TREE_LEVELS + 1):
        node = add("the block tree, level %d" % lvl, node, node)
        nv *= 2
        if lvl == MLE_TREE_REDUCE:
            first_operand("the block tree after level %d as the first operand of the product by 1" % lvl, node, nv, w)
            node, nv = list(class_m), 2
    first_operand("the block sum as the first operand of the product by 1", node, nv, w)
    rows = add("a lane of a further level: four class-M rows", add("two rows", class_m, class_m), add("two rows", class_m, class_m))
    first_operand("a lane of a further level as the first operand of the product by 1", rows, 8, w)
    margin("the chain's largest column against 2^64", worst_col, 1 << 64)
    out.append("  largest column: %d = 2^%.3f" % (worst_col, math.log2(worst_col)))
    return ok


POSEIDON_SETS = ((17, 8, 31), (5, 6, 11), (3, 2, 120))      # alpha, full and partial rounds: snarkVM's, a short one, a long lazy chain


def poseidon_schedule(t, alpha, rf, rp, sparse, K):
    """pos_schedule of csrc/poseidon.hpp, statement by statement in the same double arithmetic: (reductions per round, products)"""
    h, rounds = rf // 2, rf + rp
    sq_limit, lazy_limit, leave = 0.95 * K, 0.9 * K, t * (1 + 2 / K)
    top = alpha.bit_length() - 1
    sbox_products = sum(1 + ((alpha >> b) & 1) for b in range(top))
    b = [leave + 2] * t
    red, products = [0] * rounds, 0
    for r in range(rounds):
        full = r < h or r >= h + rp
        flags = 0
        if full or not sparse:
            nsb = t if full else 1
            for e in range(nsb):
                if (b[e] + 1) * (b[e] + 1) >= sq_limit:
                    flags |= 1
            total = 0.0
            for e in range(t):
                x = b[e] + 1
                if x >= lazy_limit:
                    return None
                if e < nsb:
                    if flags & 1:
                        x = 1 + x / K
                    if x * x >= sq_limit:
                        return None
                    x = 1 + 2 * x / K
                total += 1 + x / K
            products += nsb * (sbox_products + (flags & 1)) + t * t
            b = [total] * t
        else:
            for e in range(1, t):
                if b[e] + 3 >= lazy_limit:
                    flags |= 2
            x0 = b[0] + 1
            if x0 >= lazy_limit:
                return None
            if x0 * x0 >= sq_limit:
                flags |= 1
                x0 = 1 + x0 / K
            sb = 1 + 2 * x0 / K
            out0 = 1 + sb / K
            for e in range(1, t):
                y = b[e]
                if flags & 2:
                    y = 1 + y / K
                y += 1
                out0 += 1 + y / K
                b[e] = y + 1 + sb / K
                if b[e] >= lazy_limit:
                    return None
            b[0] = out0
            products += sbox_products + (flags & 1) + (2 * t - 1) + ((t - 1) if flags & 2 else 0)
        red[r] = flags
    if any(x > leave for x in b):
        return None
    return red, products


def analyse_poseidon(name, r, out):
    """The rounds of csrc/poseidon.hpp (python tools/limb_bounds_fr.py --poseidon) for every state width t = 2 .. 9, both forms of the
    partial rounds and the parameter sets above, carried as pos_permute performs them with the reductions pos_schedule sets -- here in
    exact integers: a value bound per state element, limbs in the carried form (fr_carry: limbs 0 .. 7 below 2^29 + 8, the top limb
    holds the rest).  Every product is judged as fr_mul judges it: the first operand below R with limbs below 2^31, the second carried,
    every column below 2^64, and the result r + a b / R below 2r (class M).  The state enters a permutation below what the last linear
    layer leaves plus an absorbed class-M element and must leave below that again."""
    import math

    rl = limbs(r)
    ok = True
    K = float(R) / float(r)
    worst = {}
    col_memo = {}          # by the two top limbs: the other limbs are the same bounds everywhere

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        ok &= m > 0
        if what not in worst or m < worst[what][0]:
            worst[what] = (m, have, limit)

    canon = [MASK] * (N - 1) + [rl[N - 1]]

    def lazy_limbs(val):
        return [MASK + 8] * (N - 1) + [(val >> (B * (N - 1))) + 1]

    def mul(what, a_val, b_val, b_limbs):
        a = lazy_limbs(a_val)
        margin(what + ": the first operand against R", a_val, R)
        margin(what + ": its largest limb against 2^31", max(a), 1 << 31)
        margin(what + ": the second operand's largest limb against 2^29 + 8", max(b_limbs), (1 << B) + 8)
        key = (a[N - 1], b_limbs[N - 1])
        if key not in col_memo:
            col_memo[key] = max(columns(a, b_limbs, rl))
        margin(what + ": the largest column against 2^64", col_memo[key], 1 << 64)
        res = r + a_val * b_val // R + 1
        margin(what + ": the result r + a b / R against 2r", res, 2 * r)
        return res

    def add(what, a_val, b_val):
        # carried + normalised limbs, then one carry pass
        margin(what + ": limb-wise sum against 2^32", 2 * MASK + 8, 1 << 32)
        margin(what + ": top limb into the carry pass against 2^31", ((a_val + b_val) >> (B * (N - 1))) + 2, 1 << 31)
        return a_val + b_val

    def sbox(x, alpha):
        top = alpha.bit_length() - 1
        acc = x
        for b in range(top - 1, -1, -1):
            acc = mul("the first square of an S-box" if acc is x and b == top - 1 else "a later square of an S-box", acc, acc, lazy_limbs(acc))
            if (alpha >> b) & 1:
                acc = mul("x times the running power of an S-box", x, acc, lazy_limbs(acc))
        return acc

    out.append("%s: r = %.3f * 2^252, R / r = %.2f  (the rounds of poseidon.hpp)" % (name, r / 2**252, K))
    margin("2r against a packed element (2^256)", 2 * r, 1 << 256)
    mul("an absorbed element: any 256-bit value times a canonical constant", (1 << 256) - 1, r, canon)
    for alpha, rf, rp in POSEIDON_SETS:
        for t in range(2, 10):
            counts = []
            for sparse in (False, True):
                sch = poseidon_schedule(t, alpha, rf, rp, sparse, K)
                if sch is None:
                    ok = False
                    out.append("  t = %d, alpha %d, %d + %d rounds, %s: NO SCHEDULE  BAD" % (t, alpha, rf, rp, "sparse" if sparse else "dense"))
                    continue
                red, products = sch
                counts.append((products, sum(1 for f in red if f)))
                h = rf // 2
                leave = int(t * (1 + 2 / K) * r) + 1
                b = [leave + 2 * r] * t
                for k in range(rf + rp):
                    full = k < h or k >= h + rp
                    if full or not sparse:
                        nsb = t if full else 1
                        nb = 0
                        for e in range(t):
                            x = add("state + round constant", b[e], r)
                            if e < nsb:
                                if red[k] & 1:
                                    x = mul("an S-box input times 1", x, r, canon)
                                x = sbox(x, alpha)
                            nb += mul("a matrix entry times a state element", x, r, canon)
                        for _ in range(t):
                            add("the sum of a matrix row", nb, 0)
                        b = [nb] * t
                    else:
                        x = add("state + round constant", b[0], r)
                        if red[k] & 1:
                            x = mul("an S-box input times 1", x, r, canon)
                        sb = sbox(x, alpha)
                        out0 = mul("N00 times the S-box output", sb, r, canon)
                        for e in range(1, t):
                            y = b[e]
                            if red[k] & 2:
                                y = mul("an element that skipped the products, times 1", y, r, canon)
                            y = add("state + round constant", y, r)
                            out0 = add("the sum out_0", out0, mul("v^_j times a lazy element", y, r, canon))
                            b[e] = add("out_i = w_i s_0 + s_i", y, mul("w_i times the S-box output", sb, r, canon))
                        b[0] = out0
                margin("the state at the end of a permutation against what the next one assumes", max(b), leave + 1)
                mul("a squeezed element times the conversion constant", max(b) + 2 * r, r, canon)
            if len(counts) == 2:
                out.append("  t = %d, alpha %2d, %d + %4d rounds: products per permutation %5d dense (%d rounds with a reduction), %5d sparse (%d)"
                           % (t, alpha, rf, rp, counts[0][0], counts[0][1], counts[1][0], counts[1][1]))
    for what, (m, have, limit) in worst.items():
        out.append("  %-80s %s (worst 2^%.3f, limit 2^%.3f)" % (what, "ok " if m > 0 else "BAD", math.log2(max(have, 1)), math.log2(limit)))
    return ok


def analyse_expr(name, r, out):
    """The stored form of csrc/expr.hpp (python tools/limb_bounds_fr.py --expr).  Every operand of an instruction is a 256-bit integer
    unpacked into normalised limbs, so the products need nothing from the compiler: ANY two 256-bit values give a class-M product.  What
    the compiler has to keep is the 2^256 of the stored form: it carries value <= B r per node, B <= LIM = 2^32 / (top word of r + 1),
    a little below 2^256 / r.  Printed: LIM, the rule for every instruction, and the reductions it leads to in small cases."""
    import math

    rl = limbs(r)
    ok = True

    def margin(what, have, limit):
        nonlocal ok
        m = limit - have
        ok &= m > 0
        out.append("  %-82s %s (limit 2^%.2f, margin %.3e)" % (what, "ok " if m > 0 else "BAD", math.log2(limit), m))

    lim = float(1 << 32) / ((r >> 224) + 1)
    K = 32 * lim
    out.append("%s: r = %.3f * 2^252, 2^256 / r = %.4f, LIM = %.4f, R / r = %.2f, 32 LIM = %.2f  (the programs of expr.hpp)"
               % (name, r / 2**252, 2.0**256 / r, lim, R / r, K))
    any256 = [MASK] * (N - 1) + [(1 << (256 - B * (N - 1))) - 1]
    margin("LIM r against the stored form (2^256)", int(lim * r), 1 << 256)
    margin("a product of any two stored values: largest column against 2^64", max(columns(any256, any256, rl)), 1 << 64)
    margin("a product of any two stored values: r + a b / R against 2r", r + (((1 << 256) - 1) ** 2) // R + 1, 2 * r)
    margin("a column operand: r + 2^256 r / R against 2r (then one conditional subtraction: below r)", r + ((1 << 256) * r) // R + 1, 2 * r)
    margin("the result: any stored value times the conversion constant, r + a r / R against 2r", r + ((1 << 256) * r) // R + 1, 2 * r)
    margin("two canonical leaves added: 2r against LIM r", 2 * r, int(lim * r))
    margin("SUB of canonical operands: r + r - 0 against LIM r", 2 * r, int(lim * r))
    out.append("  rule: MUL, SQR  B = 1 + B_a B_b / (32 LIM)   (at most 1 + LIM / 32 = %.4f)" % (1 + lim / 32))
    out.append("        ADD       B = B_a + B_b;   SUB, NEG  B = B_a + ceil(B_b);   each must stay <= LIM = %.4f" % lim)
    out.append("        else reduce an operand in place: B <= 3: one conditional subtraction, B -> max(1, B - 1); B > 3: a product by one, B -> 1 + B / (32 LIM)")
    prod = 1 + 1 / K
    out.append("  a product of canonical operands: %.4f; product + product: %.4f (%s); (product + product) + product: %.4f (%s)"
               % (prod, 2 * prod, "fits" if 2 * prod <= lim else "one reduction", 3 * prod, "fits" if 3 * prod <= lim else "one reduction"))
    b, steps = 1.0, 0
    while 2 * b <= lim:
        b, steps = 2 * b, steps + 1
    out.append("  a doubling chain a = a + a from a canonical leaf runs %d steps before its first reduction" % steps)
    return ok


def main():
    out = []
    if "--expr" in sys.argv[1:]:
        ok = all([analyse_expr(name, r, out) for name, r in FIELDS.items()])
        print("\n".join(out))
        print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
        return 0 if ok else 1
    if "--poseidon" in sys.argv[1:]:
        ok = all([analyse_poseidon(name, r, out) for name, r in FIELDS.items()])
        print("\n".join(out))
        print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
        return 0 if ok else 1
    if "--mle" in sys.argv[1:]:
        ok = all([analyse_mle(name, r, out) for name, r in FIELDS.items()])
        print("\n".join(out))
        print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
        return 0 if ok else 1
    if "--sparse" in sys.argv[1:]:
        ok = all([analyse_sparse(name, r, out) for name, r in FIELDS.items()])
        print("\n".join(out))
        print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
        return 0 if ok else 1
    if "--quotient" in sys.argv[1:]:
        ok = all([analyse_quotient(name, r, out) for name, r in FIELDS.items()])
        print("\n".join(out))
        print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
        return 0 if ok else 1
    if "--scan" in sys.argv[1:]:
        ok = all([analyse_scan(name, r, out) for name, r in FIELDS.items()])
        print("\n".join(out))
        print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
        return 0 if ok else 1
    if "--poly" in sys.argv[1:]:
        ok = all([analyse_poly(name, r, out) for name, r in FIELDS.items()])
        print("\n".join(out))
        print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
        return 0 if ok else 1
    ok = all([analyse(name, r, out) for name, r in FIELDS.items()])
    print("\n".join(out))
    print("all margins positive" if ok else "A MARGIN IS NOT POSITIVE")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
