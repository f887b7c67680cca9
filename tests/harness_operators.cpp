// Runs every class of include/mi355_msm.hpp on the device, one family of wrappers per process: `harness_operators <family> <dir>`.
// Built and run by tests/test_harness_operators.py, which writes the inputs (tests/operator_cases.py) and judges the outputs.
//
// <dir>/case.txt holds `key value` lines: the integers of the case and, as `expect.<label>`, what a guarded call must do -- `returns`
// (the default), `invalid_argument`, `runtime_error`, or `MsmError:<code>`, each optionally followed by ` | <phrase>`, words the
// exception's message must contain (the name of the vector at fault), so that no label is satisfied by another branch.  Every other
// input is a raw little-endian file <dir>/<name>; every result is written to a file of its own.  NO VALUE IS COMPARED HERE: expected
// values never pass through the code under test.  The exit status is 0 when every guarded call behaved as the case said; `ran <wrapper>`
// is printed once a wrapper has returned, and `refused <label> <kind> | <message>` when a guarded call threw.  Plain g++, no HIP
// headers: the device memory check_bases_device and multi_scalar_mult_async need comes from the HIP library by name, as in
// harness_msm_correctness.cpp.
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "mi355_msm.hpp"

using namespace mi355;
typedef BigInteger256 Fr;
typedef std::vector<Fr> FrVec;
typedef Radix2EvaluationDomain Domain;

static std::string DIR;
static std::map<std::string, std::string> CFG;
static std::set<std::string> RAN;
static int BAD = 0;

static void ran(const char* wrapper) {
  if (RAN.insert(wrapper).second) printf("ran %s\n", wrapper);
}

template <class T>
static std::vector<T> rd(const std::string& name) {
  const std::string path = DIR + "/" + name;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error(path + ": cannot open");
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (bytes < 0 || (size_t)bytes % sizeof(T)) {
    fclose(f);
    throw std::runtime_error(path + ": not a whole number of records");
  }
  std::vector<T> v((size_t)bytes / sizeof(T));
  const size_t got = v.empty() ? 0 : fread(v.data(), sizeof(T), v.size(), f);
  fclose(f);
  if (got != v.size()) throw std::runtime_error(path + ": short read");
  return v;
}
static Fr rd1(const std::string& name) { return rd<Fr>(name).at(0); }

static void wr_raw(const std::string& name, const void* p, size_t bytes) {
  const std::string path = DIR + "/" + name;
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) {
    if (f) fclose(f);
    throw std::runtime_error(path + ": cannot write");
  }
  fclose(f);
}
template <class T>
static void wr(const std::string& name, const std::vector<T>& v) { wr_raw(name, v.data(), v.size() * sizeof(T)); }
static void wr(const std::string& name, const Fr& v) { wr_raw(name, &v, sizeof v); }
static void wr(const std::string& name, const G1Projective& v) { wr_raw(name, &v, sizeof v); }
static void wr_u64(const std::string& name, std::vector<uint64_t> v) { wr(name, v); }

static long num(const std::string& key) {
  auto it = CFG.find(key);
  if (it == CFG.end()) throw std::runtime_error("case.txt: no " + key);
  return std::stol(it->second);
}

// run f; compare what it did with expect.<label>; true when it returned
template <class F>
static bool guarded(const std::string& label, F&& f) {
  auto it = CFG.find("expect." + label);
  std::string want = it == CFG.end() ? "returns" : it->second, phrase;
  const size_t bar = want.find(" | ");
  if (bar != std::string::npos) {
    phrase = want.substr(bar + 3);
    want.resize(bar);
  }
  std::string did = "returns", note;
  try {
    f();
  } catch (const MsmError& e) {
    did = "MsmError:" + std::to_string(e.code);
    note = e.what();
    if (note.empty() || note.find("(no message)") != std::string::npos) did += ":no-message";
  } catch (const std::invalid_argument& e) {
    did = "invalid_argument";
    note = e.what();
    if (note.empty()) did += ":no-message";
  } catch (const std::runtime_error& e) {
    did = "runtime_error";
    note = e.what();
  }
  if (did != "returns") printf("refused %s %s | %s\n", label.c_str(), did.c_str(), note.c_str());
  if (did != want || note.find(phrase) == std::string::npos) {
    fprintf(stderr, "%s: expected %s with \"%s\" in its message, got %s %s\n", label.c_str(), want.c_str(), phrase.c_str(), did.c_str(), note.c_str());
    BAD++;
  }
  return did == "returns";
}

// ---- the HIP runtime by name ----------------------------------------------------------------------------------------------------------------
struct Hip {
  typedef int (*malloc_t)(void**, size_t);
  typedef int (*memcpy_t)(void*, const void*, size_t, int);
  typedef int (*free_t)(void*);
  malloc_t malloc_ = nullptr;
  memcpy_t memcpy_ = nullptr;
  free_t free_ = nullptr;
  Hip() {
    void* h = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) throw std::runtime_error("libamdhip64.so: cannot load");
    malloc_ = (malloc_t)dlsym(h, "hipMalloc");
    memcpy_ = (memcpy_t)dlsym(h, "hipMemcpy");
    free_ = (free_t)dlsym(h, "hipFree");
    if (!malloc_ || !memcpy_ || !free_) throw std::runtime_error("libamdhip64.so: hipMalloc / hipMemcpy / hipFree not found");
  }
  void* upload(const void* host, size_t bytes) {
    void* d = nullptr;
    if (malloc_(&d, bytes ? bytes : 4) != 0) throw std::runtime_error("hipMalloc failed");
    if (bytes && memcpy_(d, host, bytes, 1 /* hipMemcpyHostToDevice */) != 0) {
      free_(d);
      throw std::runtime_error("hipMemcpy failed");
    }
    return d;
  }
};

// ---- the families ---------------------------------------------------------------------------------------------------------------------------
static std::unique_ptr<Domain> make_domain(size_t num_coeffs, int curve) {
  std::unique_ptr<Domain> first;
  if (!guarded("create", [&] { first.reset(new Domain(num_coeffs, curve)); })) return nullptr;
  // every object is moved once and used through the new name; the moved-from destructor must do nothing
  std::unique_ptr<Domain> dom(new Domain(std::move(*first)));
  first.reset();
  ran("Radix2EvaluationDomain");
  return dom;
}

static void transforms(int curve) {
  auto dom = make_domain((size_t)num("num_coeffs"), curve);
  if (!dom) return;
  const FrVec v = rd<Fr>("v"), too_long = rd<Fr>("too_long");
  wr_u64("size", {dom->size(), dom->query("log_size")});
  ran("size");
  ran("query");
  wr("element", dom->element((uint64_t)num("element")));
  ran("element");
  wr("fft", dom->fft(v));
  ran("fft");
  wr("ifft", dom->ifft(v));
  ran("ifft");
  wr("coset_fft", dom->coset_fft(v));
  ran("coset_fft");
  wr("coset_ifft", dom->coset_ifft(v));
  ran("coset_ifft");
  guarded("transform_too_long", [&] { dom->fft(too_long); });
  guarded("query_unknown", [&] { dom->query("no such key"); });
  wr("fft_again", dom->fft(v));
}

static void vecops(int curve) {
  auto dom = make_domain(64, curve);
  if (!dom) return;
  const FrVec a = rd<Fr>("a"), b = rd<Fr>("b"), c = rd<Fr>("c"), shorter = rd<Fr>("shorter"), inv_in = rd<Fr>("inv_in");
  const Fr s = rd1("s"), coeff = rd1("coeff");
  wr("mul", dom->mul(a, b));
  ran("mul");
  wr("add", dom->add(a, b));
  ran("add");
  wr("sub", dom->sub(a, b));
  ran("sub");
  wr("mul_sub", dom->mul_sub(a, b, c));
  ran("mul_sub");
  wr("scale", dom->scale(a, s));
  ran("scale");
  wr("batch_inversion", dom->batch_inversion(inv_in));
  ran("batch_inversion");
  wr("batch_inversion_and_mul", dom->batch_inversion_and_mul(inv_in, &coeff));
  ran("batch_inversion_and_mul");
  const std::vector<FrVec> cols = {rd<Fr>("lc0"), rd<Fr>("lc1"), rd<Fr>("lc2")};
  const FrVec lc_coeffs = rd<Fr>("lc_coeffs");
  wr("linear_combination", dom->linear_combination(cols, lc_coeffs));
  ran("linear_combination");
  guarded("mul_unequal", [&] { dom->mul(a, shorter); });
  guarded("mul_unequal_first", [&] { dom->mul(shorter, a); });
  guarded("add_unequal", [&] { dom->add(a, shorter); });
  guarded("sub_unequal", [&] { dom->sub(shorter, a); });
  guarded("mul_sub_unequal", [&] { dom->mul_sub(a, b, shorter); });
  guarded("linear_combination_coeffs", [&] { dom->linear_combination(cols, shorter); });
  guarded("vec_op_needs_c", [&] { dom->vec_op(2, a, b); });
  guarded("vec_op_unknown", [&] { dom->vec_op(9, a, b); });
  wr("mul_again", dom->mul(a, b));
  wr("mul_sub_again", dom->mul_sub(a, b, c));
}

static void polys(int curve) {
  auto dom = make_domain(64, curve);
  if (!dom) return;
  const FrVec coeffs = rd<Fr>("coeffs"), evals = rd<Fr>("evals");
  const Fr z = rd1("z"), tau = rd1("tau"), offset = rd1("offset"), zero = rd1("zero");
  wr("evaluate", dom->evaluate(coeffs, z));
  ran("evaluate");
  Fr rem;
  wr("divide_by_linear", dom->divide_by_linear(coeffs, z, &rem));
  wr("rem", rem);
  wr("divide_by_linear_norem", dom->divide_by_linear(coeffs, z));
  ran("divide_by_linear");
  wr("lagrange", dom->evaluate_all_lagrange_coefficients(tau));
  ran("evaluate_all_lagrange_coefficients");
  wr("vanishing", dom->evaluate_vanishing_polynomial(tau));
  ran("evaluate_vanishing_polynomial");
  wr("dvc", dom->divide_by_vanishing_poly_on_coset(evals));
  wr("dvc_offset", dom->divide_by_vanishing_poly_on_coset(evals, &offset));
  ran("divide_by_vanishing_poly_on_coset");
  guarded("dvc_zero_offset", [&] { dom->divide_by_vanishing_poly_on_coset(evals, &zero); });
  wr("dvc_again", dom->divide_by_vanishing_poly_on_coset(evals));
}

static void scans(int curve) {
  auto dom = make_domain(64, curve);
  if (!dom) return;
  const FrVec v = rd<Fr>("v");
  Fr total;
  wr("product_exclusive", dom->prefix_product(v, false, &total));
  wr("product_exclusive_total", total);
  wr("product_inclusive", dom->prefix_product(v, true, &total));
  wr("product_inclusive_total", total);
  ran("prefix_product");
  wr("sum_exclusive", dom->prefix_sum(v, false, &total));
  wr("sum_exclusive_total", total);
  wr("sum_inclusive", dom->prefix_sum(v, true, &total));
  wr("sum_inclusive_total", total);
  wr("sum_default", dom->prefix_sum(v));
  ran("prefix_sum");
  ran("scan");
  const FrVec wires = rd<Fr>("wires"), broken = rd<Fr>("wires_broken"), sigmas = rd<Fr>("sigmas"), ks = rd<Fr>("ks");
  const Fr beta = rd1("beta"), gamma = rd1("gamma");
  const size_t stride = (size_t)num("stride");
  wr("permutation", dom->permutation_product(wires, sigmas, stride, ks, beta, gamma, &total));
  wr("permutation_total", total);
  wr("permutation_broken", dom->permutation_product(broken, sigmas, stride, ks, beta, gamma, &total));
  wr("permutation_broken_total", total);
  ran("permutation_product");
  FrVec cut(wires.begin(), wires.end() - 1);
  guarded("permutation_short_wires", [&] { dom->permutation_product(cut, sigmas, stride, ks, beta, gamma); });
  guarded("permutation_short_sigmas", [&] { dom->permutation_product(wires, cut, stride, ks, beta, gamma); });
  guarded("permutation_small_stride", [&] { dom->permutation_product(wires, sigmas, dom->size() - 1, ks, beta, gamma); });
  guarded("permutation_no_columns", [&] { dom->permutation_product(wires, sigmas, stride, FrVec(), beta, gamma); });
  guarded("permutation_nine_columns", [&] { dom->permutation_product(FrVec(9 * stride), FrVec(9 * stride), stride, FrVec(9), beta, gamma); });
  wr("permutation_again", dom->permutation_product(wires, sigmas, stride, ks, beta, gamma, &total));
  wr("permutation_again_total", total);
}

static void quotient(int curve) {
  auto dom = make_domain((size_t)num("M"), curve);
  if (!dom) return;
  const size_t stride = (size_t)num("stride"), n = (size_t)num("n");
  const FrVec wires = rd<Fr>("wires"), sigmas = rd<Fr>("sigmas"), selectors = rd<Fr>("selectors"), z = rd<Fr>("z"), pi = rd<Fr>("pi"), ks = rd<Fr>("ks");
  const Fr alpha = rd1("alpha"), beta = rd1("beta"), gamma = rd1("gamma"), offset = rd1("offset");
  const FrVec none;
  wr("full", dom->plonk_quotient(wires, sigmas, selectors, z, pi, stride, n, ks, alpha, beta, gamma));
  wr("no_selectors", dom->plonk_quotient(wires, sigmas, none, z, pi, stride, n, ks, alpha, beta, gamma));
  wr("no_pi", dom->plonk_quotient(wires, sigmas, selectors, z, none, stride, n, ks, alpha, beta, gamma));
  wr("bare_offset", dom->plonk_quotient(wires, sigmas, none, z, none, stride, n, ks, alpha, beta, gamma, &offset));
  ran("plonk_quotient");
  const FrVec cut_w(wires.begin(), wires.end() - 1), cut_s(selectors.begin(), selectors.end() - 1), cut_z(z.begin(), z.end() - 1);
  guarded("short_wires", [&] { dom->plonk_quotient(cut_w, sigmas, selectors, z, pi, stride, n, ks, alpha, beta, gamma); });
  guarded("short_sigmas", [&] { dom->plonk_quotient(wires, cut_w, selectors, z, pi, stride, n, ks, alpha, beta, gamma); });
  guarded("short_selectors", [&] { dom->plonk_quotient(wires, sigmas, cut_s, z, pi, stride, n, ks, alpha, beta, gamma); });
  guarded("short_z", [&] { dom->plonk_quotient(wires, sigmas, selectors, cut_z, pi, stride, n, ks, alpha, beta, gamma); });
  guarded("short_pi", [&] { dom->plonk_quotient(wires, sigmas, selectors, z, cut_z, stride, n, ks, alpha, beta, gamma); });
  guarded("small_stride", [&] { dom->plonk_quotient(wires, sigmas, selectors, z, pi, dom->size() - 1, n, ks, alpha, beta, gamma); });
  guarded("no_columns", [&] { dom->plonk_quotient(wires, sigmas, none, z, pi, stride, n, none, alpha, beta, gamma); });
  guarded("bad_ratio", [&] { dom->plonk_quotient(wires, sigmas, selectors, z, pi, stride, dom->size(), ks, alpha, beta, gamma); });
  wr("full_again", dom->plonk_quotient(wires, sigmas, selectors, z, pi, stride, n, ks, alpha, beta, gamma));
}

static void sparse(int curve) {
  auto dom = make_domain((size_t)num("domain"), curve);
  if (!dom) return;
  const std::vector<uint64_t> row_ptr = rd<uint64_t>("row_ptr");
  const std::vector<uint32_t> col_idx = rd<uint32_t>("col_idx");
  const FrVec values = rd<Fr>("values"), z = rd<Fr>("z");
  const size_t rows = (size_t)num("rows"), cols = (size_t)num("cols");
  {
    SparseMatrix first(*dom, rows, cols, row_ptr, col_idx, values);
    SparseMatrix M(std::move(first));
    ran("SparseMatrix");
    wr_u64("shape", {M.rows(), M.cols(), M.query("nnz")});
    ran("rows");
    ran("cols");
    ran("SparseMatrix::query");
    wr("apply", M.apply(z));
    ran("apply");
    guarded("apply_short_z", [&] { M.apply(FrVec(z.begin(), z.end() - 1)); });
    guarded("apply_long_z", [&] {
      FrVec more(z);
      more.push_back(z[0]);
      M.apply(more);
    });
    wr("apply_again", M.apply(z));
  }
  std::vector<uint64_t> rp_short(row_ptr.begin(), row_ptr.end() - 1);
  guarded("create_short_row_ptr", [&] { SparseMatrix(*dom, rows, cols, rp_short, col_idx, values); });
  guarded("create_empty_row_ptr", [&] { SparseMatrix(*dom, ~(size_t)0, cols, std::vector<uint64_t>(), col_idx, values); });
  guarded("create_short_col_idx", [&] { SparseMatrix(*dom, rows, cols, row_ptr, std::vector<uint32_t>(col_idx.begin(), col_idx.end() - 1), values); });
  guarded("create_short_values", [&] { SparseMatrix(*dom, rows, cols, row_ptr, col_idx, FrVec(values.begin(), values.end() - 1)); });
  std::vector<uint32_t> wild(col_idx);
  wild[0] = (uint32_t)cols;
  guarded("create_column_out_of_range", [&] { SparseMatrix(*dom, rows, cols, row_ptr, wild, values); });
  // the witness map of a toy R1CS
  const size_t constraints = (size_t)num("constraints"), nvars = (size_t)num("nvars"), num_inputs = (size_t)num("num_inputs");
  SparseMatrix A(*dom, constraints, nvars, rd<uint64_t>("a_row_ptr"), rd<uint32_t>("a_col_idx"), rd<Fr>("a_values"));
  SparseMatrix B(*dom, constraints, nvars, rd<uint64_t>("b_row_ptr"), rd<uint32_t>("b_col_idx"), rd<Fr>("b_values"));
  const FrVec w = rd<Fr>("witness");
  wr("witness_a", A.apply(w));
  wr("witness_b", B.apply(w));
  wr("witness_h", groth16_witness_map(*dom, A, B, w, num_inputs));
  ran("groth16_witness_map");
  guarded("witness_map_inputs", [&] { groth16_witness_map(*dom, A, B, w, w.size() + 1); });
  Domain small((size_t)num("constraints"), curve);       // holds the constraints, but not the inputs behind them
  guarded("witness_map_domain", [&] { groth16_witness_map(small, A, B, w, num_inputs); });
}

static void lookup(int curve) {
  auto dom = make_domain(64, curve);
  if (!dom) return;
  const FrVec table = rd<Fr>("table"), values = rd<Fr>("values"), present = rd<Fr>("values_present");
  LookupTable first(*dom, table);
  LookupTable t(std::move(first));
  ran("LookupTable");
  wr_u64("query", {t.query("n"), t.query("distinct")});
  ran("LookupTable::query");
  LookupTable::Counts c = t.multiplicities(values);
  wr("mult", c.mult);
  wr("index", c.index);
  wr_u64("stats", {c.missing, c.first_missing});
  ran("multiplicities");
  uint64_t first_missing = ~(uint64_t)0;
  FrVec s = t.sorted(values, &first_missing);
  wr("sorted_missing", s);
  wr_u64("sorted_missing_first", {first_missing});
  first_missing = ~(uint64_t)0;
  s = t.sorted(present, &first_missing);
  wr("sorted", s);
  wr_u64("sorted_first", {first_missing});
  ran("sorted");
  c = t.multiplicities(present);
  wr("mult_present", c.mult);
  // logUp
  const FrVec lt = rd<Fr>("logup_table"), lm = rd<Fr>("logup_mult"), beta = rd<Fr>("logup_beta");
  const std::vector<FrVec> columns = {rd<Fr>("logup_col0"), rd<Fr>("logup_col1")};
  Fr total;
  wr("logup", logup_sum(*dom, lt, lm, columns, beta[0], &total));
  wr("logup_total", total);
  wr("logup_nototal", logup_sum(*dom, lt, lm, columns, beta[0]));
  ran("logup_sum");
  std::vector<FrVec> ragged = columns;
  ragged[1].pop_back();
  guarded("logup_short_column", [&] { logup_sum(*dom, lt, lm, ragged, beta[0]); });
  ragged = columns;
  ragged[0].push_back(beta[0]);
  guarded("logup_long_column", [&] { logup_sum(*dom, lt, lm, ragged, beta[0]); });
  guarded("logup_short_mult", [&] { logup_sum(*dom, lt, FrVec(lm.begin(), lm.end() - 1), columns, beta[0]); });
  guarded("logup_no_columns", [&] { logup_sum(*dom, lt, lm, std::vector<FrVec>(), beta[0]); });
  guarded("create_empty_table", [&] { LookupTable(*dom, FrVec()); });
  wr("logup_again", logup_sum(*dom, lt, lm, columns, beta[0], &total));
  wr("mult_again", t.multiplicities(values).mult);
}

static void expr(int curve) {
  auto dom = make_domain(64, curve);
  if (!dom) return;
  const std::vector<uint32_t> nodes = rd<uint32_t>("nodes");
  const FrVec consts = rd<Fr>("consts"), chals = rd<Fr>("challenges");
  const std::vector<FrVec> cols = {rd<Fr>("col0"), rd<Fr>("col1"), rd<Fr>("col2")};
  GateProgram first(*dom, nodes, consts, chals.size(), cols.size());
  GateProgram prog(std::move(first));
  ran("GateProgram");
  wr_u64("query", {prog.query("slots"), prog.query("nodes"), prog.query("columns")});
  ran("GateProgram::query");
  const size_t rot_step = (size_t)num("rot_step");
  wr("run", prog.run(cols, chals, rot_step));
  wr("run_step1", prog.run(cols, chals));
  ran("run");
  guarded("run_column_missing", [&] { prog.run(std::vector<FrVec>(cols.begin(), cols.end() - 1), chals, rot_step); });
  guarded("run_challenge_missing", [&] { prog.run(cols, FrVec(chals.begin(), chals.end() - 1), rot_step); });
  guarded("create_bad_nodes", [&] { GateProgram(*dom, std::vector<uint32_t>(nodes.begin(), nodes.end() - 1), consts, chals.size(), cols.size()); });
  wr("run_again", prog.run(cols, chals, rot_step));
}

static void poseidon(int curve) {
  auto dom = make_domain(64, curve);
  if (!dom) return;
  const unsigned rate = (unsigned)num("rate"), alpha = (unsigned)num("alpha"), full = (unsigned)num("full_rounds"), partial = (unsigned)num("partial_rounds");
  const FrVec ark = rd<Fr>("ark"), mds = rd<Fr>("mds"), in = rd<Fr>("in"), header = rd<Fr>("header"), leaves = rd<Fr>("leaves");
  const Fr sep = rd1("domain_sep");
  const size_t in_len = (size_t)num("in_len"), n_out = (size_t)num("n_out"), leaf_len = (size_t)num("leaf_len");
  guarded("create_short_ark", [&] { Poseidon(*dom, rate, alpha, full, partial, FrVec(ark.begin(), ark.end() - 1), mds); });
  guarded("create_short_mds", [&] { Poseidon(*dom, rate, alpha, full, partial, ark, FrVec(mds.begin(), mds.end() - 1)); });
  guarded("create_even_alpha", [&] { Poseidon(*dom, rate, 4, full, partial, ark, mds); });
  Poseidon first(*dom, rate, alpha, full, partial, ark, mds);
  Poseidon p(std::move(first));
  ran("Poseidon");
  wr_u64("query", {p.query("rate"), p.query("state"), p.query("rounds")});
  ran("Poseidon::query");
  wr("hash", p.hash(in, in_len, n_out));
  wr("hash_header", p.hash(in, in_len, n_out, header));
  wr("hash_one_out", p.hash(in, in_len, 1, header));
  ran("hash");
  wr("merkle_tree", p.merkle_tree(sep, leaves, leaf_len));
  ran("merkle_tree");
  guarded("hash_bad_header", [&] { p.hash(in, in_len, n_out, FrVec(header.begin(), header.end() - 1)); });
  guarded("hash_ragged_rows", [&] { p.hash(FrVec(in.begin(), in.end() - 1), in_len, n_out); });
  guarded("merkle_ragged_leaves", [&] { p.merkle_tree(sep, FrVec(leaves.begin(), leaves.end() - 1), leaf_len); });
  guarded("merkle_no_leaves", [&] { p.merkle_tree(sep, FrVec(), leaf_len); });
  wr("hash_again", p.hash(in, in_len, n_out, header));
}

static void pairing(int curve) {
  std::unique_ptr<Pairing> first;
  if (!guarded("create", [&] { first.reset(new Pairing(curve)); })) return;
  Pairing e(std::move(*first));
  first.reset();
  ran("Pairing");
  const std::vector<uint8_t> g1 = rd<uint8_t>("g1"), g2 = rd<uint8_t>("g2"), c1 = rd<uint8_t>("check_g1"), c2 = rd<uint8_t>("check_g2");
  wr_u64("query", {e.query("curve")});
  ran("Pairing::query");
  wr("pairing", e.pairing(g1, g2));
  wr("pairing_canonical", e.pairing(g1, g2, 1, true));
  wr("pairing_group2", e.pairing(g1, g2, 2));
  ran("pairing");
  wr("product", e.product_of_pairings(g1, g2));
  wr("product_canonical", e.product_of_pairings(g1, g2, true));
  ran("product_of_pairings");
  wr("check_groups", e.check_groups(c1, c2, 2));
  wr("check_groups_single", e.check_groups(c1, c2, 1));
  ran("check_groups");
  const std::vector<uint8_t> empty;
  guarded("pairing_ragged_g1", [&] { e.pairing(std::vector<uint8_t>(g1.begin(), g1.end() - 1), g2); });
  guarded("pairing_short_g2", [&] { e.pairing(g1, std::vector<uint8_t>(g2.begin(), g2.end() - 200)); });
  guarded("pairing_group_zero", [&] { e.pairing(g1, g2, 0); });
  guarded("pairing_partial_group", [&] { e.pairing(g1, g2, 3); });
  guarded("product_empty", [&] { e.product_of_pairings(empty, empty); });
  guarded("check_partial_group", [&] { e.check_groups(c1, c2, 3); });
  guarded("check_short_g2", [&] { e.check_groups(c1, std::vector<uint8_t>(c2.begin(), c2.end() - 200), 2); });
  guarded("query_unknown", [&] { e.query("no such key"); });
  wr("pairing_again", e.pairing(g1, g2, 2));
}

static void h2c(int curve) {
  const std::vector<uint8_t> dst = rd<uint8_t>("dst"), packed = rd<uint8_t>("messages"), u = rd<uint8_t>("u");
  const std::vector<uint64_t> off = rd<uint64_t>("message_offsets");
  std::vector<std::string> msgs;
  for (size_t i = 0; i + 1 < off.size(); i++) msgs.emplace_back(packed.begin() + off[i], packed.begin() + off[i + 1]);
  std::unique_ptr<HashToCurve> first;
  if (!guarded("create", [&] { first.reset(new HashToCurve(curve, std::string(dst.begin(), dst.end()))); })) return;
  HashToCurve h(std::move(*first));
  first.reset();
  ran("HashToCurve");
  wr_u64("query", {h.query("curve"), h.query("dst_bytes"), h.m(), h.image_bytes()});
  ran("HashToCurve::query");
  wr("hash", h.hash(msgs));
  wr("encode", h.hash(msgs, true));
  ran("HashToCurve::hash");
  wr("field", h.hash_to_field(msgs));
  wr("field_one", h.hash_to_field(msgs, 1));
  ran("hash_to_field");
  wr("map", h.map_to_curve(u));
  wr("map_pairs", h.map_to_curve(u, true));
  ran("map_to_curve");
  guarded("map_ragged", [&] { h.map_to_curve(std::vector<uint8_t>(u.begin(), u.end() - 1)); });
  guarded("map_odd_pairs", [&] { h.map_to_curve(std::vector<uint8_t>(u.begin(), u.end() - 48 * h.m()), true); });
  guarded("field_count_three", [&] { h.hash_to_field(msgs, 3); });
  guarded("create_377", [&] { HashToCurve(MI355_BLS12_377_G1, "tag"); });
  guarded("create_empty_tag", [&] { HashToCurve(curve, ""); });
  wr("hash_again", h.hash(msgs));
}

static void mle(int curve) {
  auto dom = make_domain(64, curve);
  if (!dom) return;
  const FrVec evals = rd<Fr>("evals"), fix_point = rd<Fr>("fix_point"), full_point = rd<Fr>("full_point"), eq_point = rd<Fr>("eq_point");
  wr("fix", mle_fix_variables(*dom, evals, fix_point));
  ran("mle_fix_variables");
  wr("evaluate", mle_evaluate(*dom, evals, full_point));
  ran("mle_evaluate");
  wr("eq", eq_table(*dom, eq_point));
  ran("eq_table");
  const size_t m = (size_t)num("tables");
  std::vector<FrVec> tables;
  for (size_t k = 0; k < m; k++) tables.push_back(rd<Fr>("table" + std::to_string(k)));
  const FrVec coeffs = rd<Fr>("term_coeffs");
  const std::vector<uint32_t> n_factors = rd<uint32_t>("term_n_factors"), factors = rd<uint32_t>("term_factors");
  std::vector<SumcheckTerm> terms(coeffs.size());
  for (size_t j = 0; j < terms.size(); j++) {
    terms[j].coeff = coeffs[j];
    terms[j].factors.assign(factors.begin() + 5 * j, factors.begin() + 5 * j + n_factors[j]);
  }
  wr("round", sumcheck_round(*dom, tables, terms));
  const Fr r_prev = rd1("r_prev");
  std::vector<FrVec> folded;
  wr("round_fused", sumcheck_round(*dom, tables, terms, &r_prev, &folded));
  for (size_t k = 0; k < folded.size(); k++) wr("folded" + std::to_string(k), folded[k]);
  wr_u64("folded_count", {folded.size()});
  ran("sumcheck_round");
  guarded("fix_not_a_power_of_two", [&] { mle_fix_variables(*dom, FrVec(evals.begin(), evals.end() - 1), fix_point); });
  guarded("fix_long_point", [&] {
    FrVec p(full_point);
    p.push_back(full_point[0]);
    mle_fix_variables(*dom, evals, p);
  });
  guarded("evaluate_short_point", [&] { mle_evaluate(*dom, evals, fix_point); });
  guarded("round_no_tables", [&] { sumcheck_round(*dom, std::vector<FrVec>(), terms); });
  guarded("round_ragged_tables", [&] {
    std::vector<FrVec> t(tables);
    t.back().resize(t.back().size() / 2);
    sumcheck_round(*dom, t, terms);
  });
  guarded("round_no_place_for_folded", [&] { sumcheck_round(*dom, tables, terms, &r_prev); });
  guarded("round_six_factors", [&] {
    std::vector<SumcheckTerm> t(terms);
    t[0].factors.assign(6, 0);
    sumcheck_round(*dom, tables, t);
  });
  guarded("round_no_factors", [&] {
    std::vector<SumcheckTerm> t(terms);
    t[0].factors.clear();
    sumcheck_round(*dom, tables, t);
  });
  guarded("round_unknown_table", [&] {
    std::vector<SumcheckTerm> t(terms);
    t[0].factors[0] = (uint32_t)m;
    sumcheck_round(*dom, tables, t);
  });
  wr("round_again", sumcheck_round(*dom, tables, terms));
}

static void fixed(int curve) {
  const std::vector<G1Affine> g = rd<G1Affine>("g");
  const FrVec scalars = rd<Fr>("scalars");
  std::unique_ptr<WindowTable> made;
  if (!guarded("create", [&] { made.reset(new WindowTable(FixedBase::get_window_table(g.at(0), 0, curve))); })) return;
  WindowTable& chosen = *made;
  ran("get_window_table");
  WindowTable forced(FixedBase::get_window_table(g[0], (int)num("window"), curve, scalars.size()));
  wr_u64("window_bits", {chosen.query("window_bits"), forced.query("window_bits"), forced.query("levels")});
  ran("WindowTable::query");
  wr_u64("window_size", {FixedBase::get_mul_window_size(10), FixedBase::get_mul_window_size(1000)});
  ran("get_mul_window_size");
  wr("msm", FixedBase::msm(chosen, scalars));
  wr("msm_forced", FixedBase::msm(forced, scalars));
  ran("msm");
  wr("msm_affine", FixedBase::msm_affine(chosen, scalars));
  ran("msm_affine");
  WindowTable moved(std::move(forced));
  wr("msm_affine_moved", FixedBase::msm_affine(moved, scalars));
  guarded("window_too_wide", [&] { FixedBase::get_window_table(g[0], 21, curve); });
  guarded("unknown_curve", [&] { FixedBase::get_window_table(g[0], 0, 17); });
  guarded("query_unknown", [&] { moved.query("no such key"); });
  wr("msm_again", FixedBase::msm(moved, scalars));
}

static void wr_check(const std::string& name, const CheckResult& r) {
  wr(name + "_status", r.status);
  wr_u64(name + "_counts", {r.valid, r.flagged_infinity, r.not_canonical, r.off_curve, r.off_subgroup, r.first_invalid, r.ok ? 1u : 0u, r.method});
}

static void points(int curve) {
  const std::vector<G1Affine> few = rd<G1Affine>("mul_points");
  const std::vector<uint8_t> plain = rd<uint8_t>("mul_scalars"), mont = rd<uint8_t>("mul_scalars_montgomery"), k = rd<uint8_t>("k");
  std::unique_ptr<MultiScalarMultContext> first;
  if (!guarded("create", [&] { first.reset(new MultiScalarMultContext(multi_scalar_mult_init(few, curve))); })) return;
  MultiScalarMultContext ctx(std::move(*first));
  first.reset();
  ran("multi_scalar_mult_init");
  Hip hip;
  // the checks
  const std::vector<G1Affine> corpus = rd<G1Affine>("corpus");
  wr_check("check", check_bases(ctx, corpus));
  wr_check("check_exact", check_bases(ctx, corpus, true));
  ran("check_bases");
  {
    void* d = hip.upload(corpus.data(), corpus.size() * sizeof(G1Affine));
    guarded("check_bases_device", [&] {
      wr_check("check_device", check_bases_device(ctx, d, corpus.size(), sizeof(G1Affine)));
      wr_check("check_device_exact", check_bases_device(ctx, d, corpus.size(), sizeof(G1Affine), true));
      ran("check_bases_device");
    });
    guarded("check_device_bad_stride", [&] { check_bases_device(ctx, d, corpus.size(), 6); });
    hip.free_(d);
  }
  // the codec
  std::vector<uint8_t> records;
  wr_check("compress", compress_points(ctx, rd<G1Affine>("compress_points"), records));
  wr("compress_records", records);
  ran("compress_points");
  std::vector<G1Affine> decoded;
  const std::vector<uint8_t> to_decode = rd<uint8_t>("records");
  wr_check("decompress", decompress_points(ctx, to_decode, decoded));
  wr("decompress_points", decoded);
  wr_check("decompress_validate", decompress_points(ctx, to_decode, decoded, true));
  wr("decompress_validate_points", decoded);
  ran("decompress_points");
  // point multiplication
  wr("mul_points", mul_points(ctx, few, plain));
  wr("mul_points_montgomery", mul_points(ctx, few, mont, true));
  ran("mul_points");
  wr("mul_points_by", mul_points_by(ctx, few, k));
  ran("mul_points_by");
  wr("mul_by_cofactor", mul_by_cofactor(ctx, few));
  ran("mul_by_cofactor");
  guarded("mul_points_ragged", [&] { mul_points(ctx, few, std::vector<uint8_t>(plain.begin(), plain.end() - 1)); });
  guarded("mul_points_by_three_bytes", [&] { mul_points_by(ctx, few, std::vector<uint8_t>(3, 1)); });
  wr("mul_points_again", mul_points(ctx, few, plain));
  // MSMs on the bases of init, then on bases set from compressed records
  const std::vector<BigInteger256> few_scalars = rd<BigInteger256>("few_scalars");
  wr("msm_init", multi_scalar_mult(ctx, few, few_scalars));
  ran("multi_scalar_mult");
  const std::vector<uint8_t> msm_records = rd<uint8_t>("msm_records");
  const std::vector<G1Affine> msm_points = rd<G1Affine>("msm_points");
  const std::vector<BigInteger256> msm_scalars = rd<BigInteger256>("msm_scalars");
  guarded("msm_point_count", [&] { multi_scalar_mult(ctx, msm_points, msm_scalars); });
  set_bases_compressed(ctx, msm_records);
  ran("set_bases_compressed");
  wr("msm_compressed", multi_scalar_mult(ctx, msm_points, msm_scalars));
  guarded("msm_partial_batch", [&] { multi_scalar_mult(ctx, msm_points, std::vector<BigInteger256>(msm_scalars.begin(), msm_scalars.end() - 1)); });
  guarded("set_bases_compressed_malformed", [&] { set_bases_compressed(ctx, to_decode); });
  wr("msm_compressed_again", multi_scalar_mult(ctx, msm_points, msm_scalars));
  {
    void* d = hip.upload(msm_scalars.data(), msm_scalars.size() * sizeof(BigInteger256));
    guarded("multi_scalar_mult_async", [&] {
      MsmJob job = multi_scalar_mult_async(ctx, d, msm_scalars.size() / msm_points.size());
      ran("multi_scalar_mult_async");
      MsmJob moved(std::move(job));
      wr("msm_async", moved.wait());
      ran("MsmJob::wait");
      wr_u64("msm_async_done", {moved.done() ? 1u : 0u, job.done() ? 1u : 0u});
      ran("MsmJob::done");
    });
    hip.free_(d);
  }
  wr("msm_stateless", msm(msm_points, msm_scalars, curve));
  ran("msm");
  // msm_chunks: the bases outnumber the scalars, which pair up with the last ones
  const std::vector<G1Affine> chunk_bases = rd<G1Affine>("chunk_bases");
  const std::vector<BigInteger256> chunk_scalars = rd<BigInteger256>("chunk_scalars");
  wr("msm_chunks", msm_chunks(chunk_bases, chunk_scalars, (size_t)num("step"), curve));
  wr("msm_chunks_one_step", msm_chunks(chunk_bases, chunk_scalars, size_t(1) << 20, curve));
  ran("msm_chunks");
  guarded("msm_chunks_more_scalars", [&] { msm_chunks(msm_points, chunk_scalars, 100, curve); });
  guarded("msm_chunks_step_zero", [&] { msm_chunks(chunk_bases, chunk_scalars, 0, curve); });
  // transforms of points
  auto dom = make_domain((size_t)num("fft_size"), curve);
  const std::vector<G1Affine> fft_in = rd<G1Affine>("fft_points_in");
  wr("fft_points", fft_points(ctx, *dom, fft_in));
  ran("fft_points");
  wr("ifft_points", ifft_points(ctx, *dom, fft_in));
  ran("ifft_points");
  guarded("fft_points_too_long", [&] { fft_points(ctx, *dom, msm_points); });
  wr("fft_points_again", fft_points(ctx, *dom, fft_in));
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <family> <dir>\n", argv[0]);
    return 2;
  }
  const std::string family = argv[1];
  DIR = argv[2];
  static const std::map<std::string, void (*)(int)> families = {
      {"transforms", transforms}, {"vecops", vecops}, {"polys", polys},     {"scans", scans}, {"quotient", quotient}, {"sparse", sparse}, {"lookup", lookup},
      {"expr", expr},             {"poseidon", poseidon}, {"pairing", pairing}, {"h2c", h2c},     {"mle", mle},           {"fixed", fixed},   {"points", points}};
  auto it = families.find(family);
  if (it == families.end()) {
    fprintf(stderr, "unknown family %s\n", family.c_str());
    return 2;
  }
  try {
    FILE* f = fopen((DIR + "/case.txt").c_str(), "r");
    if (!f) throw std::runtime_error("case.txt: cannot open");
    char line[512];
    while (fgets(line, sizeof line, f)) {      // `key value`, the value running to the end of the line
      std::string s(line);
      while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
      const size_t sp = s.find(' ');
      if (sp != std::string::npos) CFG[s.substr(0, sp)] = s.substr(sp + 1);
    }
    fclose(f);
    it->second((int)num("curve"));
  } catch (const MsmError& e) {
    fprintf(stderr, "unexpected MsmError %d: %s\n", e.code, e.what());
    return 1;
  } catch (const std::exception& e) {
    fprintf(stderr, "unexpected exception: %s\n", e.what());
    return 1;
  }
  printf("%s: %s\n", family.c_str(), BAD ? "FAILED" : "done");
  return BAD ? 1 : 0;
}
