// mi355_msm.hpp -- header-only C++ mirror of the reference's Rust operator API over the C ABI (mi355_msm.h).
//
// The reference's host layer is Rust (P1A <entry>/src/lib.rs); this image has no Rust toolchain, so the host side above
// the C ABI is C++ where the reference is compiled code (the brief's rule).  Same names, argument meaning and error
// behaviour: `multi_scalar_mult_init(points) -> MultiScalarMultContext`, `multi_scalar_mult(ctx, points, scalars)
// -> Vec<G::Projective>` with batch_size = scalars.len() / points.len() (P1A 6block/src/lib.rs:54-109); a non-zero error
// code panics on the Rust side and throws here.  VariableBaseMSM::msm chops to the shorter slice
// (ARK ec/src/msm/variable_base/mod.rs:44-53).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mi355_msm.h"

namespace mi355 {

struct G1Affine {        // arkworks Affine image: size_of::<G1Affine>() == 104
  uint64_t x[6], y[6];
  uint8_t infinity;
  uint8_t pad[7];
};
struct BigInteger256 {
  uint64_t limbs[4];
};
struct G1Projective {    // arkworks Projective image (Jacobian), 144 bytes
  uint64_t x[6], y[6], z[6];
};
static_assert(sizeof(G1Affine) == 104 && sizeof(BigInteger256) == 32 && sizeof(G1Projective) == 144, "ABI layouts");

struct MsmError : std::runtime_error {
  int code;
  MsmError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void check(RustError e) {
  if (e.code != 0) {
    std::string msg = e.message ? e.message : "(no message)";
    if (e.message) std::free(e.message);
    throw MsmError(e.code, "mi355_msm error " + std::to_string(e.code) + ": " + msg);
  }
}

struct MultiScalarMultContext {   // #[repr(C)] struct { context: *mut c_void }
  mi355_msm_ctx* context = nullptr;
  size_t npoints = 0;
  MultiScalarMultContext() = default;
  MultiScalarMultContext(const MultiScalarMultContext&) = delete;
  MultiScalarMultContext& operator=(const MultiScalarMultContext&) = delete;
  MultiScalarMultContext(MultiScalarMultContext&& o) noexcept : context(o.context), npoints(o.npoints) { o.context = nullptr; }
  ~MultiScalarMultContext() {
    if (context) {
      RustError e = mi355_msm_destroy(context);
      if (e.message) std::free(e.message);
    }
  }
};

// On-curve and subgroup check of host-resident points (mi355_msm_check_bases): status[i] in 0..3, true when every point is valid.
struct CheckResult {
  bool ok = true;
  uint64_t valid = 0, flagged_infinity = 0, not_canonical = 0, off_curve = 0, off_subgroup = 0, first_invalid = 0, method = 0, device_us = 0;
  std::vector<uint8_t> status;
};
inline CheckResult check_bases(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points, bool exact = false) {
  CheckResult r;
  uint64_t out[8] = {0};
  r.status.resize(points.size());
  check(mi355_msm_check_bases(ctx.context, points.data(), points.size(), sizeof(G1Affine), exact ? 2u : 0u, r.status.data(), out));
  r.valid = out[0]; r.flagged_infinity = out[1]; r.not_canonical = out[2]; r.off_curve = out[3]; r.off_subgroup = out[4];
  r.first_invalid = out[5]; r.method = out[6]; r.device_us = out[7];
  r.ok = out[5] == points.size();
  return r;
}
inline CheckResult check_bases_device(MultiScalarMultContext& ctx, const void* d_points, size_t npoints, size_t stride, bool exact = false) {
  CheckResult r;
  uint64_t out[8] = {0};
  r.status.resize(npoints);
  check(mi355_msm_check_bases_device(ctx.context, d_points, npoints, stride, exact ? 2u : 0u, r.status.data(), out));
  r.valid = out[0]; r.flagged_infinity = out[1]; r.not_canonical = out[2]; r.off_curve = out[3]; r.off_subgroup = out[4];
  r.first_invalid = out[5]; r.method = out[6]; r.device_us = out[7];
  r.ok = out[5] == npoints;
  return r;
}

// arkworks compressed G1 records (48 bytes each, mi355_msm_decompress_points) -> Affine images; `r.status[i]`: 0 decoded, 1 malformed,
// 2 no point has this x, 3 (validate) outside the order-r subgroup.  The counters of CheckResult read: not_canonical = status 1,
// off_curve = status 2.
inline CheckResult decompress_points(MultiScalarMultContext& ctx, const std::vector<uint8_t>& records, std::vector<G1Affine>& out, bool validate = false) {
  CheckResult r;
  uint64_t o[8] = {0};
  const size_t n = records.size() / 48;
  out.resize(n);
  r.status.resize(n);
  check(mi355_msm_decompress_points(ctx.context, records.data(), n, out.data(), sizeof(G1Affine), validate ? 2u : 0u, r.status.data(), o));
  r.valid = o[0]; r.flagged_infinity = o[1]; r.not_canonical = o[2]; r.off_curve = o[3]; r.off_subgroup = o[4];
  r.first_invalid = o[5]; r.method = o[6]; r.device_us = o[7];
  r.ok = o[5] == n;
  return r;
}
// Affine images -> compressed records (mi355_msm_compress_points); status 1: a coordinate is not canonical
inline CheckResult compress_points(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points, std::vector<uint8_t>& out_records) {
  CheckResult r;
  uint64_t o[8] = {0};
  out_records.resize(points.size() * 48);
  r.status.resize(points.size());
  check(mi355_msm_compress_points(ctx.context, points.data(), points.size(), sizeof(G1Affine), 0u, out_records.data(), r.status.data(), o));
  r.valid = o[0]; r.flagged_infinity = o[1]; r.not_canonical = o[2]; r.first_invalid = o[5]; r.device_us = o[7];
  r.ok = o[5] == points.size();
  return r;
}
// out[i] = scalars[i] * points[i] (mi355_msm_mul_points): 32-byte little-endian integers, all 256 bits significant; `montgomery`: arkworks
// Fr images.  Any curve points: no curve test, no subgroup test.  Affine images out.
inline std::vector<G1Affine> mul_points(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points, const std::vector<uint8_t>& scalars,
                                        bool montgomery = false) {
  if (scalars.size() != 32 * points.size()) throw std::runtime_error("mul_points: one 32-byte scalar per point");
  std::vector<G1Affine> out(points.size());
  check(mi355_msm_mul_points(ctx.context, points.data(), points.size(), sizeof(G1Affine), scalars.data(), 32, montgomery ? 1u : 0u, out.data(),
                             sizeof(G1Affine)));
  return out;
}
// out[i] = k * points[i] for ONE little-endian integer k of 4 .. 64 bytes (a multiple of 4)
inline std::vector<G1Affine> mul_points_by(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points, const std::vector<uint8_t>& k) {
  std::vector<G1Affine> out(points.size());
  check(mi355_msm_mul_points(ctx.context, points.data(), points.size(), sizeof(G1Affine), k.data(), k.size(), 4u, out.data(), sizeof(G1Affine)));
  return out;
}
// arkworks' mul_by_cofactor over a vector (not clear_cofactor)
inline std::vector<G1Affine> mul_by_cofactor(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points) {
  std::vector<G1Affine> out(points.size());
  check(mi355_msm_mul_points(ctx.context, points.data(), points.size(), sizeof(G1Affine), nullptr, 0, 8u, out.data(), sizeof(G1Affine)));
  return out;
}
// bases from compressed records in host memory (mi355_msm_set_bases_compressed)
inline void set_bases_compressed(MultiScalarMultContext& ctx, const std::vector<uint8_t>& records) {
  check(mi355_msm_set_bases_compressed(ctx.context, records.data(), records.size() / 48));
  ctx.npoints = records.size() / 48;
}

inline MultiScalarMultContext multi_scalar_mult_init(const std::vector<G1Affine>& points, int curve = MI355_BLS12_377_G1) {
  MultiScalarMultContext ctx;
  check(mi355_msm_create(&ctx.context, curve, -1));
  check(mi355_msm_set_bases(ctx.context, points.data(), points.size(), sizeof(G1Affine)));
  ctx.npoints = points.size();
  return ctx;
}

inline std::vector<G1Projective> multi_scalar_mult(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points,
                                                   const std::vector<BigInteger256>& scalars) {
  const size_t npoints = points.size();
  if (npoints != ctx.npoints) throw MsmError(-1, "multi_scalar_mult: context was initialised with a different point count");
  if (npoints == 0 || scalars.size() % npoints != 0) throw MsmError(-1, "multi_scalar_mult: scalars is not a whole number of batches");
  const size_t batch_size = scalars.size() / npoints;
  std::vector<G1Projective> ret(batch_size);
  check(mi355_msm_run(ctx.context, ret.data(), scalars.data(), npoints, batch_size));
  return ret;
}

// Stream-ordered run (mi355_msm_run_async; the role of ML bellman-cuda.h:48-75 msm_execute_async as P1A matter-labs/src/lib.rs:150-190
// uses it): `d_scalars` -- DEVICE memory, batch_size * npoints BigInteger256 -- must stay valid until wait() returns; the MSM is ordered
// after the work already enqueued in `stream` and runs on the context's own stream.  The job owns its output buffer.
struct MsmJob {
  mi355_msm_job* job = nullptr;
  std::vector<G1Projective> out;
  MsmJob() = default;
  MsmJob(const MsmJob&) = delete;
  MsmJob& operator=(const MsmJob&) = delete;
  MsmJob(MsmJob&& o) noexcept : job(o.job), out(std::move(o.out)) { o.job = nullptr; }
  bool done() const { return job == nullptr || mi355_msm_job_done(job) != 0; }
  std::vector<G1Projective>& wait() {
    if (job) {
      mi355_msm_job* j = job;
      job = nullptr;
      check(mi355_msm_job_wait(j));   // (releases the handle, whatever the status)
    }
    return out;
  }
  ~MsmJob() {
    if (job) {
      RustError e = mi355_msm_job_wait(job);
      if (e.message) std::free(e.message);
    }
  }
};

inline MsmJob multi_scalar_mult_async(MultiScalarMultContext& ctx, const void* d_scalars, size_t batch_size, void* stream = nullptr) {
  MsmJob j;
  j.out.resize(batch_size);
  check(mi355_msm_run_async(ctx.context, j.out.data(), d_scalars, ctx.npoints, batch_size, stream, nullptr, nullptr, &j.job));
  return j;
}

// VariableBaseMSM::msm_bigint shape: one stateless MSM, chopped to the shorter input.
inline G1Projective msm(const std::vector<G1Affine>& bases, const std::vector<BigInteger256>& scalars, int curve = MI355_BLS12_377_G1) {
  const size_t n = bases.size() < scalars.size() ? bases.size() : scalars.size();
  G1Projective out;
  check(mi355_msm(curve, &out, bases.data(), n, scalars.data(), sizeof(G1Affine)));
  return out;
}

// VariableBaseMSM::msm_chunks (ARK ec/src/msm/variable_base/mod.rs:165-199): `scalars` are Fr values (Montgomery form,
// converted on the device like into_bigint), must not outnumber the bases, pair up with the LAST scalars.size() bases, and
// are consumed `step` pairs at a time (the reference hard-codes 2^20); the partial sums are added.
inline G1Projective msm_chunks(const std::vector<G1Affine>& bases, const std::vector<BigInteger256>& scalars_fr,
                               size_t step = size_t(1) << 20, int curve = MI355_BLS12_377_G1) {
  if (scalars_fr.size() > bases.size() || step == 0) throw MsmError(-1, "msm_chunks: scalars_stream.len() <= bases_stream.len()");
  const size_t ns = scalars_fr.size(), skip = bases.size() - ns;
  MultiScalarMultContext ctx;
  check(mi355_msm_create(&ctx.context, curve, -1));
  check(mi355_msm_set_option(ctx.context, "scalars_montgomery", 1));
  std::vector<G1Projective> partials;
  for (size_t lo = 0; lo < ns; lo += step) {
    const size_t n = ns - lo < step ? ns - lo : step;
    check(mi355_msm_set_bases(ctx.context, bases.data() + skip + lo, n, sizeof(G1Affine)));
    partials.emplace_back();
    check(mi355_msm_run(ctx.context, &partials.back(), scalars_fr.data() + lo, n, 1));
  }
  G1Projective out;
  check(mi355_msm_fold(curve, &out, partials.data(), partials.size()));
  return out;
}

// arkworks' FixedBase (ARK ec/src/msm/fixed_base.rs:8-97): out[i] = scalars[i] * g through a window table that lives on the GPU.
// `scalars_fr` are Fr values (Montgomery form), as FixedBase::msm takes them; the results are normalised.
struct WindowTable {   // what get_window_table returns: owns the device table
  mi355_msm_fixed* handle = nullptr;
  WindowTable() = default;
  WindowTable(const WindowTable&) = delete;
  WindowTable& operator=(const WindowTable&) = delete;
  WindowTable(WindowTable&& o) noexcept : handle(o.handle) { o.handle = nullptr; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_fixed_query(handle, key, &v));
    return v;
  }
  ~WindowTable() {
    if (handle) {
      RustError e = mi355_msm_fixed_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

struct FixedBase {
  // arkworks' rule (a CPU cache heuristic, for parity; WindowTable::query("window_bits") says what a table uses)
  static size_t get_mul_window_size(size_t num_scalars) { return mi355_msm_fixed_window_size(num_scalars); }
  // window = 0: the engine chooses for `expected_scalars` (0 = a large batch)
  static WindowTable get_window_table(const G1Affine& g, int window = 0, int curve = MI355_BLS12_377_G1, size_t expected_scalars = 0) {
    WindowTable t;
    check(mi355_msm_fixed_create(&t.handle, curve, -1, &g, window, expected_scalars));
    return t;
  }
  static std::vector<G1Projective> msm(const WindowTable& table, const std::vector<BigInteger256>& scalars_fr) {
    std::vector<G1Projective> out(scalars_fr.size());
    check(mi355_msm_fixed_mul(table.handle, out.data(), sizeof(G1Projective), scalars_fr.data(), scalars_fr.size(), 1u | 2u));
    return out;
  }
  // msm + batch_normalization_into_affine: Affine images, ready for multi_scalar_mult_init
  static std::vector<G1Affine> msm_affine(const WindowTable& table, const std::vector<BigInteger256>& scalars_fr) {
    std::vector<G1Affine> out(scalars_fr.size());
    check(mi355_msm_fixed_mul(table.handle, out.data(), sizeof(G1Affine), scalars_fr.data(), scalars_fr.size(), 1u));
    return out;
  }
};

namespace detail {
// Does a vector of `have` elements hold m columns of n elements, `stride` >= n >= 1 elements apart?  Several C entry points take no
// length for such a vector, so the wrappers look; by division, so that no product of the caller's numbers can wrap.
inline bool holds_columns(size_t have, size_t m, size_t stride, size_t n) {
  return m == 0 || (have >= n && (m == 1 || (stride != 0 && (have - n) / stride >= m - 1)));
}
}  // namespace detail

// ark-poly's Radix2EvaluationDomain over the curve family's Fr (ARK poly/src/domain/radix2/mod.rs): vectors of Fr values (Montgomery
// form, what a Vec<Fr> holds), zero-extended to the domain size, transformed on the GPU.
struct Radix2EvaluationDomain {
  mi355_msm_domain* handle = nullptr;
  explicit Radix2EvaluationDomain(size_t num_coeffs, int curve = MI355_BLS12_377_G1) { check(mi355_msm_domain_create(&handle, curve, -1, num_coeffs)); }
  Radix2EvaluationDomain(const Radix2EvaluationDomain&) = delete;
  Radix2EvaluationDomain& operator=(const Radix2EvaluationDomain&) = delete;
  Radix2EvaluationDomain(Radix2EvaluationDomain&& o) noexcept : handle(o.handle) { o.handle = nullptr; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_domain_query(handle, key, &v));
    return v;
  }
  size_t size() const { return (size_t)query("size"); }
  BigInteger256 element(uint64_t i) const {
    BigInteger256 e;
    check(mi355_msm_domain_element(handle, i, &e));
    return e;
  }
  std::vector<BigInteger256> transform(const std::vector<BigInteger256>& v, unsigned kind) const {
    std::vector<BigInteger256> out(size());
    check(mi355_msm_domain_transform(handle, out.data(), v.data(), v.size(), 1, kind, 0, nullptr));
    return out;
  }
  std::vector<BigInteger256> fft(const std::vector<BigInteger256>& coeffs) const { return transform(coeffs, 0); }
  std::vector<BigInteger256> ifft(const std::vector<BigInteger256>& evals) const { return transform(evals, 1); }
  std::vector<BigInteger256> coset_fft(const std::vector<BigInteger256>& coeffs) const { return transform(coeffs, 2); }
  std::vector<BigInteger256> coset_ifft(const std::vector<BigInteger256>& evals) const { return transform(evals, 3); }
  // mul_polynomials_in_evaluation_domain.  Like vec_op below, mul REFUSES operands of unequal length (std::invalid_argument): an
  // output sized by one operand and computed over the shorter one would hand back elements that were never written.
  std::vector<BigInteger256> mul(const std::vector<BigInteger256>& a, const std::vector<BigInteger256>& b) const {
    if (a.size() != b.size()) throw std::invalid_argument("mul: a and b differ in length");
    std::vector<BigInteger256> out(a.size());
    check(mi355_msm_domain_mul(handle, out.data(), a.data(), b.data(), a.size(), 0));
    return out;
  }
  // ark-ff batch_inversion_and_mul: coeff / v[i], zeros stay zero
  std::vector<BigInteger256> batch_inversion_and_mul(const std::vector<BigInteger256>& v, const BigInteger256* coeff = nullptr) const {
    std::vector<BigInteger256> out(v.size());
    check(mi355_msm_domain_batch_inverse(handle, out.data(), v.data(), v.size(), coeff, 0));
    return out;
  }
  std::vector<BigInteger256> batch_inversion(const std::vector<BigInteger256>& v) const { return batch_inversion_and_mul(v); }
  // op 0 a + b, 1 a - b, 2 a * b - c; operands of unequal length are refused (std::invalid_argument)
  std::vector<BigInteger256> vec_op(unsigned op, const std::vector<BigInteger256>& a, const std::vector<BigInteger256>& b,
                                    const std::vector<BigInteger256>* c = nullptr) const {
    if (a.size() != b.size()) throw std::invalid_argument("vec_op: a and b differ in length");
    if (c && c->size() != a.size()) throw std::invalid_argument("vec_op: c differs in length from a and b");
    if (op == 2 && !c) throw std::invalid_argument("vec_op: a * b - c needs c");
    std::vector<BigInteger256> out(a.size());
    check(mi355_msm_domain_vec_op(handle, out.data(), a.data(), b.data(), c ? c->data() : nullptr, a.size(), op, 0));
    return out;
  }
  std::vector<BigInteger256> add(const std::vector<BigInteger256>& a, const std::vector<BigInteger256>& b) const { return vec_op(0, a, b); }
  std::vector<BigInteger256> sub(const std::vector<BigInteger256>& a, const std::vector<BigInteger256>& b) const { return vec_op(1, a, b); }
  std::vector<BigInteger256> mul_sub(const std::vector<BigInteger256>& a, const std::vector<BigInteger256>& b, const std::vector<BigInteger256>& c) const {
    return vec_op(2, a, b, &c);
  }
  std::vector<BigInteger256> scale(const std::vector<BigInteger256>& a, const BigInteger256& s) const {
    std::vector<BigInteger256> out(a.size());
    check(mi355_msm_domain_vec_op(handle, out.data(), a.data(), &s, nullptr, a.size(), 3, 0));
    return out;
  }
  // DensePolynomial::evaluate
  BigInteger256 evaluate(const std::vector<BigInteger256>& coeffs, const BigInteger256& z) const {
    BigInteger256 out;
    check(mi355_msm_domain_evaluate(handle, &out, coeffs.data(), coeffs.size(), &z, 0));
    return out;
  }
  // (p - p(z)) / (X - z): coeffs.size() - 1 coefficients; *rem = p(z)
  std::vector<BigInteger256> divide_by_linear(const std::vector<BigInteger256>& coeffs, const BigInteger256& z, BigInteger256* rem = nullptr) const {
    std::vector<BigInteger256> q(coeffs.empty() ? 0 : coeffs.size() - 1);
    check(mi355_msm_domain_divide_by_linear(handle, q.data(), rem, coeffs.data(), coeffs.size(), &z, 0));
    return q;
  }
  std::vector<BigInteger256> evaluate_all_lagrange_coefficients(const BigInteger256& tau) const {
    std::vector<BigInteger256> out(size());
    check(mi355_msm_domain_lagrange(handle, out.data(), &tau, 0));
    return out;
  }
  BigInteger256 evaluate_vanishing_polynomial(const BigInteger256& tau) const {
    BigInteger256 out;
    check(mi355_msm_domain_vanishing(handle, &out, &tau, 0));
    return out;
  }
  // divide_by_vanishing_poly_on_coset_in_place; offset NULL: GENERATOR
  std::vector<BigInteger256> divide_by_vanishing_poly_on_coset(const std::vector<BigInteger256>& evals, const BigInteger256* offset = nullptr) const {
    std::vector<BigInteger256> out(evals.size());
    check(mi355_msm_domain_divide_by_vanishing_on_coset(handle, out.data(), evals.data(), evals.size(), offset, 0));
    return out;
  }
  // the running product (op 0) or sum (op 1): exclusive unless `inclusive`; zeros are not skipped; *total = the combination of all of v
  std::vector<BigInteger256> scan(unsigned op, const std::vector<BigInteger256>& v, bool inclusive = false, BigInteger256* total = nullptr) const {
    std::vector<BigInteger256> out(v.size());
    check(mi355_msm_domain_scan(handle, out.data(), total, v.data(), v.size(), op, inclusive ? 2u : 0u));
    return out;
  }
  std::vector<BigInteger256> prefix_product(const std::vector<BigInteger256>& v, bool inclusive = false, BigInteger256* total = nullptr) const {
    return scan(0, v, inclusive, total);
  }
  std::vector<BigInteger256> prefix_sum(const std::vector<BigInteger256>& v, bool inclusive = false, BigInteger256* total = nullptr) const {
    return scan(1, v, inclusive, total);
  }
  // the Plonk permutation grand product z over the size() rows: wires and sigmas hold ks.size() columns `stride` >= size() elements
  // apart; *total = z[n-1] f[n-1], 1 exactly when the copy constraints hold.  A zero denominator zeroes the rest of z and *total.
  std::vector<BigInteger256> permutation_product(const std::vector<BigInteger256>& wires, const std::vector<BigInteger256>& sigmas, size_t stride,
                                                 const std::vector<BigInteger256>& ks, const BigInteger256& beta, const BigInteger256& gamma,
                                                 BigInteger256* total = nullptr) const {
    const size_t n = size();
    if (ks.empty()) throw std::invalid_argument("permutation_product: ks is empty");
    if (stride < n) throw std::invalid_argument("permutation_product: stride is below the domain size");
    if (!detail::holds_columns(wires.size(), ks.size(), stride, n))
      throw std::invalid_argument("permutation_product: wires holds fewer than ks.size() columns of size() elements");
    if (!detail::holds_columns(sigmas.size(), ks.size(), stride, n))
      throw std::invalid_argument("permutation_product: sigmas holds fewer than ks.size() columns of size() elements");
    std::vector<BigInteger256> out(size());
    check(mi355_msm_domain_permutation_product(handle, out.data(), total, wires.data(), sigmas.data(), ks.size(), stride, ks.data(), &beta, &gamma, 0));
    return out;
  }
  // the rows of a TurboPlonk quotient on THIS domain as the quotient domain (size() = M, n = the constraint domain's size, M / n in
  // 2, 4, 8, 16): wires and sigmas hold ks.size() columns of coset evaluations `stride` >= size() elements apart, selectors is empty
  // (the gate is pi alone) or holds the 13 columns q_lc, q_mul, q_hash, q_o, q_c, q_ecc beside 5 wires; pi may be empty (0)
  std::vector<BigInteger256> plonk_quotient(const std::vector<BigInteger256>& wires, const std::vector<BigInteger256>& sigmas,
                                            const std::vector<BigInteger256>& selectors, const std::vector<BigInteger256>& z,
                                            const std::vector<BigInteger256>& pi, size_t stride, size_t n, const std::vector<BigInteger256>& ks,
                                            const BigInteger256& alpha, const BigInteger256& beta, const BigInteger256& gamma,
                                            const BigInteger256* offset = nullptr) const {
    const size_t M = size();
    if (ks.empty()) throw std::invalid_argument("plonk_quotient: ks is empty");
    if (stride < M) throw std::invalid_argument("plonk_quotient: stride is below the domain size");
    if (!detail::holds_columns(wires.size(), ks.size(), stride, M))
      throw std::invalid_argument("plonk_quotient: wires holds fewer than ks.size() columns of size() elements");
    if (!detail::holds_columns(sigmas.size(), ks.size(), stride, M))
      throw std::invalid_argument("plonk_quotient: sigmas holds fewer than ks.size() columns of size() elements");
    if (!selectors.empty() && !detail::holds_columns(selectors.size(), 13, stride, M))
      throw std::invalid_argument("plonk_quotient: selectors holds fewer than 13 columns of size() elements");
    if (z.size() < M) throw std::invalid_argument("plonk_quotient: z holds fewer than size() elements");
    if (!pi.empty() && pi.size() < M) throw std::invalid_argument("plonk_quotient: pi holds fewer than size() elements");
    std::vector<BigInteger256> out(size());
    check(mi355_msm_domain_plonk_quotient(handle, out.data(), wires.data(), sigmas.data(), selectors.empty() ? nullptr : selectors.data(), z.data(),
                                          pi.empty() ? nullptr : pi.data(), ks.size(), stride, n, ks.data(), &alpha, &beta, &gamma, offset, 0));
    return out;
  }
  // sum_j coeffs[j] * cols[j][i], as long as the longest column; a column contributes 0 past its end
  std::vector<BigInteger256> linear_combination(const std::vector<std::vector<BigInteger256>>& cols, const std::vector<BigInteger256>& coeffs) const {
    std::vector<const void*> ptrs;
    std::vector<size_t> lens;
    size_t n = 0;
    for (const auto& c : cols) {
      ptrs.push_back(c.data());
      lens.push_back(c.size());
      n = c.size() > n ? c.size() : n;
    }
    if (coeffs.size() != cols.size()) throw std::invalid_argument("linear_combination: coeffs holds one element per column");
    std::vector<BigInteger256> out(n);
    check(mi355_msm_domain_linear_combination(handle, out.data(), ptrs.data(), lens.data(), coeffs.data(), cols.size(), 0));
    return out;
  }
  ~Radix2EvaluationDomain() {
    if (handle) {
      RustError e = mi355_msm_domain_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

// arkworks' Matrix<F> = Vec<Vec<(F, usize)>> resident on the GPU (mi355_msm_sparse_*): the R1CS matrices of a proving key, uploaded once
// on a domain that outlives them; apply is y = M z, the evaluate_constraint loop of ark-groth16's witness map.  CSR: row_ptr holds
// rows + 1 offsets, col_idx and values one entry per coefficient (Fr values in Montgomery form).
struct SparseMatrix {
  mi355_msm_sparse* handle = nullptr;
  SparseMatrix(const Radix2EvaluationDomain& dom, size_t rows, size_t cols, const std::vector<uint64_t>& row_ptr, const std::vector<uint32_t>& col_idx,
               const std::vector<BigInteger256>& values) {
    if (row_ptr.empty() || row_ptr.size() - 1 != rows) throw std::invalid_argument("SparseMatrix: row_ptr holds rows + 1 offsets");
    if (col_idx.size() != row_ptr.back()) throw std::invalid_argument("SparseMatrix: col_idx holds row_ptr.back() entries");
    if (values.size() != row_ptr.back()) throw std::invalid_argument("SparseMatrix: values holds row_ptr.back() entries");
    check(mi355_msm_sparse_create(&handle, dom.handle, rows, cols, row_ptr.data(), col_idx.data(), values.data(), 0));
  }
  SparseMatrix(const SparseMatrix&) = delete;
  SparseMatrix& operator=(const SparseMatrix&) = delete;
  SparseMatrix(SparseMatrix&& o) noexcept : handle(o.handle) { o.handle = nullptr; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_sparse_query(handle, key, &v));
    return v;
  }
  size_t rows() const { return (size_t)query("rows"); }
  size_t cols() const { return (size_t)query("cols"); }
  // y[i] = sum_k values[k] * z[col_idx[k]] over the entries of row i; z holds cols() elements
  std::vector<BigInteger256> apply(const std::vector<BigInteger256>& z) const {
    if (z.size() != cols()) throw std::invalid_argument("SparseMatrix::apply: z holds cols() elements");
    std::vector<BigInteger256> out(rows());
    check(mi355_msm_sparse_apply(handle, out.data(), z.data(), 0, nullptr));
    return out;
  }
  ~SparseMatrix() {
    if (handle) {
      RustError e = mi355_msm_sparse_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

// A lookup table over Fr resident on the GPU (mi355_msm_lookup_*), on a domain that outlives it: multiplicities are logUp's m, sorted is
// plookup's s = (f, t) sorted by t (Jellyfish's h1 = s[:n], h2 = s[n-1:] are slices of it).  Fr values in Montgomery form; equality is
// equality modulo r, duplicates are credited to their first occurrence, and a missing value is reported, not an error.
struct LookupTable {
  mi355_msm_lookup* handle = nullptr;
  size_t n = 0;
  struct Counts {
    std::vector<BigInteger256> mult;
    std::vector<uint32_t> index;
    uint64_t missing = 0, first_missing = 0;
  };
  LookupTable(const Radix2EvaluationDomain& dom, const std::vector<BigInteger256>& table) : n(table.size()) {
    check(mi355_msm_lookup_create(&handle, dom.handle, table.data(), table.size(), 0, nullptr));
  }
  LookupTable(const LookupTable&) = delete;
  LookupTable& operator=(const LookupTable&) = delete;
  LookupTable(LookupTable&& o) noexcept : handle(o.handle), n(o.n) { o.handle = nullptr; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_lookup_query(handle, key, &v));
    return v;
  }
  Counts multiplicities(const std::vector<BigInteger256>& values) const {
    Counts c;
    c.mult.resize(n);
    c.index.resize(values.size());
    uint64_t stats[2] = {0, 0};
    check(mi355_msm_lookup_count(handle, c.mult.data(), c.index.data(), stats, values.data(), values.size(), 0, nullptr));
    c.missing = stats[0];
    c.first_missing = stats[1];
    return c;
  }
  // empty, with *first_missing set, when a value is not in the table
  std::vector<BigInteger256> sorted(const std::vector<BigInteger256>& values, uint64_t* first_missing = nullptr) const {
    std::vector<BigInteger256> s(n + values.size());
    uint64_t stats[2] = {0, 0};
    check(mi355_msm_lookup_sorted(handle, s.data(), stats, values.data(), values.size(), 0, nullptr));
    if (stats[0]) {
      if (first_missing) *first_missing = stats[1];
      s.clear();
    }
    return s;
  }
  ~LookupTable() {
    if (handle) {
      RustError e = mi355_msm_lookup_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

// A custom-gate expression compiled for the GPU (mi355_msm_expr_*), on a domain that outlives it: nodes are (op, a, b) triples in
// topological order, the last one the result (0 COL column a at the signed rotation b, 1 CONST, 2 CHAL, 3 ADD, 4 SUB, 5 MUL, 6 NEG,
// 7 SQR); one launch of run evaluates it for every row.  Fr values in Montgomery form.
struct GateProgram {
  mi355_msm_expr* handle = nullptr;
  size_t n_cols = 0, n_chal = 0;
  GateProgram(const Radix2EvaluationDomain& dom, const std::vector<uint32_t>& nodes, const std::vector<BigInteger256>& consts, size_t n_chal_, size_t n_cols_)
      : n_cols(n_cols_), n_chal(n_chal_) {
    if (nodes.size() % 3) throw std::invalid_argument("GateProgram: nodes holds (op, a, b) triples");
    check(mi355_msm_expr_create(&handle, dom.handle, nodes.data(), nodes.size() / 3, consts.empty() ? nullptr : consts.data(), consts.size(), n_chal, n_cols, 0));
  }
  GateProgram(const GateProgram&) = delete;
  GateProgram& operator=(const GateProgram&) = delete;
  GateProgram(GateProgram&& o) noexcept : handle(o.handle), n_cols(o.n_cols), n_chal(o.n_chal) { o.handle = nullptr; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_expr_query(handle, key, &v));
    return v;
  }
  // out[i] for i < the longest column; column j at rotation rot is read at row ((i + rot * rot_step) mod len) mod cols[j].size()
  std::vector<BigInteger256> run(const std::vector<std::vector<BigInteger256>>& cols, const std::vector<BigInteger256>& challenges, size_t rot_step = 1) const {
    std::vector<const void*> ptrs;
    std::vector<size_t> lens;
    size_t len = 0;
    for (const auto& c : cols) {
      ptrs.push_back(c.data());
      lens.push_back(c.size());
      len = c.size() > len ? c.size() : len;
    }
    std::vector<BigInteger256> out(len);
    check(mi355_msm_expr_run(handle, out.data(), ptrs.data(), lens.data(), cols.size(), len, rot_step, challenges.empty() ? nullptr : challenges.data(),
                             challenges.size(), 0, nullptr));
    return out;
  }
  ~GateProgram() {
    if (handle) {
      RustError e = mi355_msm_expr_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

// phi[0] = 0, phi[j+1] = phi[j] + sum_c 1 / (beta + columns[c][j]) - mult[j] / (beta + table[j]); *total is zero exactly when the
// multiset relation holds.  A zero denominator contributes 0.
inline std::vector<BigInteger256> logup_sum(const Radix2EvaluationDomain& dom, const std::vector<BigInteger256>& table, const std::vector<BigInteger256>& mult,
                                            const std::vector<std::vector<BigInteger256>>& columns, const BigInteger256& beta, BigInteger256* total = nullptr) {
  const size_t n = table.size();
  if (mult.size() != n) throw std::invalid_argument("logup_sum: mult holds one element per table row");
  if (columns.empty()) throw std::invalid_argument("logup_sum: columns is empty");
  std::vector<BigInteger256> flat, phi(n);
  for (const auto& c : columns) {
    if (c.size() != n) throw std::invalid_argument("logup_sum: every one of columns holds one element per table row");
    flat.insert(flat.end(), c.begin(), c.end());
  }
  check(mi355_msm_domain_logup_sum(dom.handle, phi.data(), total, nullptr, table.data(), mult.data(), flat.data(), columns.size(), n, n, &beta, 0, nullptr));
  return phi;
}

// ark-groth16's LibsnarkReduction::witness_map on host vectors, from the full assignment z to the size() coefficients of h: a = A z with
// z[0 .. num_inputs) appended behind the constraints, b = B z, c = a * b element by element, all zero-padded to the domain;
// h = coset_ifft((coset_fft(ifft(a)) * coset_fft(ifft(b)) - coset_fft(ifft(c))) / Z(g)).  (The Python layer keeps every step in device memory.)
inline std::vector<BigInteger256> groth16_witness_map(const Radix2EvaluationDomain& dom, const SparseMatrix& A, const SparseMatrix& B,
                                                      const std::vector<BigInteger256>& z, size_t num_inputs) {
  if (num_inputs > z.size()) throw std::invalid_argument("groth16_witness_map: z holds fewer than num_inputs elements");
  std::vector<BigInteger256> a = A.apply(z), b = B.apply(z);
  if (a.size() + num_inputs > dom.size() || b.size() > dom.size())
    throw std::invalid_argument("groth16_witness_map: the constraints and the inputs of z do not fit the domain");
  a.insert(a.end(), z.begin(), z.begin() + num_inputs);
  a.resize(dom.size());
  b.resize(dom.size());
  const std::vector<BigInteger256> c = dom.mul(a, b);
  const std::vector<BigInteger256> h = dom.mul_sub(dom.coset_fft(dom.ifft(a)), dom.coset_fft(dom.ifft(b)), dom.coset_fft(dom.ifft(c)));
  return dom.coset_ifft(dom.divide_by_vanishing_poly_on_coset(h));
}

// snarkVM's PoseidonSponge, Poseidon::hash_many and its Poseidon Merkle tree for batches on the GPU (mi355_msm_poseidon_*): the caller
// supplies the round constants (one row of rate + 1 per round) and the MDS matrix as Fr values in Montgomery form, uploaded once on a
// domain that outlives them.
struct Poseidon {
  mi355_msm_poseidon* handle = nullptr;
  unsigned rate;
  Poseidon(const Radix2EvaluationDomain& dom, unsigned rate_, unsigned alpha, unsigned full_rounds, unsigned partial_rounds,
           const std::vector<BigInteger256>& ark, const std::vector<BigInteger256>& mds)
      : rate(rate_) {
    if (ark.size() != (size_t)(full_rounds + partial_rounds) * (rate + 1) || mds.size() != (size_t)(rate + 1) * (rate + 1))
      throw std::invalid_argument("ark: one row of rate + 1 constants per round; mds: rate + 1 rows of rate + 1");
    check(mi355_msm_poseidon_create(&handle, dom.handle, rate, alpha, full_rounds, partial_rounds, ark.data(), mds.data(), 0));
  }
  Poseidon(const Poseidon&) = delete;
  Poseidon& operator=(const Poseidon&) = delete;
  Poseidon(Poseidon&& o) noexcept : handle(o.handle), rate(o.rate) { o.handle = nullptr; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_poseidon_query(handle, key, &v));
    return v;
  }
  // n = in.size() / in_len sponges: absorb the header (empty, or `rate` elements) and a row, squeeze n_out elements
  std::vector<BigInteger256> hash(const std::vector<BigInteger256>& in, size_t in_len, size_t n_out,
                                  const std::vector<BigInteger256>& header = {}) const {
    if (!header.empty() && header.size() != rate) throw std::invalid_argument("a header holds `rate` elements");
    const size_t n = in_len ? in.size() / in_len : 1;
    if (n * in_len != in.size()) throw std::invalid_argument("whole rows of in_len elements");
    std::vector<BigInteger256> out(n * n_out);
    check(mi355_msm_poseidon_hash(handle, out.data(), in.data(), n, in_len, n_out, header.empty() ? nullptr : header.data(), 0, nullptr));
    return out;
  }
  // the 2P - 1 nodes of the Poseidon Merkle tree under the domain separator, root of the built part first
  std::vector<BigInteger256> merkle_tree(const BigInteger256& domain_sep, const std::vector<BigInteger256>& leaves, size_t leaf_len) const {
    if (!leaf_len || leaves.empty() || leaves.size() % leaf_len) throw std::invalid_argument("whole leaves of leaf_len elements");
    const size_t n = leaves.size() / leaf_len;
    size_t P = 1;
    while (P < n) P *= 2;
    std::vector<BigInteger256> out(2 * P - 1);
    check(mi355_msm_poseidon_merkle(handle, out.data(), leaves.data(), n, leaf_len, &domain_sep, 0, nullptr));
    return out;
  }
  ~Poseidon() {
    if (handle) {
      RustError e = mi355_msm_poseidon_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

// Bls12::pairing and product_of_pairings for batches on the GPU (mi355_msm_pairing_*): g1 holds n arkworks Affine<G1> images of 104
// bytes, g2 n Affine<G2> images of 200; a Gt value is 576 bytes, arkworks' in-memory Fq12 or -- canonical -- its CanonicalSerialize.
// The points must be of order r or flagged infinity; nothing is tested.
struct Pairing {
  mi355_msm_pairing* handle = nullptr;
  static constexpr size_t GT_BYTES = 576;
  explicit Pairing(int curve = MI355_BLS12_377_G1, int device = -1) { check(mi355_msm_pairing_create(&handle, curve, device)); }
  Pairing(const Pairing&) = delete;
  Pairing& operator=(const Pairing&) = delete;
  Pairing(Pairing&& o) noexcept : handle(o.handle) { o.handle = nullptr; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_pairing_query(handle, key, &v));
    return v;
  }
  // out[j] = prod_{i < group} e(P[j group + i], Q[j group + i]): n / group images
  std::vector<uint8_t> pairing(const std::vector<uint8_t>& g1, const std::vector<uint8_t>& g2, size_t group = 1, bool canonical = false) const {
    const size_t n = g1.size() / 104;
    if (g1.size() % 104 || g2.size() != n * 200 || !group || n % group) throw std::invalid_argument("n images of 104 and of 200 bytes, whole groups");
    std::vector<uint8_t> out(n / group * GT_BYTES);
    check(mi355_msm_pairing_run(handle, out.data(), g1.data(), 104, g2.data(), 200, n, group, canonical ? 1u : 0u, nullptr));
    return out;
  }
  std::vector<uint8_t> product_of_pairings(const std::vector<uint8_t>& g1, const std::vector<uint8_t>& g2, bool canonical = false) const {
    if (g1.empty()) throw std::invalid_argument("at least one pair");
    return pairing(g1, g2, g1.size() / 104, canonical);
  }
  // one byte per group: 1 exactly when the product over the group is one
  std::vector<uint8_t> check_groups(const std::vector<uint8_t>& g1, const std::vector<uint8_t>& g2, size_t group) const {
    const size_t n = g1.size() / 104;
    if (g1.size() % 104 || g2.size() != n * 200 || !group || n % group) throw std::invalid_argument("n images of 104 and of 200 bytes, whole groups");
    std::vector<uint8_t> ok(n / group);
    check(mi355_msm_pairing_check(handle, ok.data(), g1.data(), 104, g2.data(), 200, n, group, 0, nullptr));
    return ok;
  }
  ~Pairing() {
    if (handle) {
      RustError e = mi355_msm_pairing_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

// RFC 9380 hash-to-curve for batches on the GPU (mi355_msm_h2c_*): hash_to_curve / encode_to_curve / hash_to_field / map_to_curve for
// MI355_BLS12_381_G1 or MI355_BLS12_381_G2 and one domain separation tag.  Messages are host byte strings; points come back as arkworks
// Affine images (104 / 200 bytes), field elements as 48-byte Montgomery images.
struct HashToCurve {
  mi355_msm_h2c* handle = nullptr;
  int curve;
  HashToCurve(int curve_, const std::string& dst, int device = -1) : curve(curve_) {
    check(mi355_msm_h2c_create(&handle, curve, dst.data(), dst.size(), device));
  }
  HashToCurve(const HashToCurve&) = delete;
  HashToCurve& operator=(const HashToCurve&) = delete;
  HashToCurve(HashToCurve&& o) noexcept : handle(o.handle), curve(o.curve) { o.handle = nullptr; }
  size_t m() const { return curve >= 2 ? 2 : 1; }
  size_t image_bytes() const { return 96 * m() + 8; }
  uint64_t query(const char* key) const {
    uint64_t v = 0;
    check(mi355_msm_h2c_query(handle, key, &v));
    return v;
  }
  static void pack(const std::vector<std::string>& msgs, std::vector<uint8_t>& data, std::vector<uint64_t>& off) {
    off.assign(1, 0);
    for (const std::string& s : msgs) {
      data.insert(data.end(), s.begin(), s.end());
      off.push_back(data.size());
    }
  }
  // hash_to_curve (encode = false) or encode_to_curve: one Affine image per message
  std::vector<uint8_t> hash(const std::vector<std::string>& msgs, bool encode = false) const {
    std::vector<uint8_t> data, out(msgs.size() * image_bytes());
    std::vector<uint64_t> off;
    pack(msgs, data, off);
    check(mi355_msm_h2c_hash(handle, out.data(), image_bytes(), data.data(), data.size(), off.data(), msgs.size(), encode ? 1u : 0u, nullptr));
    return out;
  }
  // hash_to_field: count * m images of 48 bytes per message
  std::vector<uint8_t> hash_to_field(const std::vector<std::string>& msgs, unsigned count = 2) const {
    std::vector<uint8_t> data, out(msgs.size() * count * m() * 48);
    std::vector<uint64_t> off;
    pack(msgs, data, off);
    check(mi355_msm_h2c_field(handle, out.data(), data.data(), data.size(), off.data(), msgs.size(), count, 0, nullptr));
    return out;
  }
  // map_to_curve of n field images; pairs: n / 2 points clear_cofactor(map(u[2j]) + map(u[2j + 1]))
  std::vector<uint8_t> map_to_curve(const std::vector<uint8_t>& u, bool pairs = false) const {
    const size_t n = u.size() / (48 * m());
    if (u.size() % (48 * m()) || (pairs && (n & 1))) throw std::invalid_argument("n field images of 48 m bytes, whole pairs");
    std::vector<uint8_t> out((pairs ? n / 2 : n) * image_bytes());
    check(mi355_msm_h2c_map(handle, out.data(), image_bytes(), u.data(), n, pairs ? 4u : 0u, nullptr));
    return out;
  }
  ~HashToCurve() {
    if (handle) {
      RustError e = mi355_msm_h2c_destroy(handle);
      if (e.message) std::free(e.message);
    }
  }
};

// ark-poly's DenseMultilinearExtension and the prover of ark-linear-sumcheck's ListOfProductsOfPolynomials on host vectors
// (mi355_msm_domain_mle_fix, _mle_eq, _sumcheck_round): a table holds 2^nv evaluations, index b the point (b_0, .., b_{nv-1}) with b_0 the
// lowest bit, and variables are fixed from the lowest bit upward.  The domain lends its field and its device; its size plays no part.
inline unsigned mle_num_vars(size_t len) {
  unsigned nv = 0;
  while (((size_t)1 << nv) < len) nv++;
  if (((size_t)1 << nv) != len) throw std::invalid_argument("a table holds 2^num_vars elements");
  return nv;
}

inline std::vector<BigInteger256> mle_fix_variables(const Radix2EvaluationDomain& dom, const std::vector<BigInteger256>& evals,
                                                    const std::vector<BigInteger256>& point) {
  const unsigned nv = mle_num_vars(evals.size());
  if (point.size() > nv) throw std::invalid_argument("more values than variables");
  std::vector<BigInteger256> out(evals.size() >> point.size());
  check(mi355_msm_domain_mle_fix(dom.handle, out.data(), evals.data(), nv, point.data(), (unsigned)point.size(), 0, nullptr));
  return out;
}

inline BigInteger256 mle_evaluate(const Radix2EvaluationDomain& dom, const std::vector<BigInteger256>& evals, const std::vector<BigInteger256>& point) {
  if (point.size() != mle_num_vars(evals.size())) throw std::invalid_argument("one value per variable");
  return mle_fix_variables(dom, evals, point)[0];
}

inline std::vector<BigInteger256> eq_table(const Radix2EvaluationDomain& dom, const std::vector<BigInteger256>& point) {
  std::vector<BigInteger256> out((size_t)1 << point.size());
  check(mi355_msm_domain_mle_eq(dom.handle, out.data(), point.data(), (unsigned)point.size(), 0, nullptr));
  return out;
}

// one term c * prod_k f_k of g: the coefficient and the indices of its factors (at most 5; a repeated index is a power)
struct SumcheckTerm {
  BigInteger256 coeff;
  std::vector<uint32_t> factors;
};

// One prover round for g = sum_j c_j prod_k f_k over m tables of 2^nv elements: the d + 1 evaluations P(0) .. P(d).  With r_prev the
// tables are folded by it first, in the same pass, `folded` receives the m halved tables and the evaluations are those of the folded
// tables.
inline std::vector<BigInteger256> sumcheck_round(const Radix2EvaluationDomain& dom, const std::vector<std::vector<BigInteger256>>& tables,
                                                 const std::vector<SumcheckTerm>& terms, const BigInteger256* r_prev = nullptr,
                                                 std::vector<std::vector<BigInteger256>>* folded = nullptr) {
  if (tables.empty()) throw std::invalid_argument("no tables");
  const size_t n = tables[0].size();
  const unsigned nv = mle_num_vars(n);
  std::vector<mi355_msm_sumcheck_term> recs(terms.size());
  size_t d = 0;
  for (size_t j = 0; j < terms.size(); j++) {
    if (terms[j].factors.empty() || terms[j].factors.size() > 5) throw std::invalid_argument("a term takes 1 .. 5 factors");
    std::memcpy(recs[j].coeff, &terms[j].coeff, 32);
    recs[j].n_factors = (uint32_t)terms[j].factors.size();
    for (size_t q = 0; q < 5; q++) recs[j].factors[q] = q < terms[j].factors.size() ? terms[j].factors[q] : 0;
    d = std::max(d, terms[j].factors.size());
  }
  std::vector<const void*> ptrs;
  for (const auto& t : tables) {
    if (t.size() != n) throw std::invalid_argument("the tables differ in length");
    ptrs.push_back(t.data());
  }
  std::vector<void*> fptrs;
  if (r_prev) {
    if (!folded) throw std::invalid_argument("r_prev needs a place for the folded tables");
    folded->assign(tables.size(), std::vector<BigInteger256>(n / 2));
    for (auto& t : *folded) fptrs.push_back(t.data());
  }
  std::vector<BigInteger256> evals(6);
  check(mi355_msm_domain_sumcheck_round(dom.handle, evals.data(), ptrs.data(), ptrs.size(), nv, recs.data(), recs.size(), r_prev,
                                        r_prev ? fptrs.data() : nullptr, 0, nullptr));
  evals.resize(d + 1);
  return evals;
}

// domain.fft / ifft / coset_fft / coset_ifft on a vector of G1 points (mi355_msm_fft_points): kind 0 .. 3 as for Fr; `points` may be
// shorter than the domain (the rest is the point at infinity); offset NULL: GENERATOR.  Affine images out, ready for
// multi_scalar_mult_init -- kind 1 on a monomial SRS [tau^j] G gives the Lagrange SRS [L_i(tau)] G.
inline std::vector<G1Affine> fft_points(MultiScalarMultContext& ctx, const Radix2EvaluationDomain& dom, const std::vector<G1Affine>& points, unsigned kind = 0,
                                        const BigInteger256* offset = nullptr) {
  std::vector<G1Affine> out(dom.size());
  check(mi355_msm_fft_points(ctx.context, dom.handle, out.data(), sizeof(G1Affine), points.data(), points.size(), sizeof(G1Affine), kind, 0u, offset));
  return out;
}
inline std::vector<G1Affine> ifft_points(MultiScalarMultContext& ctx, const Radix2EvaluationDomain& dom, const std::vector<G1Affine>& points) {
  return fft_points(ctx, dom, points, 1);
}

}  // namespace mi355
