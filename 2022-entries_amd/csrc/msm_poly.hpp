// msm_poly.hpp -- the calls between a transform and an MSM on the domain handle (included by msm_engine.hip after msm_ntt.hpp): the C
// ABI mi355_msm_domain_{batch_inverse, vec_op, evaluate, divide_by_linear, lagrange, vanishing, divide_by_vanishing_on_coset} of
// include/mi355_msm.h over the kernels of poly.hpp.
//
// Reference: ARK ff/src/fields/mod.rs:811-873, poly/src/polynomial/univariate/dense.rs:41-94, poly/src/polynomial/univariate/mod.rs:102,
// poly/src/domain/radix2/mod.rs:141-216, poly/src/domain/mod.rs:190-197.  Every call judges its arguments first (the handle last, so the
// other errors read the same with and without one), derives its constants in host arithmetic (the powers z^(2^i), n / Z(tau),
// 1 / Z(g)) and enqueues separate launches on one stream.  The partial vectors of the scans live in `poly` (allocated on the first such
// call, kept by the handle: query "poly_work_bytes"); host-pointer calls stage whole vectors through `pstage`, with the FrStage of
// fr_stage.hpp, which every call body below uses to name each of its vectors once, whichever kind of pointer the caller brought.
#pragma once

#include "launch_poly.hpp"

namespace {

constexpr size_t kPolyMaxN = (size_t)1 << POLY_MAX_LOG;

template <class FR>
struct PolyRun {
  hipStream_t st;
  void eval(const PolyEval& p) { HIP_OK(LaunchPoly<FR>::eval(p, st)); }
  void div(const PolyDiv& p) { HIP_OK(LaunchPoly<FR>::div(p, st)); }
  void inv_prod(const PolyInv& p) { HIP_OK(LaunchPoly<FR>::inv_prod(p, st)); }
  void inv_tiles(Fr* tiles, uint64_t count, const Fr& coeff) { HIP_OK(LaunchPoly<FR>::inv_tiles(tiles, count, coeff, st)); }
  void inv_apply(const PolyInv& p) { HIP_OK(LaunchPoly<FR>::inv_apply(p, st)); }
};

void poly_check_flags(unsigned flags, size_t n) {
  if (flags & ~kPolyNormal) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements)", flags);
  if (n > kPolyMaxN) bad_arg("%zu elements exceed 2^30", n);
}

bool poly_overlap(const void* a, size_t a_elems, const void* b, size_t b_elems) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && a_elems && b_elems && x < y + b_elems * 32 && y < x + a_elems * 32;
}

// out against one input of the same length: the same vector or disjoint
void poly_check_alias(const void* out, const void* in, size_t n, const char* name) {
  if (out != in && poly_overlap(out, n, in, n)) bad_arg("the output overlaps %s in part (out == %s is allowed)", name, name);
}

void poly_check_aligned(bool device_ptrs, std::initializer_list<const void*> ptrs) {
  if (!device_ptrs) return;
  for (const void* p : ptrs)
    if ((uintptr_t)p & 3) bad_arg("device pointers must be 4-byte aligned");
}

// the calls that take the pointer kind as a flag bit (msm_mle.hpp, msm_sparse.hpp, msm_poseidon.hpp) take a stream with it
void poly_check_stream(bool device_ptrs, hipStream_t st) {
  if (!device_ptrs && st) bad_arg("a stream goes with device pointers (flag bit 1) only");
}

void poly_check_handle(mi355_msm_domain* d) {
  if (!d) bad_arg("null domain handle");
}

Fr* poly_work(mi355_msm_domain* d, size_t n) {
  d->poly.reserve((size_t)poly_work_elems(n, d->poly_tile_log) * sizeof(Fr));
  return d->poly.as<Fr>();
}

// events, the host clock and the synchronisation around what fn enqueues on st
template <class Fn>
void poly_timed(mi355_msm_domain* d, hipStream_t st, Fn&& fn) {
  HIP_OK(hipSetDevice(d->device));
  const auto t0 = std::chrono::steady_clock::now();
  try {
    HIP_OK(hipEventRecord(d->ev[0], st));
    fn();
    HIP_OK(hipEventRecord(d->ev[1], st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  domain_finish(d, t0);
}

// a class-M element of device memory, after the stream is idle, as 32 host bytes in the form of the call
void poly_fetch(mi355_msm_domain* d, void* out32, const Fr* dev, unsigned flags) {
  Fr x;
  HIP_OK(hipMemcpy(&x, dev, sizeof x, hipMemcpyDeviceToHost));
  with_fr(d->curve, [&]<class FR>() { poly_scalar_out<FR>(out32, x, (flags & kPolyNormal) != 0); });
}

// ---- batch inversion --------------------------------------------------------------------------------------------------------------

void poly_inverse_check(mi355_msm_domain* d, const void* out, const void* in, size_t n, unsigned flags, bool device_ptrs) {
  poly_check_flags(flags, n);
  if (n && (!out || !in)) bad_arg("null input or output pointer");
  poly_check_alias(out, in, n, "in");
  poly_check_aligned(device_ptrs, {out, in});
  poly_check_handle(d);
}

void poly_inverse_enqueue(mi355_msm_domain* d, uint32_t* out, const uint32_t* in, size_t n, const void* coeff, unsigned flags, hipStream_t st) {
  const bool normal = (flags & kPolyNormal) != 0;
  Fr* work = poly_work(d, n);
  with_fr(d->curve, [&]<class FR>() {
    Fr c;
    if (coeff) poly_scalar<FR>(c, coeff, normal); else fr_set<FR>(c, FR::ONE);
    PolyRun<FR> run{st};
    poly_chain_inverse<FR>(run, out, in, n, normal, d->poly_tile_log, c, work);
  });
}

void poly_inverse(mi355_msm_domain* d, void* out, const void* in, size_t n, const void* coeff, unsigned flags, bool device_ptrs, hipStream_t st) {
  poly_inverse_check(d, out, in, n, flags, device_ptrs);
  if (n == 0) return;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->pstage, device_ptrs, on, n);
    const uint32_t* src = g.in(in, n);
    uint32_t* dst = g.out_over(out, src);
    poly_inverse_enqueue(d, dst, src, n, coeff, flags, on);
    g.back(out, dst, n);
  });
}

// ---- element-wise -----------------------------------------------------------------------------------------------------------------

// b is a vector for the sum, the difference and a*b - c, and ONE HOST ELEMENT for the scaling; c is read by a*b - c only
void poly_vec_check(mi355_msm_domain* d, const void* out, const void* a, const void* b, const void* c, size_t n, unsigned op, unsigned flags,
                    bool device_ptrs) {
  poly_check_flags(flags, n);
  if (op > kPolyScale) bad_arg("unknown element-wise operation %u (0 a + b, 1 a - b, 2 a*b - c, 3 s * a)", op);
  if (op == kPolyScale && !b) bad_arg("null factor pointer");
  if (n && (!out || !a || !b || (op == kPolyMulSub && !c))) bad_arg("null input or output pointer");
  poly_check_alias(out, a, n, "a");
  if (op != kPolyScale) poly_check_alias(out, b, n, "b");
  if (op == kPolyMulSub) poly_check_alias(out, c, n, "c");
  poly_check_aligned(device_ptrs, {out, a, op != kPolyScale ? b : nullptr, op == kPolyMulSub ? c : nullptr});
  poly_check_handle(d);
}

void poly_vec_enqueue(mi355_msm_domain* d, uint32_t* out, const uint32_t* a, const uint32_t* b, const uint32_t* c, size_t n, unsigned op, const Fr& s,
                      unsigned flags, hipStream_t st) {
  with_fr(d->curve, [&]<class FR>() {
    PolyVecOp p{a, b, c, out, n, op, (flags & kPolyNormal) ? 1u : 0u, s};
    HIP_OK(LaunchPoly<FR>::vec_op(p, st));
  });
}

void poly_vec(mi355_msm_domain* d, void* out, const void* a, const void* b, const void* c, size_t n, unsigned op, unsigned flags, bool device_ptrs,
              hipStream_t st) {
  poly_vec_check(d, out, a, b, c, n, op, flags, device_ptrs);
  Fr s;
  fr_zero(s);
  if (op == kPolyScale) with_fr(d->curve, [&]<class FR>() { poly_scalar<FR>(s, b, (flags & kPolyNormal) != 0); });
  if (n == 0) return;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->pstage, device_ptrs, on, 3 * n);
    const uint32_t* da = g.in(a, n);
    const uint32_t* db = op != kPolyScale ? g.in(b, n) : nullptr;
    const uint32_t* dc = op == kPolyMulSub ? g.in(c, n) : nullptr;
    uint32_t* dst = g.out_over(out, da);
    poly_vec_enqueue(d, dst, da, db, dc, n, op, s, flags, on);
    g.back(out, dst, n);
  });
}

// ---- evaluation and division by X - z ---------------------------------------------------------------------------------------------

void poly_eval_check(mi355_msm_domain* d, const void* out32, const void* coeffs, size_t n, const void* z, unsigned flags, bool device_ptrs) {
  poly_check_flags(flags, n);
  if (!out32 || !z || (n && !coeffs)) bad_arg("null input or output pointer");
  poly_check_aligned(device_ptrs, {coeffs});
  poly_check_handle(d);
}

void poly_evaluate(mi355_msm_domain* d, void* out32, const void* coeffs, size_t n, const void* z, unsigned flags, bool device_ptrs, hipStream_t st) {
  poly_eval_check(d, out32, coeffs, n, z, flags, device_ptrs);
  if (n == 0) {
    memset(out32, 0, 32);
    return;
  }
  const bool normal = (flags & kPolyNormal) != 0;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const Fr* res = nullptr;
  poly_timed(d, on, [&] {
    FrStage g(d->pstage, device_ptrs, on, n);
    const uint32_t* src = g.in(coeffs, n);
    Fr* work = poly_work(d, n);
    with_fr(d->curve, [&]<class FR>() {
      Fr zz;
      poly_scalar<FR>(zz, z, normal);
      PolyRun<FR> run{on};
      res = poly_chain_evaluate<FR>(run, src, n, normal, d->poly_tile_log, zz, work);
    });
  });
  poly_fetch(d, out32, res, flags);
}

void poly_divide_check(mi355_msm_domain* d, const void* q, const void* coeffs, size_t n, const void* z, unsigned flags, bool device_ptrs) {
  poly_check_flags(flags, n);
  if (!z || (n && !coeffs) || (n > 1 && !q)) bad_arg("null input or output pointer");
  if (n > 1 && poly_overlap(q, n - 1, coeffs, n)) bad_arg("the quotient overlaps the coefficients (the division is not done in place)");
  poly_check_aligned(device_ptrs, {q, coeffs});
  poly_check_handle(d);
}

void poly_divide(mi355_msm_domain* d, void* q, void* rem32, const void* coeffs, size_t n, const void* z, unsigned flags, bool device_ptrs, hipStream_t st) {
  poly_divide_check(d, q, coeffs, n, z, flags, device_ptrs);
  if (n == 0) {
    if (rem32) memset(rem32, 0, 32);
    return;
  }
  const bool normal = (flags & kPolyNormal) != 0;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const Fr* res = nullptr;
  poly_timed(d, on, [&] {
    FrStage g(d->pstage, device_ptrs, on, 2 * n);
    const uint32_t* src = g.in(coeffs, n);
    uint32_t* dst = g.out(q, n);
    Fr* work = poly_work(d, n);
    with_fr(d->curve, [&]<class FR>() {
      Fr zz;
      poly_scalar<FR>(zz, z, normal);
      PolyRun<FR> run{on};
      res = poly_chain_divide<FR>(run, dst, src, n, normal, d->poly_tile_log, zz, work);
    });
    g.back(q, dst, n - 1);
  });
  if (rem32) poly_fetch(d, rem32, res, flags);
}

// ---- the domain's own polynomials -------------------------------------------------------------------------------------------------

void poly_lagrange(mi355_msm_domain* d, void* out, const void* tau, unsigned flags, bool device_ptrs, hipStream_t st) {
  poly_check_flags(flags, 0);
  if (!out || !tau) bad_arg("null input or output pointer");
  poly_check_aligned(device_ptrs, {out});
  poly_check_handle(d);
  const bool normal = (flags & kPolyNormal) != 0;
  const size_t n = (size_t)1 << d->k;
  const NttLayout at(d->k);
  Fr* t = d->tables.as<Fr>();
  PolyLagrange p{};
  p.k = d->k;
  p.normal = normal ? 1u : 0u;
  p.w = NttTable{t + at.wlo, t + at.whi};
  p.wi = NttTable{t + at.ilo, t + at.ihi};
  with_fr(d->curve, [&]<class FR>() {
    Fr zt, zero;
    fr_zero(zero);
    poly_scalar<FR>(p.tau, tau, normal);
    poly_vanishing<FR>(zt, p.tau, d->k);
    p.in_domain = fr_same(zt, zero) ? 1u : 0u;
    p.c = zero;
    if (!p.in_domain) {   // n / Z(tau) = 1 / (n^-1 Z(tau))
      fr_mul<FR>(zt, zt, d->size_inv);
      fr_reduce<FR>(zt);
      fr_inv<FR>(p.c, zt);
    }
  });
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->pstage, device_ptrs, on, n);
    p.dst = g.out(out, n);
    with_fr(d->curve, [&]<class FR>() { HIP_OK(LaunchPoly<FR>::lagrange(p, on)); });
    if (!p.in_domain) poly_inverse_enqueue(d, p.dst, p.dst, n, nullptr, flags, on);
    g.back(out, p.dst, n);
  });
}

void poly_vanishing_host(mi355_msm_domain* d, void* out32, const void* tau, unsigned flags) {
  poly_check_flags(flags, 0);
  if (!out32 || !tau) bad_arg("null input or output pointer");
  poly_check_handle(d);
  with_fr(d->curve, [&]<class FR>() {
    Fr x, zt;
    poly_scalar<FR>(x, tau, (flags & kPolyNormal) != 0);
    poly_vanishing<FR>(zt, x, d->k);
    poly_scalar_out<FR>(out32, zt, (flags & kPolyNormal) != 0);
  });
}

void poly_divide_vanishing(mi355_msm_domain* d, void* out, const void* in, size_t n, const void* offset, unsigned flags, bool device_ptrs, hipStream_t st) {
  poly_check_flags(flags, n);
  if (n && (!out || !in)) bad_arg("null input or output pointer");
  poly_check_alias(out, in, n, "in");
  poly_check_aligned(device_ptrs, {out, in});
  poly_check_handle(d);
  Fr s;
  with_fr(d->curve, [&]<class FR>() {
    Fr g, zg, zero;
    fr_zero(zero);
    if (offset) poly_scalar<FR>(g, offset, (flags & kPolyNormal) != 0); else fr_set<FR>(g, FR::GENERATOR);
    if (fr_same(g, zero)) bad_arg("the coset offset is zero");
    poly_vanishing<FR>(zg, g, d->k);
    if (fr_same(zg, zero)) bad_arg("the offset lies in the domain: the vanishing polynomial is zero on all of its coset");
    fr_inv<FR>(s, zg);
  });
  if (n == 0) return;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->pstage, device_ptrs, on, n);
    const uint32_t* src = g.in(in, n);
    uint32_t* dst = g.out_over(out, src);
    poly_vec_enqueue(d, dst, src, nullptr, nullptr, n, kPolyScale, s, flags, on);
    g.back(out, dst, n);
  });
}

}  // namespace

extern "C" {

RustError mi355_msm_domain_batch_inverse(mi355_msm_domain* d, void* out, const void* in, size_t n, const void* coeff, unsigned flags) {
  return guarded_dev([&] { poly_inverse(d, out, in, n, coeff, flags, false, nullptr); });
}

RustError mi355_msm_domain_batch_inverse_device(mi355_msm_domain* d, void* d_out, const void* d_in, size_t n, const void* coeff, unsigned flags, void* stream) {
  return guarded_dev([&] { poly_inverse(d, d_out, d_in, n, coeff, flags, true, (hipStream_t)stream); });
}

RustError mi355_msm_domain_vec_op(mi355_msm_domain* d, void* out, const void* a, const void* b, const void* c, size_t n, unsigned op, unsigned flags) {
  return guarded_dev([&] { poly_vec(d, out, a, b, c, n, op, flags, false, nullptr); });
}

RustError mi355_msm_domain_vec_op_device(mi355_msm_domain* d, void* d_out, const void* d_a, const void* d_b, const void* d_c, size_t n, unsigned op,
                                         unsigned flags, void* stream) {
  return guarded_dev([&] { poly_vec(d, d_out, d_a, d_b, d_c, n, op, flags, true, (hipStream_t)stream); });
}

RustError mi355_msm_domain_evaluate(mi355_msm_domain* d, void* out32, const void* coeffs, size_t n, const void* z, unsigned flags) {
  return guarded_dev([&] { poly_evaluate(d, out32, coeffs, n, z, flags, false, nullptr); });
}

RustError mi355_msm_domain_evaluate_device(mi355_msm_domain* d, void* out32, const void* d_coeffs, size_t n, const void* z, unsigned flags, void* stream) {
  return guarded_dev([&] { poly_evaluate(d, out32, d_coeffs, n, z, flags, true, (hipStream_t)stream); });
}

RustError mi355_msm_domain_divide_by_linear(mi355_msm_domain* d, void* q_out, void* rem32, const void* coeffs, size_t n, const void* z, unsigned flags) {
  return guarded_dev([&] { poly_divide(d, q_out, rem32, coeffs, n, z, flags, false, nullptr); });
}

RustError mi355_msm_domain_divide_by_linear_device(mi355_msm_domain* d, void* d_q_out, void* rem32, const void* d_coeffs, size_t n, const void* z,
                                                   unsigned flags, void* stream) {
  return guarded_dev([&] { poly_divide(d, d_q_out, rem32, d_coeffs, n, z, flags, true, (hipStream_t)stream); });
}

RustError mi355_msm_domain_lagrange(mi355_msm_domain* d, void* out, const void* tau, unsigned flags) {
  return guarded_dev([&] { poly_lagrange(d, out, tau, flags, false, nullptr); });
}

RustError mi355_msm_domain_lagrange_device(mi355_msm_domain* d, void* d_out, const void* tau, unsigned flags, void* stream) {
  return guarded_dev([&] { poly_lagrange(d, d_out, tau, flags, true, (hipStream_t)stream); });
}

RustError mi355_msm_domain_vanishing(mi355_msm_domain* d, void* out32, const void* tau, unsigned flags) {
  return guarded([&] { poly_vanishing_host(d, out32, tau, flags); });
}

RustError mi355_msm_domain_divide_by_vanishing_on_coset(mi355_msm_domain* d, void* out, const void* in, size_t n, const void* offset, unsigned flags) {
  return guarded_dev([&] { poly_divide_vanishing(d, out, in, n, offset, flags, false, nullptr); });
}

RustError mi355_msm_domain_divide_by_vanishing_on_coset_device(mi355_msm_domain* d, void* d_out, const void* d_in, size_t n, const void* offset,
                                                               unsigned flags, void* stream) {
  return guarded_dev([&] { poly_divide_vanishing(d, d_out, d_in, n, offset, flags, true, (hipStream_t)stream); });
}

}  // extern "C"
