// msm_quot.hpp -- the rows of the Plonk quotient and linear combinations on the domain handle (included by msm_engine.hip after
// msm_scan.hpp): the C ABI mi355_msm_domain_{plonk_quotient, linear_combination} of include/mi355_msm.h over the kernels of
// quotient.hpp.
//
// Every call judges its arguments first (the handle last, so the other errors read the same with and without one; what depends on
// the size or the field of the domain can only be judged with one), derives its constants in host arithmetic and enqueues separate
// launches on one stream.  The values x_i - 1, their inverses and the tile products of that inversion live in `quot` (allocated on the
// first such call, kept by the handle: query "quotient_work_bytes"); host-pointer calls stage whole vectors through `qstage` (with
// the FrStage of fr_stage.hpp).  The other buffers of the handle are not touched.
#pragma once

#include "launch_quot.hpp"

namespace {

template <class FR>
struct QuotRun : PolyRun<FR> {
  void xm1(const QuotXm1& p) { HIP_OK(LaunchQuot<FR>::xm1(p, this->st)); }
  void rows(const QuotRows& p) { HIP_OK(LaunchQuot<FR>::rows(p, this->st)); }
};

bool quot_all_zero(const void* bytes32) {
  const uint8_t* b = (const uint8_t*)bytes32;
  uint8_t o = 0;
  for (int i = 0; i < 32; i++) o |= b[i];
  return o == 0;
}

// ---- the rows of the quotient -------------------------------------------------------------------------------------------------------

struct QuotArgs {
  void* out;
  const void *wires, *sigmas, *selectors, *z, *pi;
  size_t m, stride, n;
  const void *ks, *alpha, *beta, *gamma, *offset;
  unsigned flags;
};

// returns log2(n)
uint32_t quot_check(mi355_msm_domain* d, const QuotArgs& a, bool device_ptrs) {
  if (a.flags & ~kQuotNormal) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements)", a.flags);
  if (a.selectors) {
    if (a.m != QUOT_GATE_WIRES) bad_arg("%zu columns: the gate of the 13 selectors takes %u wires", a.m, QUOT_GATE_WIRES);
  } else if (a.m < 1 || a.m > QUOT_MAX_COLUMNS) {
    bad_arg("%zu columns: the quotient takes 1 .. %u without selectors", a.m, QUOT_MAX_COLUMNS);
  }
  if (a.n == 0 || (a.n & (a.n - 1))) bad_arg("a constraint domain of %zu rows: not a power of two", a.n);
  if (a.n > ((size_t)1 << (NTT_MAX_LOG - 1))) bad_arg("a constraint domain of %zu rows leaves no domain a ratio of 2, 4, 8 or 16", a.n);
  if (a.stride == 0) bad_arg("a column stride of 0 elements is below the rows of every domain");
  if (a.stride > kPolyMaxN) bad_arg("a column stride of %zu elements exceeds 2^30", a.stride);
  if (!a.out || !a.wires || !a.sigmas || !a.z || !a.ks || !a.alpha || !a.beta || !a.gamma) bad_arg("null input or output pointer");
  poly_check_aligned(device_ptrs, {a.out, a.wires, a.sigmas, a.selectors, a.z, a.pi});
  for (const void* in : {a.wires, a.sigmas, a.selectors, a.z, a.pi})
    if (in == a.out) bad_arg("the output overlaps an input (z is read `ratio` rows ahead: the rows are not computed in place)");
  if (a.offset && quot_all_zero(a.offset)) bad_arg("the coset offset is zero");
  poly_check_handle(d);
  // (what depends on the size of the domain can only be judged with one)
  const size_t M = (size_t)1 << d->k;
  uint32_t log_n = 0;
  while (((size_t)1 << log_n) < a.n) log_n++;
  const size_t ratio = a.n <= M ? M / a.n : 0;
  if (ratio != 2 && ratio != 4 && ratio != 8 && ratio != 16)
    bad_arg("a domain of %zu points over a constraint domain of %zu rows: the ratio must be 2, 4, 8 or 16", M, a.n);
  if (ratio >= M) bad_arg("a ratio of %zu needs a domain of more than %zu points", ratio, M);
  if (a.stride < M) bad_arg("a column stride of %zu elements is below the %zu rows of the domain", a.stride, M);
  const size_t span = (a.m - 1) * a.stride + M, sel_span = (QUOT_SELECTORS - 1) * a.stride + M;
  if (poly_overlap(a.out, M, a.wires, span) || poly_overlap(a.out, M, a.sigmas, span) || poly_overlap(a.out, M, a.selectors, sel_span) ||
      poly_overlap(a.out, M, a.z, M) || poly_overlap(a.out, M, a.pi, M))
    bad_arg("the output overlaps an input (z is read `ratio` rows ahead: the rows are not computed in place)");
  return log_n;
}

void quot_call(mi355_msm_domain* d, const QuotArgs& a, bool device_ptrs, hipStream_t st) {
  const uint32_t log_n = quot_check(d, a, device_ptrs);
  const bool normal = (a.flags & kQuotNormal) != 0;
  const size_t M = (size_t)1 << d->k, span = (a.m - 1) * a.stride + M, sel_span = (QUOT_SELECTORS - 1) * a.stride + M;
  const NttLayout at(d->k);
  QuotRows p{};
  Fr a2n;
  p.stride = a.stride;
  p.k = d->k;
  p.m = (uint32_t)a.m;
  p.ratio = (uint32_t)(M >> log_n);
  Fr* t = d->tables.as<Fr>();
  p.w = NttTable{t + at.wlo, t + at.whi};
  with_fr(d->curve, [&]<class FR>() {
    Fr zero, alpha;
    fr_zero(zero);
    quot_form<FR>(p.cin, p.cout, normal);
    if (a.offset) poly_scalar<FR>(p.g, a.offset, normal); else fr_set<FR>(p.g, FR::GENERATOR);
    if (fr_same(p.g, zero)) bad_arg("the coset offset is zero");
    poly_scalar<FR>(alpha, a.alpha, normal);
    poly_scalar<FR>(p.beta, a.beta, normal);
    poly_scalar<FR>(p.gamma, a.gamma, normal);
    for (size_t j = 0; j < a.m; j++) poly_scalar<FR>(p.bks[j], (const uint8_t*)a.ks + 32 * j, normal);
    if (!quot_constants<FR>(p, a2n, alpha, log_n))
      bad_arg("the offset's %zu-th power is a root of unity of order %u: the vanishing polynomial of the constraint domain is zero on rows of the coset", a.n,
              p.ratio);
  });
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->qstage, device_ptrs, on, 2 * span + (a.selectors ? sel_span : 0) + (a.pi ? 3 : 2) * M);
    p.wires = g.in(a.wires, span);
    p.sigmas = g.in(a.sigmas, span);
    p.selectors = a.selectors ? g.in(a.selectors, sel_span) : nullptr;
    p.z = g.in(a.z, M);
    p.pi = a.pi ? g.in(a.pi, M) : nullptr;
    p.dst = g.out(a.out, M);
    d->quot.reserve((size_t)quot_work_elems(M, d->poly_tile_log) * sizeof(Fr));
    with_fr(d->curve, [&]<class FR>() {
      QuotRun<FR> run{{on}};
      quot_chain<FR>(run, p, a2n, d->poly_tile_log, d->quot.as<Fr>());
    });
    g.back(a.out, p.dst, M);
  });
}

// ---- the linear combination ---------------------------------------------------------------------------------------------------------

// returns max(lens)
size_t lincomb_check(mi355_msm_domain* d, const void* out, const void* const* cols, const size_t* lens, const void* coeffs, size_t m, unsigned flags,
                     bool device_ptrs) {
  if (flags & ~kQuotNormal) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements)", flags);
  if (m < 1 || m > LINCOMB_MAX_COLUMNS) bad_arg("%zu columns: a linear combination takes 1 .. %u", m, LINCOMB_MAX_COLUMNS);
  if (!cols || !lens || !coeffs) bad_arg("null input or output pointer");
  size_t n = 0;
  for (size_t j = 0; j < m; j++) {
    if (lens[j] > kPolyMaxN) bad_arg("column %zu: %zu elements exceed 2^30", j, lens[j]);
    if (lens[j] && !cols[j]) bad_arg("null input or output pointer");
    if (lens[j] > n) n = lens[j];
  }
  if (n && !out) bad_arg("null input or output pointer");
  for (size_t j = 0; j < m; j++) {
    if (out != cols[j] && poly_overlap(out, n, cols[j], lens[j])) bad_arg("the output overlaps column %zu in part (out == a column is allowed)", j);
    poly_check_aligned(device_ptrs, {cols[j]});
  }
  poly_check_aligned(device_ptrs, {out});
  poly_check_handle(d);
  return n;
}

void lincomb_call(mi355_msm_domain* d, void* out, const void* const* cols, const size_t* lens, const void* coeffs, size_t m, unsigned flags,
                  bool device_ptrs, hipStream_t st) {
  const size_t n = lincomb_check(d, out, cols, lens, coeffs, m, flags, device_ptrs);
  if (n == 0) return;
  const bool normal = (flags & kQuotNormal) != 0;
  LinComb p{};
  p.n = (uint32_t)n;
  p.m = (uint32_t)m;
  size_t total = 0;
  with_fr(d->curve, [&]<class FR>() {
    quot_form<FR>(p.cin, p.cout, normal);
    for (size_t j = 0; j < m; j++) {
      poly_scalar<FR>(p.coeffs[j], (const uint8_t*)coeffs + 32 * j, normal);
      p.lens[j] = (uint32_t)lens[j];
      total += lens[j];
    }
  });
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->qstage, device_ptrs, on, total + n);
    for (size_t j = 0; j < m; j++) p.cols[j] = g.in(cols[j], lens[j]);
    p.dst = g.out(out, n);
    with_fr(d->curve, [&]<class FR>() { HIP_OK(LaunchQuot<FR>::lincomb(p, on)); });
    g.back(out, p.dst, n);
  });
}

}  // namespace

extern "C" {

RustError mi355_msm_domain_plonk_quotient(mi355_msm_domain* d, void* out, const void* wires, const void* sigmas, const void* selectors, const void* z,
                                          const void* pi, size_t m, size_t stride, size_t n, const void* ks, const void* alpha, const void* beta,
                                          const void* gamma, const void* offset, unsigned flags) {
  return guarded_dev([&] { quot_call(d, QuotArgs{out, wires, sigmas, selectors, z, pi, m, stride, n, ks, alpha, beta, gamma, offset, flags}, false, nullptr); });
}

RustError mi355_msm_domain_plonk_quotient_device(mi355_msm_domain* d, void* d_out, const void* d_wires, const void* d_sigmas, const void* d_selectors,
                                                 const void* d_z, const void* d_pi, size_t m, size_t stride, size_t n, const void* ks, const void* alpha,
                                                 const void* beta, const void* gamma, const void* offset, unsigned flags, void* stream) {
  return guarded_dev([&] {
    quot_call(d, QuotArgs{d_out, d_wires, d_sigmas, d_selectors, d_z, d_pi, m, stride, n, ks, alpha, beta, gamma, offset, flags}, true, (hipStream_t)stream);
  });
}

RustError mi355_msm_domain_linear_combination(mi355_msm_domain* d, void* out, const void* const* cols, const size_t* lens, const void* coeffs, size_t m,
                                              unsigned flags) {
  return guarded_dev([&] { lincomb_call(d, out, cols, lens, coeffs, m, flags, false, nullptr); });
}

RustError mi355_msm_domain_linear_combination_device(mi355_msm_domain* d, void* d_out, const void* const* d_cols, const size_t* lens, const void* coeffs,
                                                     size_t m, unsigned flags, void* stream) {
  return guarded_dev([&] { lincomb_call(d, d_out, d_cols, lens, coeffs, m, flags, true, (hipStream_t)stream); });
}

}  // extern "C"
