// msm_mle.hpp -- dense multilinear extensions and sumcheck prover rounds on the domain handle (included by msm_engine.hip after
// msm_sparse.hpp): the C ABI mi355_msm_domain_{mle_fix, mle_eq, sumcheck_round} of include/mi355_msm.h over the kernels of mle.hpp.
//
// Reference: ARK poly/src/evaluations/multivariate/multilinear/dense.rs:26-134 (fix_variables, evaluate) and the prover of
// ark-linear-sumcheck's ListOfProductsOfPolynomials.  The handle lends its field, its stream for host-pointer calls and its host
// arithmetic; the vector lengths have nothing to do with the domain's size.  One call with a flag bit for device pointers, like
// mi355_msm_sparse_apply, and no twin whose name ends in _device.  Every call judges its arguments first (the handle last), derives its
// constants in host arithmetic (1 - r, the half tables of eq, the coefficients) and enqueues separate launches on one stream.  The
// passes of fix_variables, the half tables and the partial rows of a round live in `mle` (allocated on the first such call, kept by
// the handle: query "mle_work_bytes"); host-pointer calls stage whole vectors through `mstage` (with the FrStage of fr_stage.hpp).
#pragma once

#include "launch_mle.hpp"

namespace {

template <class FR>
struct MleRun {
  hipStream_t st;
  void fix(const MleFix& p) { HIP_OK(LaunchMle<FR>::fix(p, st)); }
  void eq(const MleEq& p) { HIP_OK(LaunchMle<FR>::eq(p, st)); }
  template <int D>
  void round(const MleRound& p) { HIP_OK(LaunchMle<FR>::round(p, D, st)); }
  void sum(const MleSum& p) { HIP_OK(LaunchMle<FR>::sum(p, st)); }
};

void mle_check_flags(unsigned flags) {
  if (flags & ~(kMleNormal | kMleDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
}

void mle_fix(mi355_msm_domain* d, void* out, const void* in, unsigned num_vars, const void* point, unsigned k, unsigned flags, hipStream_t st) {
  mle_check_flags(flags);
  const bool device_ptrs = (flags & kMleDevice) != 0, normal = (flags & kMleNormal) != 0;
  if (num_vars > MLE_MAX_VARS) bad_arg("%u variables exceed %u", num_vars, MLE_MAX_VARS);
  if (k > num_vars) bad_arg("%u variables to fix exceed the %u of the table", k, num_vars);
  if (!out || !in || (k && !point)) bad_arg("null input, output or point pointer");
  poly_check_aligned(device_ptrs, {out, in});
  poly_check_stream(device_ptrs, st);
  const size_t n_in = (size_t)1 << num_vars, n_out = (size_t)1 << (num_vars - k);
  if (poly_overlap(out, n_out, in, n_in)) bad_arg("the output overlaps the input (a lane's pair is another block's output: the fold is not done in place)");
  poly_check_handle(d);
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->mstage, device_ptrs, on, n_in + n_out);
    const uint32_t* src = g.in(in, n_in);
    uint32_t* dst = g.out(out, n_out);
    d->mle.reserve((size_t)mle_fix_work_elems(num_vars, k, d->poly_tile_log) * sizeof(Fr) + 64);
    with_fr(d->curve, [&]<class FR>() {
      Fr pt[MLE_MAX_VARS];
      for (unsigned i = 0; i < k; i++) poly_scalar<FR>(pt[i], (const uint8_t*)point + 32 * i, normal);
      MleRun<FR> run{on};
      mle_chain_fix<FR>(run, dst, src, num_vars, pt, k, normal, d->poly_tile_log, d->mle.as<Fr>());
    });
    g.back(out, dst, n_out);
  });
}

void mle_eq(mi355_msm_domain* d, void* out, const void* point, unsigned k, unsigned flags, hipStream_t st) {
  mle_check_flags(flags);
  const bool device_ptrs = (flags & kMleDevice) != 0, normal = (flags & kMleNormal) != 0;
  if (k > MLE_MAX_VARS) bad_arg("%u variables exceed %u", k, MLE_MAX_VARS);
  if (!out || (k && !point)) bad_arg("null output or point pointer");
  poly_check_aligned(device_ptrs, {out});
  poly_check_stream(device_ptrs, st);
  poly_check_handle(d);
  const size_t n = (size_t)1 << k;
  const uint32_t lo_log = (k + 1) / 2, hi_log = k - lo_log;
  std::vector<Fr> lo, hi;   // (alive until the stream is idle)
  with_fr(d->curve, [&]<class FR>() {
    Fr pt[MLE_MAX_VARS], one, cout;
    for (unsigned i = 0; i < k; i++) poly_scalar<FR>(pt[i], (const uint8_t*)point + 32 * i, normal);
    fr_set<FR>(one, FR::ONE);
    fr_const<FR>(cout, normal ? 3 : 2);
    mle_eq_half<FR>(lo, pt, lo_log, one);
    mle_eq_half<FR>(hi, pt + lo_log, hi_log, cout);
  });
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(d->mstage, device_ptrs, on, n);
    uint32_t* dst = g.out(out, n);
    d->mle.reserve((lo.size() + hi.size()) * sizeof(Fr) + 64);
    Fr* dlo = d->mle.as<Fr>();
    Fr* dhi = dlo + lo.size();
    HIP_OK(hipMemcpyAsync(dlo, lo.data(), lo.size() * sizeof(Fr), hipMemcpyHostToDevice, on));
    HIP_OK(hipMemcpyAsync(dhi, hi.data(), hi.size() * sizeof(Fr), hipMemcpyHostToDevice, on));
    with_fr(d->curve, [&]<class FR>() {
      MleRun<FR> run{on};
      mle_chain_eq<FR>(run, dst, dlo, dhi, k);
    });
    g.back(out, dst, n);
  });
}

void mle_round(mi355_msm_domain* d, void* evals_out, const void* const* tables, size_t m, unsigned num_vars, const mi355_msm_sumcheck_term* terms,
               size_t n_terms, const void* r_prev, void* const* folded, unsigned flags, hipStream_t st) {
  mle_check_flags(flags);
  const bool device_ptrs = (flags & kMleDevice) != 0, normal = (flags & kMleNormal) != 0, fused = r_prev != nullptr;
  if (m < 1 || m > MLE_MAX_TABLES) bad_arg("%zu tables: a round takes 1 .. %u", m, MLE_MAX_TABLES);
  if (num_vars < 1 || num_vars > MLE_MAX_VARS) bad_arg("%u variables: a round takes 1 .. %u", num_vars, MLE_MAX_VARS);
  if (n_terms < 1 || n_terms > MLE_MAX_TERMS) bad_arg("%zu terms: a round takes 1 .. %u", n_terms, MLE_MAX_TERMS);
  if (fused && num_vars < 2) bad_arg("a table of one variable cannot be folded before the round (r_prev with num_vars == 1)");
  if (!evals_out || !tables || !terms || (fused && !folded)) bad_arg("null pointer");
  for (size_t i = 0; i < m; i++)
    if (!tables[i] || (fused && !folded[i])) bad_arg("null table pointer");
  for (size_t i = 0; i < m; i++) poly_check_aligned(device_ptrs, {tables[i], fused ? folded[i] : nullptr});
  poly_check_stream(device_ptrs, st);
  const size_t n_in = (size_t)1 << num_vars, n_half = n_in / 2;
  if (fused)
    for (size_t i = 0; i < m; i++) {
      for (size_t j = 0; j < m; j++) {
        if (poly_overlap(folded[i], n_half, tables[j], n_in)) bad_arg("folded table %zu overlaps table %zu", i, j);
        if (i != j && poly_overlap(folded[i], n_half, folded[j], n_half)) bad_arg("folded table %zu overlaps folded table %zu", i, j);
      }
    }
  uint32_t D = 0;
  for (size_t j = 0; j < n_terms; j++) {
    const uint32_t nf = terms[j].n_factors;
    if (nf < 1 || nf > MLE_MAX_FACTORS) bad_arg("term %zu has %u factors: a term takes 1 .. %u", j, nf, MLE_MAX_FACTORS);
    for (uint32_t q = 0; q < nf; q++)
      if (terms[j].factors[q] >= m) bad_arg("term %zu: factor index %u is not below the %zu tables", j, terms[j].factors[q], m);
    if (nf > D) D = nf;
  }
  poly_check_handle(d);
  const size_t n_round = fused ? n_half : n_in;   // elements of a table of the round
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const Fr* res = nullptr;
  poly_timed(d, on, [&] {
    FrStage g(d->mstage, device_ptrs, on, m * n_in + (fused ? m * n_half : 0));
    MleRound p{};
    p.npts = n_round / 2;
    p.m = (uint32_t)m;
    p.n_terms = (uint32_t)n_terms;
    p.tile_log = d->poly_tile_log;
    p.fused = fused ? 1u : 0u;
    for (size_t i = 0; i < m; i++) {
      const uint32_t* src = g.in(tables[i], n_in);
      if (fused) {
        p.src[i] = src;
        p.folded[i] = g.out(folded[i], n_half);
        p.tab[i] = p.folded[i];
      } else {
        p.tab[i] = src;
      }
    }
    d->mle_levels = mle_round_levels(p.npts, p.tile_log);
    d->mle.reserve((size_t)mle_round_work_elems(p.npts, p.tile_log) * sizeof(Fr) + 64);
    with_fr(d->curve, [&]<class FR>() {
      fr_const<FR>(p.cin, normal ? 1 : 0);
      fr_const<FR>(p.cout, normal ? 3 : 2);
      for (size_t j = 0; j < n_terms; j++) {
        poly_scalar<FR>(p.term[j].c, terms[j].coeff, normal);
        p.term[j].nf = terms[j].n_factors;
        for (uint32_t q = 0; q < p.term[j].nf; q++) p.term[j].f[q] = terms[j].factors[q];
      }
      if (fused) {
        Fr r;
        poly_scalar<FR>(r, r_prev, normal);
        mle_one_minus<FR>(p.fa, r);
        mle_mul_canon<FR>(p.fa, p.fa, p.cin);
        mle_mul_canon<FR>(p.fb, r, p.cin);
      }
      MleRun<FR> run{on};
      res = mle_chain_round<FR>(run, p, D, d->mle.as<Fr>());
    });
    if (fused)
      for (size_t i = 0; i < m; i++) g.back(folded[i], p.folded[i], n_half);
  });
  Fr row[MLE_EVALS];
  HIP_OK(hipMemcpy(row, res, (D + 1) * sizeof(Fr), hipMemcpyDeviceToHost));
  with_fr(d->curve, [&]<class FR>() {
    for (uint32_t t = 0; t <= D; t++) poly_scalar_out<FR>((uint8_t*)evals_out + 32 * t, row[t], normal);
  });
}

}  // namespace

extern "C" {

RustError mi355_msm_domain_mle_fix(mi355_msm_domain* d, void* out, const void* in, unsigned num_vars, const void* point, unsigned k, unsigned flags,
                                   void* stream) {
  return guarded_dev([&] { mle_fix(d, out, in, num_vars, point, k, flags, (hipStream_t)stream); });
}

RustError mi355_msm_domain_mle_eq(mi355_msm_domain* d, void* out, const void* point, unsigned k, unsigned flags, void* stream) {
  return guarded_dev([&] { mle_eq(d, out, point, k, flags, (hipStream_t)stream); });
}

RustError mi355_msm_domain_sumcheck_round(mi355_msm_domain* d, void* evals_out, const void* const* tables, size_t m, unsigned num_vars,
                                          const mi355_msm_sumcheck_term* terms, size_t n_terms, const void* r_prev, void* const* folded,
                                          unsigned flags, void* stream) {
  return guarded_dev([&] { mle_round(d, evals_out, tables, m, num_vars, terms, n_terms, r_prev, folded, flags, (hipStream_t)stream); });
}

}  // extern "C"
