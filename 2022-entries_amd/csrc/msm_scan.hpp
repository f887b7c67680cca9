// msm_scan.hpp -- prefix scans and the permutation product on the domain handle (included by msm_engine.hip after msm_poly.hpp): the
// C ABI mi355_msm_domain_{scan, permutation_product} of include/mi355_msm.h over the kernels of scan.hpp.
//
// Every call judges its arguments first (the handle last, so the other errors read the same with and without one) and enqueues
// separate launches on one stream.  The totals and carries of the levels, and the numerators and denominators of the permutation
// product with the work memory of their batch inversion, live in `scan` (allocated on the first such call, kept by the handle: query
// "scan_work_bytes"); host-pointer calls stage whole vectors through `sstage` (with the FrStage of fr_stage.hpp).  `work`, `stage`,
// `poly` and `pstage` are not touched.
#pragma once

#include "launch_scan.hpp"

namespace {

template <class FR>
struct ScanRun {
  hipStream_t st;
  template <unsigned OP>
  void up(const ScanUp& p) { HIP_OK(LaunchScan<FR>::up(OP, p, st)); }
  template <unsigned OP>
  void down(const ScanDown& p) { HIP_OK(LaunchScan<FR>::down(OP, p, st)); }
};

void scan_identity_out(mi355_msm_domain* d, void* total32, unsigned op, unsigned flags) {
  with_fr(d->curve, [&]<class FR>() {
    Fr x;
    if (op == kScanProduct) fr_set<FR>(x, FR::ONE); else fr_zero(x);
    poly_scalar_out<FR>(total32, x, (flags & kScanNormal) != 0);
  });
}

// ---- the scans --------------------------------------------------------------------------------------------------------------------

void scan_check(mi355_msm_domain* d, const void* out, const void* in, size_t n, unsigned op, unsigned flags, bool device_ptrs) {
  if (flags & ~(kScanNormal | kScanInclusive)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: inclusive scan)", flags);
  if (n > kPolyMaxN) bad_arg("%zu elements exceed 2^30", n);
  if (op > kScanSum) bad_arg("unknown scan operation %u (0 product, 1 sum)", op);
  if (n && (!out || !in)) bad_arg("null input or output pointer");
  poly_check_alias(out, in, n, "in");
  poly_check_aligned(device_ptrs, {out, in});
  poly_check_handle(d);
}

const Fr* scan_enqueue(mi355_msm_domain* d, uint32_t* out, const uint32_t* in, const uint32_t* mul, size_t n, unsigned op, unsigned flags, Fr* work,
                       hipStream_t st) {
  const bool normal = (flags & kScanNormal) != 0, inclusive = (flags & kScanInclusive) != 0;
  const Fr* res = nullptr;
  with_fr(d->curve, [&]<class FR>() {
    ScanRun<FR> run{st};
    res = op == kScanProduct ? scan_chain<FR, kScanProduct>(run, out, in, mul, n, normal, inclusive, d->poly_tile_log, work)
                             : scan_chain<FR, kScanSum>(run, out, in, mul, n, normal, inclusive, d->poly_tile_log, work);
  });
  return res;
}

void scan_call(mi355_msm_domain* d, void* out, void* total32, const void* in, size_t n, unsigned op, unsigned flags, bool device_ptrs, hipStream_t st) {
  scan_check(d, out, in, n, op, flags, device_ptrs);
  if (n == 0) {
    if (total32) scan_identity_out(d, total32, op, flags);
    return;
  }
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const Fr* res = nullptr;
  poly_timed(d, on, [&] {
    FrStage g(d->sstage, device_ptrs, on, n);
    const uint32_t* src = g.in(in, n);
    uint32_t* dst = g.out_over(out, src);
    d->scan.reserve((size_t)scan_work_elems(n, d->poly_tile_log) * sizeof(Fr));
    res = scan_enqueue(d, dst, src, nullptr, n, op, flags, d->scan.as<Fr>(), on);
    g.back(out, dst, n);
  });
  if (total32) poly_fetch(d, total32, res, flags & kScanNormal);
}

// ---- the permutation product ------------------------------------------------------------------------------------------------------

void perm_check(mi355_msm_domain* d, const void* out, const void* wires, const void* sigmas, size_t m, size_t stride, const void* ks, const void* beta,
                const void* gamma, unsigned flags, bool device_ptrs) {
  if (flags & ~kScanNormal) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements)", flags);
  if (m < 1 || m > SCAN_MAX_COLUMNS) bad_arg("%zu columns: the permutation product takes 1 .. %u", m, SCAN_MAX_COLUMNS);
  if (stride == 0) bad_arg("a column stride of 0 elements is below the rows of every domain");
  if (stride > kPolyMaxN) bad_arg("a column stride of %zu elements exceeds 2^30", stride);
  if (!out || !wires || !sigmas || !ks || !beta || !gamma) bad_arg("null input or output pointer");
  poly_check_aligned(device_ptrs, {out, wires, sigmas});
  poly_check_handle(d);
  // (what depends on the size of the domain can only be judged with one)
  const size_t n = (size_t)1 << d->k, span = (m - 1) * stride + n;
  if (stride < n) bad_arg("a column stride of %zu elements is below the %zu rows of the domain", stride, n);
  if (poly_overlap(out, n, wires, span) || poly_overlap(out, n, sigmas, span)) bad_arg("the output overlaps the wires or the sigmas");
}

void perm_call(mi355_msm_domain* d, void* out, void* total32, const void* wires, const void* sigmas, size_t m, size_t stride, const void* ks,
               const void* beta, const void* gamma, unsigned flags, bool device_ptrs, hipStream_t st) {
  perm_check(d, out, wires, sigmas, m, stride, ks, beta, gamma, flags, device_ptrs);
  const bool normal = (flags & kScanNormal) != 0;
  const size_t n = (size_t)1 << d->k, span = (m - 1) * stride + n;
  const NttLayout at(d->k);
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const Fr* res = nullptr;
  poly_timed(d, on, [&] {
    FrStage g(d->sstage, device_ptrs, on, 2 * span + n);
    ScanPerm p{};
    p.wires = g.in(wires, span);
    p.sigmas = g.in(sigmas, span);
    uint32_t* dst = g.out(out, n);
    // work memory: the scan's levels, the inversion's tile products, the numerators, the denominators
    const size_t scan_elems = (size_t)scan_work_elems(n, d->poly_tile_log), inv_elems = (size_t)poly_work_elems(n, d->poly_tile_log);
    d->scan.reserve((scan_elems + inv_elems) * sizeof(Fr) + 2 * n * 32);
    Fr* work = d->scan.as<Fr>();
    p.num = (uint32_t*)(work + scan_elems + inv_elems);
    p.den = p.num + n * 8;
    p.stride = stride;
    p.k = d->k;
    p.m = (uint32_t)m;
    p.normal = normal ? 1u : 0u;
    Fr* t = d->tables.as<Fr>();
    p.w = NttTable{t + at.wlo, t + at.whi};
    with_fr(d->curve, [&]<class FR>() {
      poly_scalar<FR>(p.beta, beta, normal);
      poly_scalar<FR>(p.gamma, gamma, normal);
      for (size_t i = 0; i < m; i++) poly_scalar<FR>(p.ks[i], (const uint8_t*)ks + 32 * i, normal);
      HIP_OK(LaunchScan<FR>::perm(p, on));
      Fr one;
      fr_set<FR>(one, FR::ONE);
      PolyRun<FR> inv{on};
      poly_chain_inverse<FR>(inv, p.den, p.den, n, normal, d->poly_tile_log, one, work + scan_elems);
    });
    res = scan_enqueue(d, dst, p.num, p.den, n, kScanProduct, flags, work, on);
    g.back(out, dst, n);
  });
  if (total32) poly_fetch(d, total32, res, flags);
}

}  // namespace

extern "C" {

RustError mi355_msm_domain_scan(mi355_msm_domain* d, void* out, void* total32, const void* in, size_t n, unsigned op, unsigned flags) {
  return guarded_dev([&] { scan_call(d, out, total32, in, n, op, flags, false, nullptr); });
}

RustError mi355_msm_domain_scan_device(mi355_msm_domain* d, void* d_out, void* total32, const void* d_in, size_t n, unsigned op, unsigned flags,
                                       void* stream) {
  return guarded_dev([&] { scan_call(d, d_out, total32, d_in, n, op, flags, true, (hipStream_t)stream); });
}

RustError mi355_msm_domain_permutation_product(mi355_msm_domain* d, void* out, void* total32, const void* wires, const void* sigmas, size_t m,
                                               size_t stride, const void* ks, const void* beta, const void* gamma, unsigned flags) {
  return guarded_dev([&] { perm_call(d, out, total32, wires, sigmas, m, stride, ks, beta, gamma, flags, false, nullptr); });
}

RustError mi355_msm_domain_permutation_product_device(mi355_msm_domain* d, void* d_out, void* total32, const void* d_wires, const void* d_sigmas,
                                                      size_t m, size_t stride, const void* ks, const void* beta, const void* gamma, unsigned flags,
                                                      void* stream) {
  return guarded_dev([&] { perm_call(d, d_out, total32, d_wires, d_sigmas, m, stride, ks, beta, gamma, flags, true, (hipStream_t)stream); });
}

}  // extern "C"
