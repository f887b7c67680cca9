// msm_ntt.hpp -- radix-2 evaluation domains over the scalar fields (included by msm_engine.hip): the C ABI mi355_msm_domain_* of
// include/mi355_msm.h over the kernels of ntt.hpp.
//
// Reference: ARK poly/src/domain/radix2/mod.rs (Radix2EvaluationDomain), poly/src/domain/mod.rs:99-170 (fft, ifft, coset_fft,
// coset_ifft), :233 (mul_polynomials_in_evaluation_domain).  A handle is one domain size on one device: the two-level twiddle
// tables of the root and of its inverse, the butterfly tables, the tables of the most recent coset offset (rebuilt when a call
// brings another) -- one DevBuf of 3 (2^h + 2^(k-h)) + 1024 elements of 36 bytes, 3.6 MB at k = 28 -- plus one work vector per
// vector in flight and, for host-pointer calls, one staged vector.  A handle serves one call at a time.
#pragma once

#include "fr_stage.hpp"
#include "launch_ntt.hpp"
#include "launch_poly.hpp"
#include "mle.hpp"      // (the limits of a sumcheck round, for the queries)

struct mi355_msm_domain {
  int curve = 0;
  int device = -1;
  uint32_t k = 0, pass_log = NTT_DEFAULT_PASS_LOG;
  hipStream_t own_stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  DevBuf tables, work, stage;
  DevBuf poly, pstage;    // msm_poly.hpp: the partial vectors of the scans; the staged vectors of its host-pointer calls
  uint32_t poly_tile_log = POLY_DEFAULT_TILE_LOG;
  DevBuf scan, sstage;    // msm_scan.hpp: the levels of the scans and the rows of the permutation product; the staged vectors of its host-pointer calls
  DevBuf quot, qstage;    // msm_quot.hpp: x - 1 per row, its inverses and their tile products; the staged vectors of its host-pointer calls
  DevBuf mle, mstage;     // msm_mle.hpp: the passes of fix_variables, the half tables of eq, the partial rows of a round; the staged vectors of its host-pointer calls
  DevBuf logup, lstage;   // msm_lookup.hpp: the denominators, the terms and the levels of the logUp sum; the staged vectors of its host-pointer calls
  uint32_t mle_levels = 0;   // launches of the most recent sumcheck round: the round and its further sums
  Fr size_inv{};
  Fr g_have{};            // the (inverted, for the inverse kinds) offset the offset tables hold
  bool g_valid = false;
  uint64_t last_us = 0, last_device_us = 0;
};

namespace {

constexpr unsigned kDomainKindMax = 3;

size_t ntt_lo_count(uint32_t k) { return (size_t)1 << ntt_lo_log(k); }
size_t ntt_hi_count(uint32_t k) { return (size_t)1 << (k - ntt_lo_log(k)); }
constexpr size_t kNttSmallCount = (size_t)1 << (NTT_SMALL_LOG - 1);

// the tables of a handle inside its one buffer, in elements
struct NttLayout {
  size_t wlo, whi, ilo, ihi, small, ismall, glo, ghi, total;
  explicit NttLayout(uint32_t k) {
    const size_t lo = ntt_lo_count(k), hi = ntt_hi_count(k);
    wlo = 0;
    whi = wlo + lo;
    ilo = whi + hi;
    ihi = ilo + lo;
    small = ihi + hi;
    ismall = small + kNttSmallCount;
    glo = ismall + kNttSmallCount;
    ghi = glo + lo;
    total = ghi + hi;
  }
};

template <class Fn>
void with_fr(int curve, Fn&& fn) {
  if (is_381(curve))
    fn.template operator()<Bls12_381_Fr29>();
  else
    fn.template operator()<Bls12_377_Fr29>();
}

void domain_release(mi355_msm_domain* d) {
  for (DevBuf* b : {&d->tables, &d->work, &d->stage, &d->poly, &d->pstage, &d->scan, &d->sstage, &d->quot, &d->qstage, &d->mle, &d->mstage, &d->logup, &d->lstage}) b->release();
  for (hipEvent_t& e : d->ev)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  if (d->own_stream) { (void)hipStreamDestroy(d->own_stream); d->own_stream = nullptr; }
}

// base^i for i < 2^h and base^(hi 2^h) for hi < 2^(k-h), enqueued on st
template <class FR>
void domain_two_level(mi355_msm_domain* d, const Fr& base, size_t lo_at, size_t hi_at, hipStream_t st) {
  Fr hb;
  ntt_hi_base<FR>(hb, base, ntt_lo_log(d->k));
  Fr* t = d->tables.as<Fr>();
  HIP_OK(LaunchNtt<FR>::table(base, (uint32_t)ntt_lo_count(d->k), t + lo_at, st));
  HIP_OK(LaunchNtt<FR>::table(hb, (uint32_t)ntt_hi_count(d->k), t + hi_at, st));
}

template <class FR>
void domain_build(mi355_msm_domain* d) {
  const NttLayout at(d->k);
  d->tables.reserve(at.total * sizeof(Fr));
  Fr root, small_root, iroot, ismall_root;
  ntt_root<FR>(root, d->k);
  ntt_root<FR>(small_root, NTT_SMALL_LOG);
  fr_inv<FR>(iroot, root);
  fr_inv<FR>(ismall_root, small_root);
  ntt_size_inv<FR>(d->size_inv, d->k);
  const hipStream_t st = d->own_stream;
  Fr* t = d->tables.as<Fr>();
  domain_two_level<FR>(d, root, at.wlo, at.whi, st);
  domain_two_level<FR>(d, iroot, at.ilo, at.ihi, st);
  HIP_OK(LaunchNtt<FR>::table(small_root, (uint32_t)kNttSmallCount, t + at.small, st));
  HIP_OK(LaunchNtt<FR>::table(ismall_root, (uint32_t)kNttSmallCount, t + at.ismall, st));
  HIP_OK(hipStreamSynchronize(st));
}

bool fr_same(const Fr& a, const Fr& b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }

// the offset of a coset call as the tables need it (host arithmetic): canonical, inverted for the inverse kind; refuses zero
template <class FR>
void domain_offset(Fr& g, const void* offset, unsigned kind, unsigned flags) {
  fr_zero(g);
  if (!(kind & kNttKindCoset)) return;
  if (offset) {
    uint32_t w[8];
    memcpy(w, offset, 32);
    fr_from_abi<FR>(g, w, (flags & kNttCallNormal) != 0);
    fr_reduce<FR>(g);
    Fr zero;
    fr_zero(zero);
    if (fr_same(g, zero)) bad_arg("the coset offset is zero");
  } else {
    fr_set<FR>(g, FR::GENERATOR);
  }
  if (kind & kNttKindInverse) fr_inv<FR>(g, g);
}

struct DomainCall {
  unsigned kind, flags;
  uint32_t in_len;
  size_t batch;
};

// everything a transform can be refused for, decided before any device call
void domain_check_call(mi355_msm_domain* d, const void* out, const void* in, size_t in_len, size_t batch, unsigned kind, unsigned flags, const void* offset,
                       bool device_ptrs) {
  if (!d) bad_arg("null domain handle");
  if (kind > kDomainKindMax) bad_arg("unknown transform kind %u (0 forward, 1 inverse, 2 coset forward, 3 coset inverse)", kind);
  if (flags & ~(kNttCallNormal | kNttCallNR | kNttCallRN))
    bad_arg("unknown transform flag bits 0x%x (bit 0: normal-form elements, bit 1: bit-reversed output, bit 2: bit-reversed input)", flags);
  if ((flags & kNttCallNR) && (kind & kNttKindInverse)) bad_arg("flag bit 1 (bit-reversed output) belongs to the forward kinds");
  if ((flags & kNttCallRN) && !(kind & kNttKindInverse)) bad_arg("flag bit 2 (bit-reversed input) belongs to the inverse kinds");
  if (offset && !(kind & kNttKindCoset)) bad_arg("an offset was given to a transform that is not over a coset");
  const size_t n = (size_t)1 << d->k;
  if (in_len > n) bad_arg("in_len %zu exceeds the domain size %zu", in_len, n);
  if (batch > 65535) bad_arg("batch %zu exceeds 65535", batch);
  if (batch && (!out || (!in && in_len))) bad_arg("null input or output pointer");
  if (batch && in && out != in) {
    // the bytes a call reads end with the in_len elements of the last vector; it writes whole vectors
    const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, wlen = (uintptr_t)(batch * n * 32), rlen = (uintptr_t)(((batch - 1) * n + in_len) * 32);
    if (rlen && a < b + wlen && b < a + rlen) bad_arg("input and output overlap in part (out == in is allowed)");
  }
  if (device_ptrs && (((uintptr_t)in | (uintptr_t)out) & 3)) bad_arg("device pointers must be 4-byte aligned");
}

// the passes of one call over `batch` vectors in device memory, enqueued on st; in == out is allowed
template <class FR>
void domain_enqueue(mi355_msm_domain* d, uint32_t* out, const uint32_t* in, const DomainCall& c, const Fr& g, hipStream_t st) {
  const NttLayout at(d->k);
  const size_t n = (size_t)1 << d->k;
  Fr* t = d->tables.as<Fr>();
  if (c.kind & kNttKindCoset) {
    if (!d->g_valid || !fr_same(g, d->g_have)) {
      d->g_valid = false;
      domain_two_level<FR>(d, g, at.glo, at.ghi, st);
      d->g_have = g;
      d->g_valid = true;
    }
  }
  uint32_t radix[NTT_MAX_LOG];
  const uint32_t npass = ntt_plan(d->k, d->pass_log, radix);
  d->work.reserve(c.batch * n * 32);
  uint32_t* work = d->work.as<uint32_t>();
  // the passes alternate between the work vectors and `out` and end in `out`; a call in place whose first pass would write over
  // its own input ends in the work vectors instead and is copied over
  const bool copy_back = (const uint32_t*)out == in && (npass & 1);
  const uint32_t* src = in;
  for (uint32_t i = 0; i < npass; i++) {
    NttPass ps;
    ntt_pass_shape(ps, d->k, radix, npass, i, c.kind, c.flags, c.in_len);
    const bool inv = (c.kind & kNttKindInverse) != 0;
    ps.w = NttTable{t + (inv ? at.ilo : at.wlo), t + (inv ? at.ihi : at.whi)};
    ps.g = NttTable{t + at.glo, t + at.ghi};
    ps.small = t + (inv ? at.ismall : at.small);
    ps.scale = d->size_inv;
    const bool to_out = (((npass - 1 - i) & 1) == 0) != copy_back;
    ps.src = src;
    ps.dst = to_out ? out : work;
    HIP_OK(LaunchNtt<FR>::pass(ps, (uint32_t)c.batch, st));
    src = ps.dst;
  }
  if (copy_back) HIP_OK(hipMemcpyAsync(out, work, c.batch * n * 32, hipMemcpyDeviceToDevice, st));
}

void domain_finish(mi355_msm_domain* d, std::chrono::steady_clock::time_point t0) {
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
  d->last_device_us = (uint64_t)(ms * 1000.0f);
  d->last_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

void domain_transform_device(mi355_msm_domain* d, void* out, const void* in, size_t in_len, size_t batch, unsigned kind, unsigned flags, const void* offset,
                             hipStream_t st) {
  domain_check_call(d, out, in, in_len, batch, kind, flags, offset, true);
  Fr g;
  with_fr(d->curve, [&]<class FR>() { domain_offset<FR>(g, offset, kind, flags); });
  if (batch == 0) return;
  HIP_OK(hipSetDevice(d->device));
  const DomainCall c{kind, flags, (uint32_t)in_len, batch};
  const auto t0 = std::chrono::steady_clock::now();
  try {
    HIP_OK(hipEventRecord(d->ev[0], st));
    with_fr(d->curve, [&]<class FR>() { domain_enqueue<FR>(d, (uint32_t*)out, (const uint32_t*)in, c, g, st); });
    HIP_OK(hipEventRecord(d->ev[1], st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  domain_finish(d, t0);
}

// Host pointers: one vector at a time is staged in (its first in_len elements), transformed in place in the staged vector and copied
// out, on the handle's stream.
void domain_transform_host(mi355_msm_domain* d, void* out, const void* in, size_t in_len, size_t batch, unsigned kind, unsigned flags, const void* offset) {
  domain_check_call(d, out, in, in_len, batch, kind, flags, offset, false);
  Fr g;
  with_fr(d->curve, [&]<class FR>() { domain_offset<FR>(g, offset, kind, flags); });
  if (batch == 0) return;
  HIP_OK(hipSetDevice(d->device));
  const hipStream_t st = d->own_stream;
  const size_t n = (size_t)1 << d->k;
  const DomainCall c{kind, flags, (uint32_t)in_len, 1};
  const auto t0 = std::chrono::steady_clock::now();
  try {
    d->stage.reserve(n * 32);
    HIP_OK(hipEventRecord(d->ev[0], st));
    for (size_t b = 0; b < batch; b++) {
      if (in_len) HIP_OK(hipMemcpyAsync(d->stage.p, (const uint8_t*)in + b * n * 32, in_len * 32, hipMemcpyHostToDevice, st));
      with_fr(d->curve, [&]<class FR>() { domain_enqueue<FR>(d, d->stage.as<uint32_t>(), d->stage.as<uint32_t>(), c, g, st); });
      HIP_OK(hipMemcpyAsync((uint8_t*)out + b * n * 32, d->stage.p, n * 32, hipMemcpyDeviceToHost, st));
      if (b + 1 == batch) HIP_OK(hipEventRecord(d->ev[1], st));
      HIP_OK(hipStreamSynchronize(st));   // (pageable host memory: the caller's buffers are free to go when the call returns)
    }
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  domain_finish(d, t0);
}

void domain_check_mul(mi355_msm_domain* d, const void* out, const void* a, const void* b, size_t n, unsigned flags, bool device_ptrs) {
  if (!d) bad_arg("null domain handle");
  if (flags & ~kNttCallNormal) bad_arg("unknown product flag bits 0x%x (bit 0: normal-form elements)", flags);
  if (n && (!out || !a || !b)) bad_arg("null input or output pointer");
  if (n > ((size_t)1 << 31)) bad_arg("%zu elements exceed 2^31", n);
  if (device_ptrs && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 3)) bad_arg("device pointers must be 4-byte aligned");
}

void domain_mul_device(mi355_msm_domain* d, void* out, const void* a, const void* b, size_t n, unsigned flags, hipStream_t st) {
  domain_check_mul(d, out, a, b, n, flags, true);
  if (n == 0) return;
  HIP_OK(hipSetDevice(d->device));
  const auto t0 = std::chrono::steady_clock::now();
  HIP_OK(hipEventRecord(d->ev[0], st));
  with_fr(d->curve, [&]<class FR>() {
    HIP_OK(LaunchNtt<FR>::mul_vec((const uint32_t*)a, (const uint32_t*)b, (uint32_t*)out, n, (flags & kNttCallNormal) != 0, st));
  });
  HIP_OK(hipEventRecord(d->ev[1], st));
  HIP_OK(hipStreamSynchronize(st));
  domain_finish(d, t0);
}

// host pointers, in pieces of one domain's worth through the staged vector and the work vector
void domain_mul_host(mi355_msm_domain* d, void* out, const void* a, const void* b, size_t n, unsigned flags) {
  domain_check_mul(d, out, a, b, n, flags, false);
  if (n == 0) return;
  HIP_OK(hipSetDevice(d->device));
  const hipStream_t st = d->own_stream;
  const size_t piece = (size_t)1 << d->k;
  const auto t0 = std::chrono::steady_clock::now();
  try {
    d->stage.reserve(piece * 32);
    d->work.reserve(piece * 32);
    HIP_OK(hipEventRecord(d->ev[0], st));
    for (size_t at = 0; at < n; at += piece) {
      const size_t cn = std::min(piece, n - at);
      HIP_OK(hipMemcpyAsync(d->stage.p, (const uint8_t*)a + at * 32, cn * 32, hipMemcpyHostToDevice, st));
      HIP_OK(hipMemcpyAsync(d->work.p, (const uint8_t*)b + at * 32, cn * 32, hipMemcpyHostToDevice, st));
      with_fr(d->curve, [&]<class FR>() {
        HIP_OK(LaunchNtt<FR>::mul_vec(d->stage.as<uint32_t>(), d->work.as<uint32_t>(), d->stage.as<uint32_t>(), cn, (flags & kNttCallNormal) != 0, st));
      });
      HIP_OK(hipMemcpyAsync((uint8_t*)out + at * 32, d->stage.p, cn * 32, hipMemcpyDeviceToHost, st));
      if (at + cn >= n) HIP_OK(hipEventRecord(d->ev[1], st));
      HIP_OK(hipStreamSynchronize(st));
    }
  } catch (...) {
    (void)hipStreamSynchronize(st);
    throw;
  }
  domain_finish(d, t0);
}

}  // namespace

extern "C" {

RustError mi355_msm_domain_create(mi355_msm_domain** out, int curve, int device, size_t num_coeffs) {
  return guarded_dev([&] {
    if (!out) bad_arg("null handle out-pointer");
    *out = nullptr;
    if (!known_curve(curve)) bad_arg("unknown curve id %d", curve);
    uint32_t k = 0;
    while (k < 63 && ((size_t)1 << k) < num_coeffs) k++;
    const uint32_t adicity = is_381(curve) ? (uint32_t)Bls12_381_Fr29::TWO_ADICITY : (uint32_t)Bls12_377_Fr29::TWO_ADICITY;
    if (k > adicity) bad_arg("%zu coefficients need a domain of 2^%u points, above the field's 2-adicity %u", num_coeffs, k, adicity);
    if (k > NTT_MAX_LOG) bad_arg("%zu coefficients need a domain of 2^%u points; this library goes up to 2^%u", num_coeffs, k, NTT_MAX_LOG);
    const int count = require_device();
    if (device >= count) bad_arg("device %d out of range (%d visible)", device, count);
    if (device < 0) HIP_OK(hipGetDevice(&device));
    HIP_OK(hipSetDevice(device));
    mi355_msm_domain* d = new mi355_msm_domain();
    d->curve = curve;
    d->device = device;
    d->k = k;
    try {
      HIP_OK(hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking));
      for (hipEvent_t& e : d->ev) HIP_OK(hipEventCreate(&e));
      with_fr(curve, [&]<class FR>() { domain_build<FR>(d); });
    } catch (...) {
      domain_release(d);
      delete d;
      throw;
    }
    *out = d;
  });
}

RustError mi355_msm_domain_transform(mi355_msm_domain* d, void* out, const void* in, size_t in_len, size_t batch, unsigned kind, unsigned flags,
                                     const void* offset) {
  return guarded_dev([&] { domain_transform_host(d, out, in, in_len, batch, kind, flags, offset); });
}

RustError mi355_msm_domain_transform_device(mi355_msm_domain* d, void* d_out, const void* d_in, size_t in_len, size_t batch, unsigned kind, unsigned flags,
                                            const void* offset, void* stream) {
  return guarded_dev([&] { domain_transform_device(d, d_out, d_in, in_len, batch, kind, flags, offset, (hipStream_t)stream); });
}

RustError mi355_msm_domain_mul(mi355_msm_domain* d, void* out, const void* a, const void* b, size_t n, unsigned flags) {
  return guarded_dev([&] { domain_mul_host(d, out, a, b, n, flags); });
}

RustError mi355_msm_domain_mul_device(mi355_msm_domain* d, void* d_out, const void* d_a, const void* d_b, size_t n, unsigned flags, void* stream) {
  return guarded_dev([&] { domain_mul_device(d, d_out, d_a, d_b, n, flags, (hipStream_t)stream); });
}

RustError mi355_msm_domain_set_option(mi355_msm_domain* d, const char* key, long value) {
  return guarded([&] {
    if (!d || !key) bad_arg("null argument");
    const std::string k(key);
    if (k == "pass_log") {   // butterfly levels per pass; 0 restores the default.  Results do not depend on it (a test hook)
      if (value < 0 || value > (long)NTT_MAX_PASS_LOG) bad_arg("pass_log %ld out of range [1, %u] (0 = default)", value, NTT_MAX_PASS_LOG);
      d->pass_log = value ? (uint32_t)value : NTT_DEFAULT_PASS_LOG;
    } else if (k == "poly_tile_log") {   // elements of a tile of the scans of msm_poly.hpp, as a power of two; 0 restores the default (a test hook)
      if (value != 0 && (value < (long)POLY_TILE_LOG_MIN || value > (long)POLY_TILE_LOG_MAX))
        bad_arg("poly_tile_log %ld out of range [%u, %u] (0 = default)", value, POLY_TILE_LOG_MIN, POLY_TILE_LOG_MAX);
      d->poly_tile_log = value ? (uint32_t)value : POLY_DEFAULT_TILE_LOG;
    } else
      bad_arg("unknown domain option '%s'", key);
  });
}

RustError mi355_msm_domain_query(mi355_msm_domain* d, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!key || !value) bad_arg("null argument");
    const std::string k(key);
    // the limits of a sumcheck round need no handle
    if (k == "sumcheck_max_tables") { *value = MLE_MAX_TABLES; return; }
    if (k == "sumcheck_max_terms") { *value = MLE_MAX_TERMS; return; }
    if (k == "sumcheck_max_factors") { *value = MLE_MAX_FACTORS; return; }
    if (!d) bad_arg("null argument");
    uint32_t radix[NTT_MAX_LOG];
    if (k == "size") *value = (uint64_t)1 << d->k;
    else if (k == "log_size") *value = d->k;
    else if (k == "passes") *value = ntt_plan(d->k, d->pass_log, radix);
    else if (k == "pass_log") *value = d->pass_log;
    else if (k == "table_bytes") *value = d->tables.bytes;
    else if (k == "work_bytes") *value = d->work.bytes + d->stage.bytes;
    else if (k == "poly_work_bytes") *value = d->poly.bytes + d->pstage.bytes;
    else if (k == "scan_work_bytes") *value = d->scan.bytes + d->sstage.bytes;
    else if (k == "quotient_work_bytes") *value = d->quot.bytes + d->qstage.bytes;
    else if (k == "mle_work_bytes") *value = d->mle.bytes + d->mstage.bytes;
    else if (k == "logup_work_bytes") *value = d->logup.bytes + d->lstage.bytes;
    else if (k == "sumcheck_levels") *value = d->mle_levels;
    else if (k == "poly_tile_log") *value = d->poly_tile_log;
    else if (k == "device") *value = (uint64_t)d->device;
    else if (k == "last_us") *value = d->last_us;
    else if (k == "last_device_us") *value = d->last_device_us;
    else bad_arg("unknown domain query '%s'", key);
  });
}

RustError mi355_msm_domain_element(mi355_msm_domain* d, uint64_t i, void* out32) {
  return guarded([&] {
    if (!d || !out32) bad_arg("null argument");
    with_fr(d->curve, [&]<class FR>() {
      Fr root, r;
      ntt_root<FR>(root, d->k);
      const uint64_t e = d->k ? i & (((uint64_t)1 << d->k) - 1) : 0;
      const uint32_t ew[8] = {(uint32_t)e, (uint32_t)(e >> 32), 0, 0, 0, 0, 0, 0};
      uint32_t w[8];
      fr_pow_words<FR>(r, root, ew);
      fr_to_abi<FR>(w, r, false);
      memcpy(out32, w, 32);
    });
  });
}

RustError mi355_msm_domain_destroy(mi355_msm_domain* d) {
  return guarded_dev([&] {
    if (!d) return;
    (void)hipSetDevice(d->device);
    domain_release(d);
    delete d;
  });
}

}  // extern "C"
