// msm_lookup.hpp -- resident lookup tables over Fr and the logUp running sum (included by msm_engine.hip after msm_gfft.hpp): the C ABI
// mi355_msm_lookup_{create, count, sorted, query, destroy} and mi355_msm_domain_logup_sum of include/mi355_msm.h over the kernels of
// lookup.hpp.
//
// A table belongs to a domain handle: the field, the device, the events and the stream of its host-pointer calls are the domain's.
// Everything else -- the canonical keys, the slots, the counters, the offsets and the levels of their scan, the staged vectors of a
// host-pointer call -- is the table's own (queries "table_bytes", "lookup_work_bytes"), so two tables on one domain do not disturb each
// other.  The logUp sum keeps its denominators, its terms and the levels of its inversion and its scan in the domain's `logup` (query
// "logup_work_bytes") and stages through `lstage`; `scan`, `poly` and the other work memory are not touched.  Every call judges its
// arguments first, the handle last.
#pragma once

#include "launch_lookup.hpp"

struct mi355_msm_lookup {
  mi355_msm_domain* d = nullptr;
  DevBuf keys, slots, work, stage;   // the canonical table; the hash table; head, counters, offsets, scan levels; staged vectors
  uint32_t n = 0, nslots = 0, distinct = 0, max_probe = 0;
  bool normal = false;
};

namespace {

constexpr size_t kLookupMaxTable = (size_t)1 << LOOKUP_MAX_TABLE_LOG, kLookupMaxValues = (size_t)1 << LOOKUP_MAX_VALUES_LOG;
constexpr size_t kLookupHeadBytes = 64;

template <class FR>
struct LookupEngineRun {
  hipStream_t st;
  void scan_up(const LookupScan& p) { HIP_OK(LaunchLookup<FR>::scan_up(p, st)); }
  void scan_down(const LookupScan& p) { HIP_OK(LaunchLookup<FR>::scan_down(p, st)); }
};

// the parts of a table's work memory
struct LookupWork {
  LookupHead* head;
  uint32_t *count, *off, *levels;
  explicit LookupWork(const mi355_msm_lookup* h) {
    uint8_t* p = (uint8_t*)h->work.p;
    head = (LookupHead*)p;
    count = (uint32_t*)(p + kLookupHeadBytes);
    off = count + h->n;
    levels = off + h->n;
  }
  static size_t bytes(size_t n) { return kLookupHeadBytes + 2 * n * 4 + (size_t)lookup_scan_work_words(n) * 4; }
};

void lookup_head_reset(LookupHead* head, hipStream_t on) {
  HIP_OK(hipMemsetAsync(head, 0, sizeof(LookupHead), on));
  HIP_OK(hipMemsetAsync(&head->first, 0xff, sizeof head->first, on));
}

// after the stream is idle
LookupHead lookup_head_fetch(const LookupHead* head) {
  LookupHead h;
  HIP_OK(hipMemcpy(&h, head, sizeof h, hipMemcpyDeviceToHost));
  if (h.err) throw HipFailure(-2, "mi355_msm: a walk of the lookup table wrapped around (internal error)");
  return h;
}

// runs of 256 values a block of the probe takes: one while the values do not fill the device (about 2^19 lanes in flight), then more, so
// that a heavy entry is added fewer times
uint32_t lookup_batches(size_t n_f) {
  const size_t b = n_f >> 20;
  return (uint32_t)(b < 1 ? 1 : b > LOOKUP_MAX_BATCHES ? LOOKUP_MAX_BATCHES : b);
}

LookupTab lookup_tab(const mi355_msm_lookup* h) { return LookupTab{h->keys.as<uint32_t>(), h->slots.as<uint32_t>(), h->n, h->nslots - 1}; }

void lookup_release(mi355_msm_lookup* h) {
  for (DevBuf* b : {&h->keys, &h->slots, &h->work, &h->stage}) b->release();
}

void lookup_create(mi355_msm_lookup** out, mi355_msm_domain* d, const void* table, size_t n_t, unsigned flags, hipStream_t st) {
  if (out) *out = nullptr;
  if (flags & ~(kLookupNormal | kLookupDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
  const bool device_ptrs = (flags & kLookupDevice) != 0;
  if (n_t < 1) bad_arg("a lookup table has at least one entry");
  if (n_t > kLookupMaxTable) bad_arg("%zu table entries exceed 2^28", n_t);
  if (!out || !table) bad_arg("null handle out-pointer or table pointer");
  poly_check_aligned(device_ptrs, {table});
  poly_check_stream(device_ptrs, st);
  poly_check_handle(d);
  HIP_OK(hipSetDevice(d->device));
  std::unique_ptr<mi355_msm_lookup> h(new mi355_msm_lookup());
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  h->d = d;
  h->n = (uint32_t)n_t;
  h->normal = (flags & kLookupNormal) != 0;
  uint32_t slots = 2;
  while (slots < 2 * n_t) slots <<= 1;
  h->nslots = slots;
  try {
    h->keys.reserve(n_t * 32);
    h->slots.reserve((size_t)slots * 4);
    h->work.reserve(LookupWork::bytes(n_t));
    const LookupWork w(h.get());
    LookupHead head{};
    poly_timed(d, on, [&] {
      FrStage g(h->stage, device_ptrs, on, n_t);
      const uint32_t* src = g.in(table, n_t);
      HIP_OK(hipMemsetAsync(h->slots.p, 0xff, (size_t)slots * 4, on));
      lookup_head_reset(w.head, on);
      with_fr(d->curve, [&]<class FR>() {
        HIP_OK(LaunchLookup<FR>::canon(LookupCanon{src, h->keys.as<uint32_t>(), n_t}, on));
        HIP_OK(LaunchLookup<FR>::build(LookupBuild{lookup_tab(h.get()), w.head}, on));
      });
    });
    h->stage.release();   // (the staged table of a host-pointer create: the stream is idle, and the keys are the handle's copy)
    head = lookup_head_fetch(w.head);
    h->distinct = head.distinct;
    h->max_probe = head.max_probe;
  } catch (...) {
    lookup_release(h.get());
    throw;
  }
  *out = h.release();
}

// what count and sorted share; returns the handle's form
void lookup_call_check(mi355_msm_lookup* h, const void* out, size_t out_elems_known, const uint32_t* index_out, const uint64_t* stats, const void* values,
                       size_t n_f, unsigned flags, hipStream_t st, bool out_required) {
  if (flags & ~(kLookupNormal | kLookupDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
  const bool device_ptrs = (flags & kLookupDevice) != 0;
  if (n_f > kLookupMaxValues) bad_arg("%zu values exceed 2^30", n_f);
  if (!stats || (n_f && !values) || (out_required && !out)) bad_arg("null input, output or stats pointer");
  poly_check_aligned(device_ptrs, {out, index_out, values});
  poly_check_stream(device_ptrs, st);
  const size_t index_elems = (n_f * 4 + 31) / 32;
  if ((out && out == values) || poly_overlap(out, out_elems_known, values, n_f) || poly_overlap(index_out, index_elems, values, n_f))
    bad_arg("an output overlaps the values");
  if (!h) bad_arg("null lookup handle");
  if (((flags & kLookupNormal) != 0) != h->normal)
    bad_arg("the table was created with %s elements and the call brings %s ones (flag bit 0)", h->normal ? "normal-form" : "Montgomery-form",
            h->normal ? "Montgomery-form" : "normal-form");
}

void lookup_stats_out(uint64_t* stats, const LookupHead& head, size_t n_f) {
  stats[0] = head.missing;
  stats[1] = head.missing ? head.first : n_f;
}

void lookup_count(mi355_msm_lookup* h, void* mult_out, uint32_t* index_out, uint64_t* stats, const void* values, size_t n_f, unsigned flags,
                  hipStream_t st) {
  lookup_call_check(h, mult_out, 0, index_out, stats, values, n_f, flags, st, false);
  const size_t index_elems = (n_f * 4 + 31) / 32;
  if (poly_overlap(mult_out, h->n, values, n_f) || poly_overlap(mult_out, h->n, index_out, index_elems)) bad_arg("an output overlaps the values or the other output");
  const bool device_ptrs = (flags & kLookupDevice) != 0;
  mi355_msm_domain* d = h->d;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const LookupWork w(h);
  poly_timed(d, on, [&] {
    FrStage g(h->stage, device_ptrs, on, n_f + (index_out ? index_elems : 0) + (mult_out ? h->n : 0));
    const uint32_t* src = g.in(values, n_f);
    uint32_t* idx = index_out ? (device_ptrs ? index_out : g.out(nullptr, index_elems)) : nullptr;
    uint32_t* dst = mult_out ? g.out(mult_out, h->n) : nullptr;
    HIP_OK(hipMemsetAsync(w.count, 0, (size_t)h->n * 4, on));
    lookup_head_reset(w.head, on);
    with_fr(d->curve, [&]<class FR>() {
      HIP_OK(LaunchLookup<FR>::probe(LookupProbe{lookup_tab(h), src, n_f, idx, w.count, w.head, lookup_batches(n_f)}, on));
      if (dst) {
        LookupMult p{w.count, dst, h->n, h->normal ? 1u : 0u, Fr{}};
        lookup_image_const<FR>(p.image);
        HIP_OK(LaunchLookup<FR>::mult(p, on));
      }
    });
    if (index_out && !device_ptrs && n_f) HIP_OK(hipMemcpyAsync(index_out, idx, n_f * 4, hipMemcpyDeviceToHost, on));
    if (dst) g.back(mult_out, dst, h->n);
  });
  lookup_stats_out(stats, lookup_head_fetch(w.head), n_f);
}

void lookup_sorted(mi355_msm_lookup* h, void* s_out, uint64_t* stats, const void* values, size_t n_f, unsigned flags, hipStream_t st) {
  lookup_call_check(h, s_out, n_f, nullptr, stats, values, n_f, flags, st, true);
  const size_t total = (size_t)h->n + n_f;
  if (poly_overlap(s_out, total, values, n_f)) bad_arg("an output overlaps the values");
  const bool device_ptrs = (flags & kLookupDevice) != 0;
  mi355_msm_domain* d = h->d;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const LookupWork w(h);
  LookupHead head{};
  poly_timed(d, on, [&] {
    FrStage g(h->stage, device_ptrs, on, n_f + total);
    const uint32_t* src = g.in(values, n_f);
    uint32_t* dst = g.out(s_out, total);
    HIP_OK(hipMemsetAsync(w.count, 0, (size_t)h->n * 4, on));
    lookup_head_reset(w.head, on);
    with_fr(d->curve, [&]<class FR>() { HIP_OK(LaunchLookup<FR>::probe(LookupProbe{lookup_tab(h), src, n_f, nullptr, w.count, w.head, lookup_batches(n_f)}, on)); });
    // whether anything is written depends on the count of the missing values: the one point where the host looks at the device
    HIP_OK(hipStreamSynchronize(on));
    head = lookup_head_fetch(w.head);
    if (head.missing) return;
    with_fr(d->curve, [&]<class FR>() {
      LookupEngineRun<FR> run{on};
      lookup_scan_chain(run, w.off, w.count, h->n, w.levels);
      HIP_OK(LaunchLookup<FR>::expand(LookupExpand{h->keys.as<uint32_t>(), w.off, dst, h->n, total}, on));
    });
    g.back(s_out, dst, total);
  });
  lookup_stats_out(stats, head, n_f);
}

// ---- the logUp running sum ----------------------------------------------------------------------------------------------------------------

void logup_check(mi355_msm_domain* d, const void* out, const void* helpers, const void* table, const void* mult, const void* values, size_t m, size_t stride,
                 size_t n, const void* beta, unsigned flags, hipStream_t st) {
  if (flags & ~(kLookupNormal | kLookupDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
  const bool device_ptrs = (flags & kLookupDevice) != 0;
  if (n > kPolyMaxN) bad_arg("%zu rows exceed 2^30", n);
  if (m < 1 || m > LOGUP_MAX_COLUMNS) bad_arg("%zu columns: the logUp sum takes 1 .. %u", m, LOGUP_MAX_COLUMNS);
  if (stride < n) bad_arg("a column stride of %zu elements is below the %zu rows", stride, n);
  if (stride > kPolyMaxN) bad_arg("a column stride of %zu elements exceeds 2^30", stride);
  if (!beta || (n && (!out || !table || !mult || !values))) bad_arg("null input or output pointer");
  poly_check_aligned(device_ptrs, {out, helpers, table, mult, values});
  poly_check_stream(device_ptrs, st);
  const size_t span = n ? (m - 1) * stride + n : 0, hn = (m + 1) * n;
  for (const void* o : {out, helpers}) {
    const size_t on = o == out ? n : hn;
    if (poly_overlap(o, on, table, n) || poly_overlap(o, on, mult, n) || poly_overlap(o, on, values, span)) bad_arg("an output overlaps an input");
  }
  if (poly_overlap(out, n, helpers, hn)) bad_arg("the running sum overlaps the helper columns");
  poly_check_handle(d);
}

void logup_call(mi355_msm_domain* d, void* out, void* total32, void* helpers, const void* table, const void* mult, const void* values, size_t m,
                size_t stride, size_t n, const void* beta, unsigned flags, hipStream_t st) {
  logup_check(d, out, helpers, table, mult, values, m, stride, n, beta, flags, st);
  const bool device_ptrs = (flags & kLookupDevice) != 0, normal = (flags & kLookupNormal) != 0;
  if (n == 0) {
    if (total32) scan_identity_out(d, total32, kScanSum, normal ? kScanNormal : 0u);
    return;
  }
  const size_t span = (m - 1) * stride + n, hn = (m + 1) * n;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  const Fr* res = nullptr;
  poly_timed(d, on, [&] {
    FrStage g(d->lstage, device_ptrs, on, span + 3 * n + (helpers ? hn : 0));
    LogupRows p{};
    p.values = g.in(values, span);
    p.table = g.in(table, n);
    p.mult = g.in(mult, n);
    uint32_t* dst = g.out(out, n);
    uint32_t* hdst = helpers ? g.out(helpers, hn) : nullptr;
    // work memory: the scan's levels, the inversion's tile products, the terms, the helper columns unless they are an output
    const size_t scan_elems = (size_t)scan_work_elems(n, d->poly_tile_log), inv_elems = (size_t)poly_work_elems(hn, d->poly_tile_log);
    d->logup.reserve((scan_elems + inv_elems) * sizeof(Fr) + n * 32 + (helpers ? 0 : hn * 32));
    Fr* work = d->logup.as<Fr>();
    p.term = (uint32_t*)(work + scan_elems + inv_elems);
    p.helpers = hdst ? hdst : p.term + n * 8;
    p.n = n;
    p.stride = stride;
    p.m = (uint32_t)m;
    p.normal = normal ? 1u : 0u;
    with_fr(d->curve, [&]<class FR>() {
      poly_scalar<FR>(p.beta, beta, normal);
      HIP_OK(LaunchLookup<FR>::logup_den(p, on));
      Fr one;
      fr_set<FR>(one, FR::ONE);
      PolyRun<FR> inv{on};
      poly_chain_inverse<FR>(inv, p.helpers, p.helpers, hn, normal, d->poly_tile_log, one, work + scan_elems);
      HIP_OK(LaunchLookup<FR>::logup_term(p, on));
    });
    res = scan_enqueue(d, dst, p.term, nullptr, n, kScanSum, normal ? kScanNormal : 0u, work, on);
    g.back(out, dst, n);
    if (hdst) g.back(helpers, hdst, hn);
  });
  if (total32) poly_fetch(d, total32, res, normal ? kPolyNormal : 0u);
}

}  // namespace

extern "C" {

RustError mi355_msm_lookup_create(mi355_msm_lookup** out, mi355_msm_domain* d, const void* table, size_t n_t, unsigned flags, void* stream) {
  return guarded_dev([&] { lookup_create(out, d, table, n_t, flags, (hipStream_t)stream); });
}

RustError mi355_msm_lookup_count(mi355_msm_lookup* h, void* mult_out, uint32_t* index_out, uint64_t* stats, const void* values, size_t n_f, unsigned flags,
                                 void* stream) {
  return guarded_dev([&] { lookup_count(h, mult_out, index_out, stats, values, n_f, flags, (hipStream_t)stream); });
}

RustError mi355_msm_lookup_sorted(mi355_msm_lookup* h, void* s_out, uint64_t* stats, const void* values, size_t n_f, unsigned flags, void* stream) {
  return guarded_dev([&] { lookup_sorted(h, s_out, stats, values, n_f, flags, (hipStream_t)stream); });
}

RustError mi355_msm_lookup_query(mi355_msm_lookup* h, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!key || !value) bad_arg("null argument");
    const std::string k(key);
    if (!h) bad_arg("null lookup handle");
    if (k == "n") *value = h->n;
    else if (k == "slots") *value = h->nslots;
    else if (k == "distinct") *value = h->distinct;
    else if (k == "max_probe") *value = h->max_probe;
    else if (k == "table_bytes") *value = h->keys.bytes + h->slots.bytes;
    else if (k == "lookup_work_bytes") *value = h->work.bytes + h->stage.bytes;
    else bad_arg("unknown lookup query '%s'", key);
  });
}

RustError mi355_msm_lookup_destroy(mi355_msm_lookup* h) {
  return guarded_dev([&] {
    if (!h) return;
    (void)hipSetDevice(h->d->device);
    lookup_release(h);
    delete h;
  });
}

RustError mi355_msm_domain_logup_sum(mi355_msm_domain* d, void* out, void* total32, void* helpers, const void* table, const void* mult, const void* values,
                                     size_t m, size_t stride, size_t n, const void* beta, unsigned flags, void* stream) {
  return guarded_dev([&] { logup_call(d, out, total32, helpers, table, mult, values, m, stride, n, beta, flags, (hipStream_t)stream); });
}

}  // extern "C"
