// msm_poseidon.hpp -- resident Poseidon parameters over Fr, batches of sponges and Merkle trees (included by msm_engine.hip after
// msm_mle.hpp): the C ABI mi355_msm_poseidon_{create, hash, merkle, set_option, query, destroy} of include/mi355_msm.h over the kernel
// of poseidon.hpp.
//
// A parameter handle belongs to a domain handle: the field, the device, the stream of its host-pointer calls and the events of a
// call are the domain's.  The table (the caller's constants and matrix, the sparse form of the partial rounds, the reductions of each
// round) and the staged vectors of a host-pointer call are the handle's own (query "work_bytes"); hash and merkle stage through
// `stage` with the FrStage of fr_stage.hpp.  create derives the sparse form in host arithmetic; every call judges its arguments
// first, the handle last.
#pragma once

#include "launch_poseidon.hpp"

struct mi355_msm_poseidon {
  mi355_msm_domain* d = nullptr;
  PosPlan plan;
  PosTab tab{};
  const uint32_t* zeros = nullptr;   // two zero elements behind the table: the children of the empty hash
  bool sparse = true;
  DevBuf table, stage;
};

namespace {

constexpr size_t kPosMaxN = (size_t)1 << POS_MAX_N_LOG;

template <class FR>
struct PosEngineRun {
  hipStream_t st;
  void hash(const PosRun& p) { HIP_OK(LaunchPoseidon<FR>::hash(p, st)); }
  void fill(uint32_t* first, uint64_t count) {
    for (uint64_t have = 1; have < count;) {
      const uint64_t c = std::min(have, count - have);
      HIP_OK(hipMemcpyAsync(first + have * 8, first, c * 32, hipMemcpyDeviceToDevice, st));
      have += c;
    }
  }
};

void pos_create(mi355_msm_poseidon** out, mi355_msm_domain* d, unsigned rate, unsigned alpha, unsigned rf, unsigned rp, const void* ark, const void* mds,
                unsigned flags) {
  if (out) *out = nullptr;
  if (flags & ~kPosNormal) bad_arg("unknown flag bits 0x%x (bit 0: the parameters are plain integers)", flags);
  if (const char* why = pos_check_shape(rate, alpha, rf, rp)) bad_arg("%s (rate %u, alpha %u, %u full and %u partial rounds)", why, rate, alpha, rf, rp);
  if (!out || !ark || !mds) bad_arg("null handle out-pointer, ark or mds");
  if (!d) bad_arg("null domain handle");
  const uint32_t t = rate + 1, rounds = rf + rp;
  std::unique_ptr<mi355_msm_poseidon> p(new mi355_msm_poseidon());
  p->d = d;
  with_fr(d->curve, [&]<class FR>() {
    std::vector<Fr> a((size_t)rounds * t), m((size_t)t * t);
    for (size_t i = 0; i < a.size(); i++) poly_scalar<FR>(a[i], (const uint8_t*)ark + 32 * i, (flags & kPosNormal) != 0);
    for (size_t i = 0; i < m.size(); i++) poly_scalar<FR>(m[i], (const uint8_t*)mds + 32 * i, (flags & kPosNormal) != 0);
    char why[256];
    if (!pos_build<FR>(p->plan, rate, alpha, rf, rp, a.data(), m.data(), why, sizeof why)) bad_arg("%s", why);
  });
  std::vector<uint8_t> img;
  pos_table_fill(img, p->plan);
  const size_t tab_bytes = img.size();
  img.resize(tab_bytes + 64, 0);
  HIP_OK(hipSetDevice(d->device));
  const hipStream_t st = d->own_stream;
  try {
    p->table.reserve(img.size());
    HIP_OK(hipMemcpyAsync(p->table.p, img.data(), img.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
  } catch (...) {
    (void)hipStreamSynchronize(st);
    p->table.release();
    throw;
  }
  p->tab = pos_table_at(p->table.p, p->plan);
  p->zeros = (const uint32_t*)((const uint8_t*)p->table.p + tab_bytes);
  *out = p.release();
}

// what every launch of a call shares
template <class FR>
PosRun pos_base(const mi355_msm_poseidon* p, bool normal) {
  PosRun r{};
  r.tab = p->tab;
  r.sparse = p->sparse ? 1u : 0u;
  fr_const<FR>(r.cin, normal ? 1 : 0);
  fr_const<FR>(r.cout, normal ? 3 : 2);
  return r;
}

void pos_hash(mi355_msm_poseidon* p, void* out, const void* in, size_t n, size_t in_len, size_t n_out, const void* header, unsigned flags, hipStream_t st) {
  if (flags & ~(kPosNormal | kPosDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
  const bool device_ptrs = (flags & kPosDevice) != 0, normal = (flags & kPosNormal) != 0;
  if (n > kPosMaxN) bad_arg("%zu sponges exceed 2^30", n);
  if (in_len > POS_MAX_LEN) bad_arg("%zu input elements per sponge exceed 2^16", in_len);
  if (n_out > POS_MAX_LEN) bad_arg("%zu output elements per sponge exceed 2^16", n_out);
  if ((n && n_out && !out) || (n && in_len && !in)) bad_arg("null input or output pointer");
  poly_check_aligned(device_ptrs, {out, in});
  poly_check_stream(device_ptrs, st);
  if (poly_overlap(out, n * n_out, in, n * in_len)) bad_arg("the output overlaps the input");
  if (!p) bad_arg("null parameter handle");
  if (n == 0 || n_out == 0) return;
  mi355_msm_domain* d = p->d;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(p->stage, device_ptrs, on, n * in_len + n * n_out);
    const uint32_t* src = g.in(in, n * in_len);
    uint32_t* dst = g.out(out, n * n_out);
    with_fr(d->curve, [&]<class FR>() {
      PosRun r = pos_base<FR>(p, normal);
      r.in = src;
      r.out = dst;
      r.n = n;
      r.row_stride = in_len;
      r.in_len = (uint32_t)in_len;
      r.n_out = (uint32_t)n_out;
      r.lead = kPosLeadNone;
      r.has_header = header ? 1u : 0u;
      if (header)
        for (uint32_t e = 0; e < p->tab.rate; e++) poly_scalar<FR>(r.hdr[e], (const uint8_t*)header + 32 * e, normal);
      HIP_OK(LaunchPoseidon<FR>::hash(r, on));
    });
    g.back(out, dst, n * n_out);
  });
}

void pos_merkle(mi355_msm_poseidon* p, void* tree_out, const void* leaves, size_t n_leaves, size_t leaf_len, const void* domain_sep, unsigned flags,
                hipStream_t st) {
  if (flags & ~(kPosNormal | kPosDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
  const bool device_ptrs = (flags & kPosDevice) != 0, normal = (flags & kPosNormal) != 0;
  if (n_leaves < 1 || n_leaves > kPosMaxN) bad_arg("%zu leaves: a tree has 1 .. 2^30", n_leaves);
  if (leaf_len >= POS_MAX_LEN) bad_arg("%zu elements per leaf exceed 2^16 - 1", leaf_len);
  if (!tree_out || !domain_sep || (leaf_len && !leaves)) bad_arg("null tree, leaves or domain separator pointer");
  poly_check_aligned(device_ptrs, {tree_out, leaves});
  poly_check_stream(device_ptrs, st);
  size_t P = 1;
  while (P < n_leaves) P *= 2;
  if (poly_overlap(tree_out, 2 * P - 1, leaves, n_leaves * leaf_len)) bad_arg("the tree overlaps the leaves");
  if (!p) bad_arg("null parameter handle");
  if (p->tab.rate < 2) bad_arg("a Merkle tree needs a rate of at least 2 (the header holds the domain and the length)");
  mi355_msm_domain* d = p->d;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(p->stage, device_ptrs, on, n_leaves * leaf_len + 2 * P - 1);
    const uint32_t* src = g.in(leaves, n_leaves * leaf_len);
    uint32_t* dst = g.out(tree_out, 2 * P - 1);
    with_fr(d->curve, [&]<class FR>() {
      const PosRun base = pos_base<FR>(p, normal);
      Fr hl[POS_MAX_RATE], hn[POS_MAX_RATE];
      for (uint32_t e = 0; e < POS_MAX_RATE; e++) {
        fr_zero(hl[e]);
        fr_zero(hn[e]);
      }
      uint8_t len[32] = {0};
      poly_scalar<FR>(hl[0], domain_sep, normal);
      hn[0] = hl[0];
      for (int q = 0; q < 4; q++) len[q] = (uint8_t)((leaf_len + 1) >> (8 * q));
      poly_scalar<FR>(hl[1], len, true);
      len[0] = 3;
      len[1] = len[2] = len[3] = 0;
      poly_scalar<FR>(hn[1], len, true);
      PosEngineRun<FR> run{on};
      pos_merkle_chain(run, base, dst, src, n_leaves, (uint32_t)leaf_len, hl, hn, p->zeros);
    });
    g.back(tree_out, dst, 2 * P - 1);
  });
}

}  // namespace

extern "C" {

RustError mi355_msm_poseidon_create(mi355_msm_poseidon** out, mi355_msm_domain* d, unsigned rate, unsigned alpha, unsigned full_rounds,
                                    unsigned partial_rounds, const void* ark, const void* mds, unsigned flags) {
  return guarded_dev([&] { pos_create(out, d, rate, alpha, full_rounds, partial_rounds, ark, mds, flags); });
}

RustError mi355_msm_poseidon_hash(mi355_msm_poseidon* p, void* out, const void* in, size_t n, size_t in_len, size_t n_out, const void* header,
                                  unsigned flags, void* stream) {
  return guarded_dev([&] { pos_hash(p, out, in, n, in_len, n_out, header, flags, (hipStream_t)stream); });
}

RustError mi355_msm_poseidon_merkle(mi355_msm_poseidon* p, void* tree_out, const void* leaves, size_t n_leaves, size_t leaf_len, const void* domain_sep,
                                    unsigned flags, void* stream) {
  return guarded_dev([&] { pos_merkle(p, tree_out, leaves, n_leaves, leaf_len, domain_sep, flags, (hipStream_t)stream); });
}

RustError mi355_msm_poseidon_set_option(mi355_msm_poseidon* p, const char* key, long value) {
  return guarded([&] {
    if (!key) bad_arg("null argument");
    if (!p) bad_arg("null parameter handle");
    const std::string k(key);
    if (k == "sparse") {   // 0: the partial rounds run densely from the caller's ark and mds (a test hook and the A/B of the measurement)
      if (value != 0 && value != 1) bad_arg("sparse is 0 or 1");
      p->sparse = value != 0;
    } else {
      bad_arg("unknown Poseidon option '%s'", key);
    }
  });
}

RustError mi355_msm_poseidon_query(mi355_msm_poseidon* p, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!key || !value) bad_arg("null argument");
    const std::string k(key);
    if (k == "block_lanes") { *value = POS_LANES; return; }   // a constant of the kernel needs no handle
    if (!p) bad_arg("null parameter handle");
    if (k == "rate") *value = p->tab.rate;
    else if (k == "state") *value = p->tab.t;
    else if (k == "rounds") *value = p->tab.rf + p->tab.rp;
    else if (k == "sparse") *value = p->sparse ? 1 : 0;
    else if (k == "products_per_permutation") *value = p->sparse ? p->plan.products_s : p->plan.products_d;
    else if (k == "lds_bytes") *value = pos_lds_bytes(p->tab.t);
    else if (k == "work_bytes") *value = p->table.bytes + p->stage.bytes;
    else bad_arg("unknown Poseidon query '%s'", key);
  });
}

RustError mi355_msm_poseidon_destroy(mi355_msm_poseidon* p) {
  return guarded_dev([&] {
    if (!p) return;
    (void)hipSetDevice(p->d->device);
    for (DevBuf* b : {&p->table, &p->stage}) b->release();
    delete p;
  });
}

}  // extern "C"
