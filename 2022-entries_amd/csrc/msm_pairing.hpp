// msm_pairing.hpp -- batch pairings and pairing products (included by msm_engine.hip after msm_poseidon.hpp): the C ABI
// mi355_msm_pairing_{create, run, check, query, destroy} of include/mi355_msm.h over the kernels of pairing.hpp.
//
// A pairing handle belongs to a device and a family (any of the four curve ids selects its family).  It owns the three programs and the
// constant table create writes, a stream for its host-pointer calls, the staged images of such a call, and the two
// lane-interleaved workspaces, which are sized by the lanes in flight of one chunk (pr_plan) and grown on demand -- never by n.
// Every call judges its arguments first, in the order of the header, and the handle last.
#pragma once

#include "launch_pairing.hpp"

struct mi355_msm_pairing {
  int curve = 0, device = 0;
  hipStream_t own_stream = nullptr;
  DevBuf table, ws, ws_f, stage;
  const Fe2* consts[2] = {nullptr, nullptr};           // for Montgomery and for canonical images
  const PrOp* prog[3] = {nullptr, nullptr, nullptr};   // Miller loop, product step, final exponentiation
  uint32_t len[3] = {0, 0, 0};
  uint64_t products[3] = {0, 0, 0};
  uint64_t last_launches = 0;
};

namespace {

template <class Fn>
void with_pairing_family(int curve, Fn&& fn) {
  if (is_381(curve)) fn.template operator()<Fp2El<Bls12_381_Fq, 1>>();
  else fn.template operator()<Fp2El<Bls12_377_Fq, 5>>();
}

template <class E>
struct PrEngineRun {
  hipStream_t st;
  uint64_t launches = 0;
  void miller(const PrRun& p, uint64_t items) { HIP_OK(LaunchPairing<E>::miller(p, items, st)); launches++; }
  void product(const PrRun& p, uint64_t lanes) { HIP_OK(LaunchPairing<E>::product(p, lanes, st)); launches++; }
  void final(const PrRun& p, uint64_t groups) { HIP_OK(LaunchPairing<E>::final(p, groups, st)); launches++; }
};

void pairing_release(mi355_msm_pairing* h) {
  (void)hipSetDevice(h->device);
  for (DevBuf* b : {&h->table, &h->ws, &h->ws_f, &h->stage}) b->release();
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  h->own_stream = nullptr;
}

void pairing_create(mi355_msm_pairing** out, int curve, int device) {
  if (!out) bad_arg("null handle out-pointer");
  *out = nullptr;
  if (!known_curve(curve)) bad_arg("unknown curve id %d", curve);
  const int count = require_device();
  if (device >= count) bad_arg("device %d out of range (%d visible)", device, count);
  if (device < 0) HIP_OK(hipGetDevice(&device));
  HIP_OK(hipSetDevice(device));
  std::unique_ptr<mi355_msm_pairing> h(new mi355_msm_pairing());
  h->curve = curve;
  h->device = device;
  // the table: the constants, then the three programs
  std::vector<uint8_t> img;
  size_t at[3];
  with_pairing_family(curve, [&]<class E>() {
    Fe2 consts[2][PR_CONSTS];
    pr_consts<E>(consts[0], false);
    pr_consts<E>(consts[1], true);
    PrGen<E> g[3];
    g[0].miller();
    g[1].accumulate();
    g[2].final_exponentiation();
    img.assign((const uint8_t*)consts, (const uint8_t*)consts + sizeof consts);
    for (int k = 0; k < 3; k++) {
      if (!g[k].check()) bad_arg("internal: a pairing program names a slot outside the workspace");
      at[k] = img.size();
      const uint8_t* b = (const uint8_t*)g[k].ops.data();
      img.insert(img.end(), b, b + g[k].ops.size() * sizeof(PrOp));
      h->len[k] = (uint32_t)g[k].ops.size();
      h->products[k] = g[k].products;
    }
    h->products[0] -= h->products[1];   // the Miller program ends with one product step
  });
  try {
    HIP_OK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->table.reserve(img.size());
    HIP_OK(hipMemcpyAsync(h->table.p, img.data(), img.size(), hipMemcpyHostToDevice, h->own_stream));
    HIP_OK(hipStreamSynchronize(h->own_stream));
  } catch (...) {
    pairing_release(h.get());
    throw;
  }
  h->consts[0] = (const Fe2*)h->table.p;
  h->consts[1] = h->consts[0] + PR_CONSTS;
  for (int k = 0; k < 3; k++) h->prog[k] = (const PrOp*)((const uint8_t*)h->table.p + at[k]);
  *out = h.release();
}

bool pr_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// run (check = false: n / group Gt images) and check (one byte per group)
void pairing_call(mi355_msm_pairing* h, void* out, const void* g1, size_t g1_stride, const void* g2, size_t g2_stride, size_t n, size_t group, unsigned flags,
                  hipStream_t st, bool check) {
  const unsigned known = check ? (unsigned)kPrDevice : (unsigned)(kPrCanonical | kPrDevice);
  if (flags & ~known) bad_arg("unknown flag bits 0x%x (%sbit 1: device pointers)", flags, check ? "" : "bit 0: canonical images, ");
  if (group == 0 || n % group) bad_arg("%zu pairs are not whole groups of %zu", n, group);
  if (g1_stride < 104 || g2_stride < 200 || (g1_stride & 3) || (g2_stride & 3))
    bad_arg("strides %zu / %zu: a G1 image has at least 104 bytes, a G2 image at least 200, both a multiple of 4", g1_stride, g2_stride);
  if (n && (!out || !g1 || !g2)) bad_arg("null output, G1 or G2 pointer");
  const bool device_ptrs = (flags & kPrDevice) != 0;
  if (device_ptrs && (((uintptr_t)out & (check ? 0 : 3)) || ((uintptr_t)g1 & 3) || ((uintptr_t)g2 & 3))) bad_arg("device pointers must be 4-byte aligned");
  poly_check_stream(device_ptrs, st);
  const size_t unit = check ? 1 : PR_GT_BYTES, groups = n / group;
  if (pr_overlap(out, groups * unit, g1, n * g1_stride) || pr_overlap(out, groups * unit, g2, n * g2_stride)) bad_arg("the output overlaps an input");
  if (!h) bad_arg("null pairing handle");
  if (n == 0) return;
  HIP_OK(hipSetDevice(h->device));
  const hipStream_t on = device_ptrs ? st : h->own_stream;
  const PrPlan pl = pr_plan(n, group);
  try {
    h->ws.reserve(pr_ws_words(pl) * 4);
    h->ws_f.reserve(pr_wsf_words(pl) * 4);
    const uint8_t* a = (const uint8_t*)g1;
    const uint8_t* b = (const uint8_t*)g2;
    uint8_t* dst = (uint8_t*)out;
    if (!device_ptrs) {
      const size_t ab = n * g1_stride, bb = n * g2_stride, ob = (groups * unit + 3) & ~(size_t)3;
      h->stage.reserve(ab + bb + ob);
      uint8_t* s = h->stage.as<uint8_t>();
      HIP_OK(hipMemcpyAsync(s, g1, ab, hipMemcpyHostToDevice, on));
      HIP_OK(hipMemcpyAsync(s + ab, g2, bb, hipMemcpyHostToDevice, on));
      a = s;
      b = s + ab;
      dst = s + ab + bb;
    }
    PrRun r{};
    r.miller = h->prog[0]; r.miller_len = h->len[0];
    r.accum = h->prog[1]; r.accum_len = h->len[1];
    r.fexp = h->prog[2]; r.fexp_len = h->len[2];
    r.consts = h->consts[check || (flags & kPrCanonical) ? 1 : 0];
    r.ws = h->ws.as<uint32_t>(); r.pitch = pr_ws_items(pl);
    r.ws_f = h->ws_f.as<uint32_t>(); r.pitch_f = pl.chunk_groups;
    r.g1 = a; r.g1_stride = g1_stride;
    r.g2 = b; r.g2_stride = g2_stride;
    r.group = pl.group; r.run = pl.run; r.parts = pl.parts;
    r.flags = (flags & kPrCanonical) | (check ? (unsigned)kPrCheck : 0u);
    with_pairing_family(h->curve, [&]<class E>() {
      PrEngineRun<E> run{on};
      pr_chain(run, r, pl, dst, unit);
      h->last_launches = run.launches;
    });
    if (!device_ptrs) HIP_OK(hipMemcpyAsync(out, dst, groups * unit, hipMemcpyDeviceToHost, on));
    HIP_OK(hipStreamSynchronize(on));   // the workspaces are the handle's: the next call may grow them
  } catch (...) {
    (void)hipStreamSynchronize(on);
    throw;
  }
}

}  // namespace

extern "C" {

RustError mi355_msm_pairing_create(mi355_msm_pairing** out, int curve, int device) {
  return guarded_dev([&] { pairing_create(out, curve, device); });
}

RustError mi355_msm_pairing_run(mi355_msm_pairing* h, void* out, const void* g1, size_t g1_stride, const void* g2, size_t g2_stride, size_t n, size_t group,
                                unsigned flags, void* stream) {
  return guarded_dev([&] { pairing_call(h, out, g1, g1_stride, g2, g2_stride, n, group, flags, (hipStream_t)stream, false); });
}

RustError mi355_msm_pairing_check(mi355_msm_pairing* h, uint8_t* ok, const void* g1, size_t g1_stride, const void* g2, size_t g2_stride, size_t n, size_t group,
                                  unsigned flags, void* stream) {
  return guarded_dev([&] { pairing_call(h, ok, g1, g1_stride, g2, g2_stride, n, group, flags, (hipStream_t)stream, true); });
}

RustError mi355_msm_pairing_query(mi355_msm_pairing* h, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!key || !value) bad_arg("null argument");
    const std::string k(key);
    // constants of the kernels need no handle
    if (k == "block_lanes") { *value = PR_LANES; return; }
    if (k == "lane_bytes") { *value = (uint64_t)PR_SLOTS * PR_FE2_WORDS * 4; return; }
    if (k == "max_lanes") { *value = PR_MAX_ITEMS; return; }
    if (k == "serial_group") { *value = PR_SERIAL_GROUP; return; }
    if (!h) bad_arg("null pairing handle");
    if (k == "workspace_bytes") *value = h->ws.bytes + h->ws_f.bytes;
    else if (k == "work_bytes") *value = h->ws.bytes + h->ws_f.bytes + h->stage.bytes + h->table.bytes;
    else if (k == "last_launches") *value = h->last_launches;
    else if (k == "device") *value = (uint64_t)h->device;
    else if (k == "curve") *value = (uint64_t)h->curve;
    else if (k == "products_miller") *value = 4 * h->products[0];      // Fp products: an Fp2 product is two fused dual products
    else if (k == "products_product_step") *value = 4 * h->products[1];
    else if (k == "products_final_exponentiation") *value = 4 * h->products[2];
    else if (k == "program_ops") *value = (uint64_t)h->len[0] + h->len[1] + h->len[2];
    else bad_arg("unknown pairing query '%s'", key);
  });
}

RustError mi355_msm_pairing_destroy(mi355_msm_pairing* h) {
  return guarded_dev([&] {
    if (!h) return;
    pairing_release(h);
    delete h;
  });
}

}  // extern "C"
