// msm_expr.hpp -- compiled custom-gate expressions over Fr columns (included by msm_engine.hip after msm_lookup.hpp): the C ABI
// mi355_msm_expr_{create, run, query, destroy} of include/mi355_msm.h over the compiler and the kernel of expr.hpp.
//
// A program belongs to a domain handle: the field, the device, the events and the stream of its host-pointer calls are the domain's.
// The instructions and the constants (`code`), the column references and the challenges of the most recent run (`args`) and the staged
// vectors of a host-pointer run (`stage`) are the program's own, so two programs on one domain do not disturb each other.  Every call
// judges its arguments first, the handle last; what only the program can decide (the counts it was created with, which column the
// output may be) comes right after the handle.
#pragma once

#include "launch_expr.hpp"

struct mi355_msm_expr {
  mi355_msm_domain* d = nullptr;
  ExprProgram prog;
  DevBuf code, args, stage;
};

namespace {

constexpr size_t kExprMaxLen = (size_t)1 << EXPR_MAX_LEN_LOG;

void expr_release(mi355_msm_expr* h) {
  for (DevBuf* b : {&h->code, &h->args, &h->stage}) b->release();
}

// one element of the caller's (in the form of the call) -> the 8 stored words of a constant operand
template <class FR>
void expr_operand_words(uint32_t* w8, const void* bytes32, bool normal) {
  Fr x;
  uint32_t w[8];
  poly_scalar<FR>(x, bytes32, normal);
  fr_pack(w, x);
  memcpy(w8, w, 32);
}

void expr_create(mi355_msm_expr** out, mi355_msm_domain* d, const uint32_t* nodes, size_t n_nodes, const void* consts, size_t n_consts, size_t n_chal,
                 size_t n_cols, unsigned flags) {
  if (out) *out = nullptr;
  if (flags & ~kExprNormal) bad_arg("unknown flag bits 0x%x (bit 0: the constants are plain integers)", flags);
  if (!out || !nodes || (n_consts && !consts)) bad_arg("null handle out-pointer, node pointer or constant pointer");
  char msg[256];
  if (!expr_check_dag(nodes, n_nodes, n_consts, n_chal, n_cols, msg, sizeof msg)) bad_arg("%s", msg);
  poly_check_handle(d);
  HIP_OK(hipSetDevice(d->device));
  std::unique_ptr<mi355_msm_expr> h(new mi355_msm_expr());
  h->d = d;
  bool ok = false;
  with_fr(d->curve, [&]<class FR>() { ok = expr_compile(h->prog, nodes, n_nodes, n_consts, n_chal, n_cols, expr_store_limit<FR>(), msg, sizeof msg); });
  if (!ok) bad_arg("%s", msg);
  std::vector<uint32_t> img(h->prog.code);
  img.resize(img.size() + n_consts * 8);
  with_fr(d->curve, [&]<class FR>() {
    for (size_t k = 0; k < n_consts; k++)
      expr_operand_words<FR>(img.data() + h->prog.code.size() + k * 8, (const uint8_t*)consts + k * 32, (flags & kExprNormal) != 0);
  });
  try {
    h->code.reserve(img.size() * 4);
    HIP_OK(hipMemcpy(h->code.p, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  } catch (...) {
    expr_release(h.get());
    throw;
  }
  *out = h.release();
}

void expr_run(mi355_msm_expr* h, void* out, const void* const* cols, const size_t* lens, size_t ncols, size_t len, size_t rot_step, const void* challenges,
              size_t nchal, unsigned flags, hipStream_t st) {
  if (flags & ~(kExprNormal | kExprDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
  const bool device_ptrs = (flags & kExprDevice) != 0, normal = (flags & kExprNormal) != 0;
  if (len > kExprMaxLen) bad_arg("%zu rows exceed 2^30", len);
  if (ncols > EXPR_MAX_COLS) bad_arg("%zu columns exceed %u", ncols, EXPR_MAX_COLS);
  if (nchal > EXPR_MAX_CHALS) bad_arg("%zu challenges exceed %u", nchal, EXPR_MAX_CHALS);
  if ((len && !out) || (ncols && (!cols || !lens)) || (nchal && !challenges)) bad_arg("null output, column, length or challenge pointer");
  for (size_t j = 0; j < ncols; j++) {
    if (lens[j] == 0) bad_arg("column %zu has length 0", j);
    if (len % lens[j]) bad_arg("the length %zu of column %zu does not divide the %zu rows", lens[j], j, len);
    if (len && !cols[j]) bad_arg("column %zu is a null pointer", j);
  }
  poly_check_aligned(device_ptrs, {out});
  for (size_t j = 0; j < ncols; j++) poly_check_aligned(device_ptrs, {cols[j]});
  poly_check_stream(device_ptrs, st);
  // the output may BE a full-length column (judged against the program below); any other overlap is refused
  for (size_t j = 0; j < ncols && len; j++)
    if (!(out == cols[j] && lens[j] == len) && poly_overlap(out, len, cols[j], lens[j]))
      bad_arg("the output overlaps column %zu (it may BE one full-length column that is read at rotation 0 only)", j);
  if (!h) bad_arg("null expression handle");
  const ExprProgram& pr = h->prog;
  if (ncols != pr.n_cols) bad_arg("%zu columns, the program was created with %u", ncols, pr.n_cols);
  if (nchal != pr.n_chal) bad_arg("%zu challenges, the program was created with %u", nchal, pr.n_chal);
  for (size_t j = 0; j < ncols && len; j++)
    if (out == cols[j] && lens[j] == len && (pr.used_cols >> j & 1) && !(pr.rot0_only >> j & 1))
      bad_arg("the output is column %zu, which the program reads at a rotation other than 0", j);
  if (len == 0) return;
  mi355_msm_domain* d = h->d;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  size_t total = len;
  for (size_t j = 0; j < ncols; j++) total += lens[j];
  // the arguments of this run: the column references, then the challenges
  const size_t nrefs = pr.refs.size(), ref_bytes = (nrefs * sizeof(ExprColRef) + 15) & ~(size_t)15;
  std::vector<uint8_t> img(ref_bytes + nchal * 32);
  poly_timed(d, on, [&] {
    FrStage g(h->stage, device_ptrs, on, total);
    std::vector<const uint32_t*> base(ncols);
    for (size_t j = 0; j < ncols; j++) base[j] = g.in(cols[j], lens[j]);
    uint32_t* dst = g.out(out, len);
    ExprColRef* refs = (ExprColRef*)img.data();
    for (size_t k = 0; k < nrefs; k++) refs[k] = ExprColRef{base[pr.refs[k].first], (uint32_t)lens[pr.refs[k].first], expr_shift(pr.refs[k].second, rot_step, len)};
    with_fr(d->curve, [&]<class FR>() {
      for (size_t k = 0; k < nchal; k++) expr_operand_words<FR>((uint32_t*)(img.data() + ref_bytes) + k * 8, (const uint8_t*)challenges + k * 32, normal);
    });
    h->args.reserve(img.size() ? img.size() : 16);
    if (!img.empty()) HIP_OK(hipMemcpyAsync(h->args.p, img.data(), img.size(), hipMemcpyHostToDevice, on));
    ExprRun p{};
    p.prog = h->code.as<uint32_t>();
    p.consts = p.prog + pr.code.size();
    p.refs = (const ExprColRef*)h->args.p;
    p.chals = (const uint32_t*)((const uint8_t*)h->args.p + ref_bytes);
    p.out = dst;
    p.ninstr = pr.ninstr();
    p.len = (uint32_t)len;
    p.normal = normal ? 1u : 0u;
    with_fr(d->curve, [&]<class FR>() { HIP_OK(LaunchExpr<FR>::rows(p, pr.slots, on)); });
    g.back(out, dst, len);
  });
}

}  // namespace

extern "C" {

RustError mi355_msm_expr_create(mi355_msm_expr** out, mi355_msm_domain* d, const uint32_t* nodes, size_t n_nodes, const void* consts, size_t n_consts,
                                size_t n_chal, size_t n_cols, unsigned flags) {
  return guarded_dev([&] { expr_create(out, d, nodes, n_nodes, consts, n_consts, n_chal, n_cols, flags); });
}

RustError mi355_msm_expr_run(mi355_msm_expr* e, void* out, const void* const* cols, const size_t* lens, size_t ncols, size_t len, size_t rot_step,
                             const void* challenges, size_t nchal, unsigned flags, void* stream) {
  return guarded_dev([&] { expr_run(e, out, cols, lens, ncols, len, rot_step, challenges, nchal, flags, (hipStream_t)stream); });
}

RustError mi355_msm_expr_query(mi355_msm_expr* e, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!key || !value) bad_arg("null argument");
    const std::string k(key);
    if (!e) bad_arg("null expression handle");
    const ExprProgram& pr = e->prog;
    if (k == "nodes") *value = pr.n_nodes;
    else if (k == "instructions") *value = pr.ninstr();
    else if (k == "slots") *value = pr.slots;
    else if (k == "products") *value = pr.products;
    else if (k == "reduces") *value = pr.reduces;
    else if (k == "columns") *value = pr.n_cols;
    else if (k == "lds_bytes") *value = expr_lds_bytes(pr.slots);
    else if (k == "last_us") *value = e->d->last_us;
    else if (k == "last_device_us") *value = e->d->last_device_us;
    else bad_arg("unknown expression query '%s'", key);
  });
}

RustError mi355_msm_expr_destroy(mi355_msm_expr* e) {
  return guarded_dev([&] {
    if (!e) return;
    (void)hipSetDevice(e->d->device);
    expr_release(e);
    delete e;
  });
}

}  // extern "C"
