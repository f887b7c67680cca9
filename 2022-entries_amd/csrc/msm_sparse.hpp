// msm_sparse.hpp -- resident sparse matrices over Fr and y = M z (included by msm_engine.hip after msm_quot.hpp): the C ABI
// mi355_msm_sparse_{create, apply, query, destroy} of include/mi355_msm.h over the kernels of sparse.hpp.
//
// A matrix belongs to a domain handle: the field, the device, the stream of its host-pointer calls and the work memory of the sum scan
// (`scan`) are the domain's.  Everything else -- the coefficients, the column indices, the row lists, the class-M copy of z, the lane
// totals and the sums at the lane boundaries, the staged vectors of a host-pointer call -- is the matrix's own (query "work_bytes"), so
// two matrices on one domain do not disturb each other; apply stages through `stage` with the FrStage of fr_stage.hpp.  Every call
// judges its arguments first, the handle last.
#pragma once

#include "launch_sparse.hpp"

struct mi355_msm_sparse {
  mi355_msm_domain* d = nullptr;
  SparseMat m{};
  DevBuf vals, idx, work, stage;   // the coefficients; the column indices and the row lists; what one apply needs; staged z and out
};

namespace {

constexpr size_t kSparseMaxDim = (size_t)1 << SPARSE_MAX_DIM_LOG;
constexpr uint64_t kSparseMaxNnz = (uint64_t)1 << SPARSE_MAX_NNZ_LOG;

template <class FR>
struct SparseEngineRun {
  mi355_msm_domain* d;
  hipStream_t st;
  void z(const SparseZ& p) { HIP_OK(LaunchSparse<FR>::z(p, st)); }
  void totals(const SparseRun& p) { HIP_OK(LaunchSparse<FR>::totals(p, st)); }
  void rows(const SparseRun& p) { HIP_OK(LaunchSparse<FR>::rows(p, st)); }
  void cross(const SparseRun& p) { HIP_OK(LaunchSparse<FR>::cross(p, st)); }
  void scan(uint32_t* v, uint64_t n) {
    d->scan.reserve((size_t)scan_work_elems(n, d->poly_tile_log) * sizeof(Fr));
    ScanRun<FR> run{st};
    scan_chain<FR, kScanSum>(run, v, v, nullptr, n, false, false, d->poly_tile_log, d->scan.as<Fr>());
  }
};

void sparse_create(mi355_msm_sparse** out, mi355_msm_domain* d, size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx,
                   const void* values, unsigned flags) {
  if (out) *out = nullptr;
  if (flags & ~kSparseNormal) bad_arg("unknown flag bits 0x%x (bit 0: the values are plain integers)", flags);
  if (rows > kSparseMaxDim) bad_arg("%zu rows exceed 2^30", rows);
  if (cols > kSparseMaxDim) bad_arg("%zu columns exceed 2^30", cols);
  if (!out || !row_ptr) bad_arg("null handle out-pointer or row_ptr");
  if ((uintptr_t)row_ptr & 7) bad_arg("row_ptr must be 8-byte aligned");
  const uint64_t nnz = row_ptr[rows];
  if (nnz > kSparseMaxNnz) bad_arg("%llu entries (row_ptr[rows]) exceed 2^31", (unsigned long long)nnz);
  if (nnz && (!col_idx || !values)) bad_arg("null col_idx or values pointer");
  if ((uintptr_t)col_idx & 3) bad_arg("col_idx must be 4-byte aligned");
  char why[256];
  if (!sparse_validate(rows, cols, row_ptr, col_idx, why, sizeof why)) bad_arg("%s", why);
  if (!d) bad_arg("null domain handle");
  SparsePlan pl;
  sparse_plan(pl, rows, row_ptr, col_idx);
  HIP_OK(hipSetDevice(d->device));
  std::unique_ptr<mi355_msm_sparse> m(new mi355_msm_sparse());
  const hipStream_t st = d->own_stream;
  try {
    m->d = d;
    // the index lists in one buffer: col, ne_end, ne_row, lane_row, row_ptr
    const size_t counts[5] = {pl.slots, pl.nne, pl.nne, pl.nlanes, rows + 1};
    const std::vector<uint32_t>* lists[5] = {&pl.col, &pl.ne_end, &pl.ne_row, &pl.lane_row, &pl.row_ptr};
    size_t total = 0;
    for (size_t c : counts) total += c;
    m->idx.reserve(total * 4 + 16);
    m->vals.reserve((size_t)pl.slots * 32 + 32);
    m->work.reserve((size_t)sparse_work_bytes(cols, pl.nlanes));
    const uint32_t* at[5];
    size_t off = 0;
    for (int i = 0; i < 5; i++) {
      at[i] = m->idx.as<uint32_t>() + off;
      if (counts[i]) HIP_OK(hipMemcpyAsync((void*)at[i], lists[i]->data(), counts[i] * 4, hipMemcpyHostToDevice, st));
      off += counts[i];
    }
    m->m = SparseMat{m->vals.as<uint32_t>(), at[0], at[1], at[2], at[3], at[4], (uint32_t)rows, (uint32_t)cols, pl.nnz, pl.nne, pl.nlanes, pl.slots};
    ScratchBuf raw(st);
    if (pl.nnz) {
      raw.reserve((size_t)pl.nnz * 32);
      HIP_OK(hipMemcpyAsync(raw.p, values, (size_t)pl.nnz * 32, hipMemcpyHostToDevice, st));
      const SparseVals p{raw.as<uint32_t>(), m->vals.as<uint32_t>(), pl.nnz, pl.slots, (flags & kSparseNormal) ? 1u : 0u};
      with_fr(d->curve, [&]<class FR>() { HIP_OK(LaunchSparse<FR>::vals(p, st)); });
    }
    HIP_OK(hipStreamSynchronize(st));
  } catch (...) {
    (void)hipStreamSynchronize(st);   // (the copies of the index lists may be in flight)
    for (DevBuf* b : {&m->vals, &m->idx, &m->work, &m->stage}) b->release();
    throw;
  }
  *out = m.release();
}

void sparse_apply(mi355_msm_sparse* m, void* out, const void* z, unsigned flags, hipStream_t st) {
  if (flags & ~(kSparseNormal | kSparseDevice)) bad_arg("unknown flag bits 0x%x (bit 0: normal-form elements, bit 1: device pointers)", flags);
  const bool device_ptrs = (flags & kSparseDevice) != 0, normal = (flags & kSparseNormal) != 0;
  if (m ? ((m->m.rows && !out) || (m->m.cols && !z)) : (!out || !z)) bad_arg("null input or output pointer");
  poly_check_aligned(device_ptrs, {out, z});
  poly_check_stream(device_ptrs, st);
  if (out && out == z) bad_arg("the output overlaps z");
  if (!m) bad_arg("null matrix handle");
  if (poly_overlap(out, m->m.rows, z, m->m.cols)) bad_arg("the output overlaps z");
  mi355_msm_domain* d = m->d;
  if (m->m.rows == 0) return;
  const hipStream_t on = device_ptrs ? st : d->own_stream;
  poly_timed(d, on, [&] {
    FrStage g(m->stage, device_ptrs, on, (size_t)m->m.cols + m->m.rows);
    const uint32_t* src = g.in(z, m->m.cols);
    uint32_t* dst = g.out(out, m->m.rows);
    with_fr(d->curve, [&]<class FR>() {
      SparseEngineRun<FR> run{d, on};
      sparse_chain<FR>(run, m->m, dst, src, normal, m->work.p);
    });
    g.back(out, dst, m->m.rows);
  });
}

}  // namespace

extern "C" {

RustError mi355_msm_sparse_create(mi355_msm_sparse** out, mi355_msm_domain* d, size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx,
                                  const void* values, unsigned flags) {
  return guarded_dev([&] { sparse_create(out, d, rows, cols, row_ptr, col_idx, values, flags); });
}

RustError mi355_msm_sparse_apply(mi355_msm_sparse* m, void* out, const void* z, unsigned flags, void* stream) {
  return guarded_dev([&] { sparse_apply(m, out, z, flags, (hipStream_t)stream); });
}

RustError mi355_msm_sparse_query(mi355_msm_sparse* m, const char* key, uint64_t* value) {
  return guarded([&] {
    if (!key || !value) bad_arg("null argument");
    const std::string k(key);
    // the constants of the kernels need no matrix
    if (k == "entries_per_lane") { *value = SPARSE_E; return; }
    if (k == "block_lanes") { *value = SPARSE_LANES; return; }
    if (!m) bad_arg("null matrix handle");
    if (k == "rows") *value = m->m.rows;
    else if (k == "cols") *value = m->m.cols;
    else if (k == "nnz") *value = m->m.nnz;
    else if (k == "work_bytes") *value = m->vals.bytes + m->idx.bytes + m->work.bytes + m->stage.bytes;
    else bad_arg("unknown matrix query '%s'", key);
  });
}

RustError mi355_msm_sparse_destroy(mi355_msm_sparse* m) {
  return guarded_dev([&] {
    if (!m) return;
    (void)hipSetDevice(m->d->device);
    for (DevBuf* b : {&m->vals, &m->idx, &m->work, &m->stage}) b->release();
    delete m;
  });
}

}  // extern "C"
