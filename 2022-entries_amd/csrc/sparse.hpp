// sparse.hpp -- a resident sparse matrix over the scalar fields and y = M z, on the arithmetic of fr.hpp and the sum scan of scan.hpp:
// the products <A_i, z>, <B_i, z> of the rows of the R1CS matrices with the full assignment that open a Groth16 or Marlin prover.
//
// Reference behaviour: ark-groth16's evaluate_constraint (the sum over the (coefficient, index) pairs of a row of arkworks' Matrix<F>)
// inside LibsnarkReduction::witness_map.  Duplicate columns in a row are summed, zero coefficients and empty rows are allowed.
//
// R1CS rows are badly skewed (most hold 1 - 3 entries, a few hold thousands), so nothing here is per row: lane t owns the
// E = SPARSE_E consecutive entries t E .. t E + E - 1 of the CSR arrays, whatever rows they belong to, and does the same work for each.
// Sums in Fr are exact, so a running sum over ALL entries, cut at the row boundaries, is a legitimate way to sum the segments.
//
// What create leaves on the device.  The coefficients as canonical Montgomery values packed in 32 bytes (a class-M value is below
// 2^256; the nine limbs come back by shifts), so apply converts none of them; they and the column indices in a lane-interleaved order --
// entry e of lane l of block b at slot (b E + e) L + l, L = SPARSE_LANES -- so that the 256 lanes of a block read 256 neighbours in
// every iteration although each walks its own E consecutive entries; slots past nnz hold coefficient 0 and column 0.  The non-empty
// rows as two lists (where each ends, which row it is), and per lane the index into those lists of the row that is open at the lane's
// first entry, so no lane searches row_ptr and an empty row costs a lane nothing.  row_ptr itself, for the last launch.
//
// Five launches on one stream; no block waits on another, nothing is atomic or polled, loads and stores are ordinary vector ones.
//   k_sparse_z       one lane per column: z in the form of the call -> class M, packed in 32 bytes (cols conversions, not nnz).
//   k_sparse_totals  lane t: the sum of its E products, stored as one canonical arkworks image.
//   the sum scan     scan.hpp's exclusive prefix sum over the ceil(nnz / E) lane totals, in place: S_t, the sum of all entries before
//                    lane t.
//   k_sparse_rows    lane t walks its entries again (a second product is cheaper than 72 bytes of traffic per entry) with two
//                    accumulators: `run` starts from S_t, `loc` from 0 at every row start.  A row that begins and ends inside the
//                    lane is written from `loc` alone.  A row that began in an earlier lane and ends here leaves `run` in bend[t]; a
//                    row that begins here (also at the lane's first entry) and ends in a later lane leaves `run` at its start in
//                    bstart[t].  At most one row of each kind exists per lane.
//   k_sparse_cross   one lane per row: an empty row is written as 0; a row whose first and last entry lie in different lanes ts, te
//                    is bend[te] - bstart[ts]; the others were written by k_sparse_rows.
//
// Lazy bounds (tools/limb_bounds_fr.py --sparse; the host build runs every step under MSM_CHECK).  A product is class M (normalised
// limbs, value < 2r).  An accumulator adds one product and runs one carry pass per entry: `loc` stays below 2 E r = 32r, `run` starts
// from a class-M prefix and stays below 34r, R / r = 70.6 for BLS12-381; both only ever meet a canonical constant (the conversion on
// the way out, the product by 1 into bstart / bend).  bend - bstart + 4r is below 6r.
#pragma once
#include <cstdio>
#include <vector>

#include "scan.hpp"

namespace msm {

constexpr unsigned kSparseNormal = 1u, kSparseDevice = 2u;             // the flags of a call: plain integers; device pointers
constexpr uint32_t SPARSE_E = 16;                                      // entries per lane
constexpr uint32_t SPARSE_LANES = POLY_THREADS;                        // lanes per block
constexpr uint32_t SPARSE_BLOCK = SPARSE_E * SPARSE_LANES;             // entries per block
constexpr uint32_t SPARSE_MAX_DIM_LOG = 30, SPARSE_MAX_NNZ_LOG = 31;
constexpr uint32_t SPARSE_NO_END = 0xffffffffu;                        // the end of the row after the last one

// the matrix on the device
struct SparseMat {
  const uint32_t* vals;       // `slots` coefficients, 8 words each: canonical, packed, lane-interleaved
  const uint32_t* col;        // `slots` column indices, lane-interleaved
  const uint32_t* ne_end;     // per non-empty row: one past its last entry
  const uint32_t* ne_row;     // per non-empty row: its index
  const uint32_t* lane_row;   // per lane: the non-empty row (an index into ne_*) that holds the lane's first entry
  const uint32_t* row_ptr;    // rows + 1
  uint32_t rows, cols, nnz, nne, nlanes, slots;
};

// create: raw coefficients in CSR order -> vals
struct SparseVals {
  const uint32_t* raw;
  uint32_t* vals;
  uint32_t nnz, slots, normal;
};

struct SparseZ {
  const uint32_t* z;          // the form of the call
  uint32_t* zm;               // class M, packed
  uint32_t cols;
  Fr cin;
};

struct SparseRun {
  SparseMat m;
  const uint32_t* zm;
  uint32_t* totals;           // nlanes arkworks images: the lane totals, then (the scan runs in place) the prefixes S_t
  Fr *bstart, *bend;          // nlanes each, class M
  uint32_t* out;              // the form of the call
  Fr cout;
};

// the slot of entry k
MSM_HD uint32_t sparse_slot(uint32_t k) {
  const uint32_t t = k / SPARSE_E, e = k % SPARSE_E;
  return (t / SPARSE_LANES) * SPARSE_BLOCK + e * SPARSE_LANES + (t % SPARSE_LANES);
}

// the first slot of lane t; entry e of the lane lies e * SPARSE_LANES further
MSM_HD uint32_t sparse_lane_slot(uint32_t t) { return (t / SPARSE_LANES) * SPARSE_BLOCK + (t % SPARSE_LANES); }

template <class FR>
MSM_HD void sparse_store(uint32_t* dst, uint64_t idx, const Fr& a, const Fr& cout) {
  Fr x;
  uint32_t o[8];
  fr_mul<FR>(x, a, cout);
  fr_pack(o, x);
  fr_canon<FR>(o);
#pragma unroll
  for (int q = 0; q < 8; q++) dst[idx * 8 + q] = o[q];
}

// create, one lane per slot
template <class FR>
MSM_HD void sparse_val_slot(const SparseVals& p, uint32_t slot) {
  const uint32_t rem = slot % SPARSE_BLOCK;
  const uint64_t k = ((uint64_t)(slot / SPARSE_BLOCK) * SPARSE_LANES + rem % SPARSE_LANES) * SPARSE_E + rem / SPARSE_LANES;
  uint32_t o[8];
#pragma unroll
  for (int q = 0; q < 8; q++) o[q] = 0;
  if (k < p.nnz) {
    uint32_t w[8];
    Fr x;
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.raw[k * 8 + q];
    fr_from_abi<FR>(x, w, p.normal != 0);
    fr_pack(o, x);
    fr_canon<FR>(o);
  }
#pragma unroll
  for (int q = 0; q < 8; q++) p.vals[(uint64_t)slot * 8 + q] = o[q];
}

// step 1, one lane per column
template <class FR>
MSM_HD void sparse_z_elem(const SparseZ& p, uint32_t i) {
  Fr x;
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = p.z[(uint64_t)i * 8 + q];
  fr_unpack(x, w);
  fr_mul<FR>(x, x, p.cin);
  fr_pack(w, x);
#pragma unroll
  for (int q = 0; q < 8; q++) p.zm[(uint64_t)i * 8 + q] = w[q];
}

// a packed record of 32 bytes (in a 32-byte aligned buffer: none straddles a 64-byte sector) -> normalised limbs
MSM_HD void sparse_load32(Fr& x, const uint32_t* src, uint64_t idx) {
  const uint32_t* s = (const uint32_t*)__builtin_assume_aligned(src, 16) + idx * 8;
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = s[q];
  fr_unpack(x, w);
}

// coefficient times z[column] of one slot, class M
template <class FR>
MSM_HD void sparse_product(Fr& x, const SparseMat& m, const uint32_t* zm, uint32_t slot) {
  Fr v, zv;
  const uint32_t c = m.col[slot];
  sparse_load32(v, m.vals, slot);
  sparse_load32(zv, zm, c);
  fr_mul<FR>(x, zv, v);
}

// step 2, lane t: the entry loop stays rolled
template <class FR>
MSM_HD void sparse_total(const SparseRun& p, uint32_t t) {
  const uint32_t base = sparse_lane_slot(t);
  Fr acc;
  fr_zero(acc);
#pragma unroll 1
  for (uint32_t e = 0; e < SPARSE_E; e++) {
    Fr x;
    sparse_product<FR>(x, p.m, p.zm, base + e * SPARSE_LANES);
    fr_add(acc, acc, x);
    fr_carry(acc);
  }
  uint32_t o[8];
  fr_to_abi<FR>(o, acc, false);
#pragma unroll
  for (int q = 0; q < 8; q++) p.totals[(uint64_t)t * 8 + q] = o[q];
}

// step 4, lane t: the entry loop stays rolled
template <class FR>
MSM_HD void sparse_rows_lane(const SparseRun& p, uint32_t t) {
  const uint32_t k0 = t * SPARSE_E, base = sparse_lane_slot(t);
  Fr run, loc, bstart, bend;
  {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.totals[(uint64_t)t * 8 + q];
    fr_from_abi<FR>(run, w, false);
  }
  uint32_t j = p.m.lane_row[t];
  uint32_t end = p.m.ne_end[j];
  uint32_t open = j ? p.m.ne_end[j - 1] : 0;   // where the open row began: below k0 when it came in from an earlier lane
  bool ended = false;
  bstart = run;
  bend = run;
  fr_zero(loc);
#pragma unroll 1
  for (uint32_t e = 0; e < SPARSE_E; e++) {
    const uint32_t k = k0 + e;
    Fr x;
    sparse_product<FR>(x, p.m, p.zm, base + e * SPARSE_LANES);
    fr_add(run, run, x);
    fr_carry(run);
    fr_add(loc, loc, x);
    fr_carry(loc);
    if (k + 1 == end) {
      if (open >= k0) {
        sparse_store<FR>(p.out, p.m.ne_row[j], loc, p.cout);
      } else {
        bend = run;
        ended = true;
      }
      j++;
      end = j < p.m.nne ? p.m.ne_end[j] : SPARSE_NO_END;
      open = k + 1;
      bstart = run;
      fr_zero(loc);
    }
  }
  if (ended) poly_store_m<FR>(p.bend + t, bend);
  if (open >= k0 && open < k0 + SPARSE_E && j < p.m.nne && end > k0 + SPARSE_E) poly_store_m<FR>(p.bstart + t, bstart);
}

// the last launch, row r
template <class FR>
MSM_HD void sparse_cross_row(const SparseRun& p, uint32_t r) {
  const uint32_t s = p.m.row_ptr[r], e = p.m.row_ptr[r + 1];
  if (s == e) {
#pragma unroll
    for (int q = 0; q < 8; q++) p.out[(uint64_t)r * 8 + q] = 0;
    return;
  }
  const uint32_t ts = s / SPARSE_E, te = (e - 1) / SPARSE_E;
  if (ts == te) return;
  Fr x;
  fr_sub<FR>(x, p.bend[te], p.bstart[ts]);
  fr_carry(x);
  sparse_store<FR>(p.out, r, x, p.cout);
}

// ---- what create derives on the host --------------------------------------------------------------------------------------------------

// the structure of a CSR matrix: false with a message that names the first offending row
inline bool sparse_validate(size_t rows, size_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, char* msg, size_t msg_len) {
  if (row_ptr[0] != 0) {
    snprintf(msg, msg_len, "row 0: row_ptr[0] is %llu, not 0", (unsigned long long)row_ptr[0]);
    return false;
  }
  for (size_t r = 0; r < rows; r++)
    if (row_ptr[r + 1] < row_ptr[r]) {
      snprintf(msg, msg_len, "row %zu: row_ptr decreases from %llu to %llu", r, (unsigned long long)row_ptr[r], (unsigned long long)row_ptr[r + 1]);
      return false;
    }
  for (size_t r = 0; r < rows; r++)
    for (uint64_t k = row_ptr[r]; k < row_ptr[r + 1]; k++)
      if (col_idx[k] >= cols) {
        snprintf(msg, msg_len, "row %zu: column index %u at entry %llu is not below the %zu columns", r, col_idx[k], (unsigned long long)k, cols);
        return false;
      }
  return true;
}

struct SparsePlan {
  uint32_t nnz = 0, nne = 0, nlanes = 0, slots = 0;
  std::vector<uint32_t> col, ne_end, ne_row, lane_row, row_ptr;
};

// the lists of a validated matrix
inline void sparse_plan(SparsePlan& pl, size_t rows, const uint64_t* row_ptr, const uint32_t* col_idx) {
  pl.nnz = (uint32_t)row_ptr[rows];
  pl.nlanes = (uint32_t)(((uint64_t)pl.nnz + SPARSE_E - 1) / SPARSE_E);
  pl.slots = (uint32_t)(((uint64_t)pl.nlanes + SPARSE_LANES - 1) / SPARSE_LANES * SPARSE_BLOCK);
  pl.col.assign(pl.slots, 0);
  for (uint32_t k = 0; k < pl.nnz; k++) pl.col[sparse_slot(k)] = col_idx[k];
  pl.row_ptr.resize(rows + 1);
  pl.ne_end.clear();
  pl.ne_row.clear();
  for (size_t r = 0; r <= rows; r++) pl.row_ptr[r] = (uint32_t)row_ptr[r];
  for (size_t r = 0; r < rows; r++)
    if (row_ptr[r + 1] > row_ptr[r]) {
      pl.ne_end.push_back((uint32_t)row_ptr[r + 1]);
      pl.ne_row.push_back((uint32_t)r);
    }
  pl.nne = (uint32_t)pl.ne_end.size();
  pl.lane_row.resize(pl.nlanes);
  uint32_t j = 0;
  for (uint32_t t = 0; t < pl.nlanes; t++) {
    while (pl.ne_end[j] <= t * SPARSE_E) j++;
    pl.lane_row[t] = j;
  }
}

// bytes of work memory one apply needs beside the matrix: z in class M, the lane totals, bstart and bend
MSM_HD uint64_t sparse_work_bytes(uint64_t cols, uint64_t nlanes) { return ((cols + nlanes) * 32 + 2 * nlanes * sizeof(Fr) + 63) / 32 * 32; }

// The chain of launches of y = M z, shared by the engine (launchers on a stream) and the host build (loops).  RUN has z(SparseZ),
// totals(SparseRun), scan(uint32_t* v, uint64_t n) -- the exclusive prefix sum of n arkworks images in place --, rows(SparseRun) and
// cross(SparseRun).  `work`: sparse_work_bytes bytes, 32-byte aligned.
template <class FR, class RUN>
void sparse_chain(RUN& run, const SparseMat& m, uint32_t* out, const uint32_t* z, bool normal, void* work) {
  SparseZ zp{};
  SparseRun p{};
  uint32_t* zm = (uint32_t*)work;
  zp.z = z;
  zp.zm = zm;
  zp.cols = m.cols;
  fr_const<FR>(zp.cin, normal ? 1 : 0);
  p.m = m;
  p.zm = zm;
  p.totals = zm + (uint64_t)m.cols * 8;
  p.bstart = (Fr*)(p.totals + (uint64_t)m.nlanes * 8);
  p.bend = p.bstart + m.nlanes;
  p.out = out;
  fr_const<FR>(p.cout, normal ? 3 : 2);
  if (m.rows == 0) return;
  if (m.nlanes) {
    run.z(zp);
    run.totals(p);
    run.scan(p.totals, m.nlanes);
    run.rows(p);
  }
  run.cross(p);
}

#if defined(__HIPCC__)
template <class FR>
__global__ void __launch_bounds__(SPARSE_LANES) k_sparse_vals(SparseVals p) {
  const uint32_t i = blockIdx.x * SPARSE_LANES + threadIdx.x;
  if (i < p.slots) sparse_val_slot<FR>(p, i);
}

template <class FR>
__global__ void __launch_bounds__(SPARSE_LANES) k_sparse_z(SparseZ p) {
  const uint32_t i = blockIdx.x * SPARSE_LANES + threadIdx.x;
  if (i < p.cols) sparse_z_elem<FR>(p, i);
}

template <class FR>
__global__ void __launch_bounds__(SPARSE_LANES) k_sparse_totals(SparseRun p) {
  const uint32_t t = blockIdx.x * SPARSE_LANES + threadIdx.x;
  if (t < p.m.nlanes) sparse_total<FR>(p, t);
}

template <class FR>
__global__ void __launch_bounds__(SPARSE_LANES) k_sparse_rows(SparseRun p) {
  const uint32_t t = blockIdx.x * SPARSE_LANES + threadIdx.x;
  if (t < p.m.nlanes) sparse_rows_lane<FR>(p, t);
}

template <class FR>
__global__ void __launch_bounds__(SPARSE_LANES) k_sparse_cross(SparseRun p) {
  const uint32_t r = blockIdx.x * SPARSE_LANES + threadIdx.x;
  if (r < p.m.rows) sparse_cross_row<FR>(p, r);
}
#endif

}  // namespace msm
