// scan.hpp -- prefix scans along a vector of the scalar fields (the running product, the running sum) and the Plonk permutation
// grand product built on them, on the arithmetic of fr.hpp and the tiled scheme of poly.hpp.
//
// Reference behaviour: the grand product z[0] = 1, z[j + 1] = z[j] * prod_i (w_i[j] + beta k_i omega^j + gamma) /
// prod_i (w_i[j] + beta sigma_i[j] + gamma) of a Plonk prover's second round (one batch inversion of the denominators, then a serial
// loop).  Zeros are NOT skipped by the product scan: after a zero input every later product is zero.  A zero denominator is left zero
// by the batch inversion (poly.hpp), so that row's factor is zero and so is everything after it.
//
// The scheme is that of the division by X - z.  A block takes a tile of T = 2^tile_log consecutive elements through LDS (coalesced
// loads, converted to class M); lane l owns the POLY_RUN = 4 neighbours 4l .. 4l + 3.  Levels are separate launches on one stream: no
// block waits on another, nothing is polled and nothing is atomic -- field arithmetic is exact, so every order gives the same bytes.
//
//   way up     one total per tile: the lane's run (3 steps), then a tree over the lanes.  What lies past n is the identity.
//   recursion  the vector of tile totals is scanned by the same two kernels (exclusive): the carry that enters each tile.
//   way down   each tile is read again; the lane forms the prefixes of its run (3 steps), a Hillis-Steele prefix scan runs over the
//              lane totals, the lane's offset is (the carry into the tile) o (the scan value of the lane to the left), and the tile is
//              stored in the form of the call: offset o prefix, shifted by one element inside the lane for the exclusive scan.  A tile
//              only writes its own elements, so out == in is safe.  The top level has one tile; its last scan value is the total.
//
// The combine step `o` is a template parameter: the product (identity 1) or the sum (identity 0).
//
// Lazy bounds (tools/limb_bounds_fr.py --scan; the host build runs every step under MSM_CHECK).  Products stay in class M.  A sum step
// is a limb-wise add and one carry pass; a lane's run of four class-M elements stays below 8r, and every tree or scan step doubles the
// bound, so every second step (the odd ones) ends with one product by 1, which brings the value back below 2r: no value exceeds 32r
// before a reduction, 16r between two steps and 26r where an offset meets a prefix, R / r = 70.6 for BLS12-381.  The factors of the permutation product,
// w + beta id + gamma and w + beta sigma + gamma, are two class-M values and one canonical one: below 5r with limbs below 3 * 2^29,
// which fr_mul takes as its first operand without a carry pass.
#pragma once
#include "poly.hpp"

namespace msm {

constexpr unsigned kScanProduct = 0, kScanSum = 1;                    // op
constexpr unsigned kScanNormal = 1u, kScanInclusive = 2u;             // the flags of a call
constexpr uint32_t SCAN_MAX_COLUMNS = 8;

// the vector a scan launch reads: a PolyTile and, at level 0 of the permutation product, a second vector in the same ABI form that is
// multiplied in as the element is loaded (numerator times inverted denominator); NULL otherwise
struct ScanTile {
  PolyTile t;
  const uint32_t* mul;
};

struct ScanUp {
  ScanTile s;
  Fr* dst;                // one total per tile, class M
};

struct ScanDown {
  ScanTile s;
  uint32_t* dst;          // 8 words canonical in the ABI form (dst_internal == 0) or 9 words class M
  uint32_t dst_internal, inclusive;
  const Fr* carry;        // what enters tile t from the left, at position t; NULL at the top level
  Fr* total;              // the combination of all elements, class M: the top level only, else NULL
};

// one row per lane: the m-fold numerator and denominator of the permutation product
struct ScanPerm {
  const uint32_t *wires, *sigmas;   // m columns `stride` elements apart, the ABI form
  uint32_t *num, *den;              // 2^k elements each, the ABI form
  uint64_t stride;
  uint32_t k, m, normal;
  NttTable w;                       // the tables of omega
  Fr beta, gamma;                   // canonical
  Fr ks[SCAN_MAX_COLUMNS];          // canonical
};

struct ScanLane {
  Fr p[POLY_RUN];         // the prefixes of the lane's run
};

template <class FR, unsigned OP>
MSM_HD void scan_identity(Fr& x) {
  if constexpr (OP == kScanProduct) fr_set<FR>(x, FR::ONE); else fr_zero(x);
}

// r = a o b; the sum is carried
template <class FR, unsigned OP>
MSM_HD void scan_op(Fr& r, const Fr& a, const Fr& b) {
  if constexpr (OP == kScanProduct) {
    fr_mul<FR>(r, a, b);
  } else {
    fr_add(r, a, b);
    fr_carry(r);
  }
}

// after tree or scan step s: the sums come back to class M on every odd step
template <class FR, unsigned OP>
MSM_HD void scan_relax(Fr& a, uint32_t s) {
  if constexpr (OP == kScanSum) {
    if (s & 1) poly_store_m<FR>(&a, a);
  }
}

// a value of the scan -> class M, as limbs
template <class FR, unsigned OP>
MSM_HD void scan_store_m(Fr* dst, const Fr& x) {
  if constexpr (OP == kScanProduct) *dst = x; else poly_store_m<FR>(dst, x);
}

template <class FR, unsigned OP>
MSM_HD void scan_load(Fr& x, const ScanTile& s, uint64_t idx) {
  if (idx >= s.t.n) {
    scan_identity<FR, OP>(x);
    return;
  }
  poly_load<FR>(x, s.t, idx);
  if (s.mul) {
    uint32_t w[8];
    Fr y;
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = s.mul[idx * 8 + q];
    fr_from_abi<FR>(y, w, s.t.normal != 0);
    fr_mul<FR>(x, x, y);
  }
}

// ---- the way up -------------------------------------------------------------------------------------------------------------------

template <class FR, unsigned OP>
MSM_HD void scan_up_lane(Fr* lds, uint32_t l) {
  Fr acc = lds[POLY_RUN * l];
#pragma unroll
  for (int j = 1; j < (int)POLY_RUN; j++) scan_op<FR, OP>(acc, acc, lds[POLY_RUN * l + j]);
  lds[POLY_RUN * l] = acc;
}

// level s of the tree, pair j: v[l] = v[l] o v[l + 2^s], l = j 2^(s + 1)
template <class FR, unsigned OP>
MSM_HD void scan_up_tree(Fr* lds, uint32_t s, uint32_t j) {
  const uint32_t l = j << (s + 1);
  Fr a = lds[POLY_RUN * l];
  scan_op<FR, OP>(a, a, lds[POLY_RUN * (l + (1u << s))]);
  scan_relax<FR, OP>(a, s);
  lds[POLY_RUN * l] = a;
}

// ---- the way down -----------------------------------------------------------------------------------------------------------------

// lane l: the prefixes of its run; sc[l] = the run's total
template <class FR, unsigned OP>
MSM_HD void scan_down_lane(ScanLane& st, const Fr* lds, Fr* sc, uint32_t l) {
  Fr acc = lds[POLY_RUN * l];
  st.p[0] = acc;
#pragma unroll
  for (int j = 1; j < (int)POLY_RUN; j++) {
    scan_op<FR, OP>(acc, acc, lds[POLY_RUN * l + j]);
    st.p[j] = acc;
  }
  sc[l] = acc;
}

// step s of the prefix scan: the new sc[l] (written after a barrier)
template <class FR, unsigned OP>
MSM_HD void scan_down_step(Fr& nv, const Fr* sc, uint32_t s, uint32_t l) {
  nv = sc[l];
  if (l >= (1u << s)) scan_op<FR, OP>(nv, sc[l - (1u << s)], nv);
  scan_relax<FR, OP>(nv, s);
}

// lane l: offset = (the carry into the tile) o (the lanes to the left); out = offset o prefix, back into the tile
template <class FR, unsigned OP>
MSM_HD void scan_down_finish(const ScanLane& st, Fr* lds, const Fr* sc, const ScanDown& p, uint64_t tile, uint32_t lanes, uint32_t l) {
  Fr off;
  if (p.carry) off = p.carry[tile]; else scan_identity<FR, OP>(off);
  if (l > 0) scan_op<FR, OP>(off, sc[l - 1], off);
  if (p.total && l + 1 == lanes) scan_store_m<FR, OP>(p.total, sc[l]);
  Fr prev = off;
#pragma unroll
  for (int j = 0; j < (int)POLY_RUN; j++) {
    Fr y = prev;
    if (p.inclusive || j + 1 < (int)POLY_RUN) scan_op<FR, OP>(y, off, st.p[j]);
    Fr o;
#pragma unroll
    for (int q = 0; q < FR_NL; q++) o.v[q] = p.inclusive ? y.v[q] : prev.v[q];
    lds[POLY_RUN * l + j] = o;
    prev = y;
  }
}

template <class FR, unsigned OP>
MSM_HD void scan_down_store(const Fr* lds, const ScanDown& p, uint64_t tile, uint32_t i) {
  const uint64_t g = (tile << p.s.t.tile_log) + i;
  if (g >= p.s.t.n) return;
  if (p.dst_internal) {
    scan_store_m<FR, OP>((Fr*)p.dst + g, lds[i]);
    return;
  }
  uint32_t w[8];
  fr_to_abi<FR>(w, lds[i], p.s.t.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[g * 8 + q] = w[q];
}

// ---- the permutation product's rows -------------------------------------------------------------------------------------------------

// row j: num = prod_i (w_i + beta k_i omega^j + gamma), den = prod_i (w_i + beta sigma_i + gamma); the column loop stays rolled
template <class FR>
MSM_HD void scan_perm_row(const ScanPerm& p, uint32_t j) {
  const uint32_t h = ntt_lo_log(p.k);
  Fr bw = p.w.lo[j & ((1u << h) - 1)], num, den;
  fr_mul<FR>(bw, bw, p.w.hi[j >> h]);
  fr_mul<FR>(bw, bw, p.beta);
  fr_set<FR>(num, FR::ONE);
  den = num;
#pragma unroll 1
  for (uint32_t i = 0; i < p.m; i++) {
    uint32_t w[8];
    Fr wv, sg, t;
    const uint64_t at = (i * p.stride + j) * 8;
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.wires[at + q];
    fr_from_abi<FR>(wv, w, p.normal != 0);
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.sigmas[at + q];
    fr_from_abi<FR>(sg, w, p.normal != 0);
    fr_add(wv, wv, p.gamma);
    fr_mul<FR>(t, bw, p.ks[i]);
    fr_add(t, t, wv);
    fr_mul<FR>(num, t, num);
    fr_mul<FR>(t, sg, p.beta);
    fr_add(t, t, wv);
    fr_mul<FR>(den, t, den);
  }
  uint32_t o[8];
  fr_to_abi<FR>(o, num, p.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.num[(size_t)j * 8 + q] = o[q];
  fr_to_abi<FR>(o, den, p.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.den[(size_t)j * 8 + q] = o[q];
}

// ---- the chain of launches, shared by the engine (launchers on a stream) and the host build (loops) -------------------------------

// elements of work memory a scan of n elements needs: per level above the first the totals and the carries, and the total
MSM_HD uint64_t scan_work_elems(uint64_t n, uint32_t tile_log) { return poly_work_elems(n, tile_log); }

// dst[i] = the scan of src (times mul, element by element, when mul is given) in the ABI form; dst == src is allowed; n >= 1.  Returns
// the combination of all n elements as one class-M element in work memory.  RUN has up(ScanUp) and down(ScanDown).
template <class FR, unsigned OP, class RUN>
const Fr* scan_chain(RUN& run, uint32_t* dst, const uint32_t* src, const uint32_t* mul, uint64_t n, bool normal, bool inclusive, uint32_t tile_log,
                     Fr* work) {
  uint64_t len[POLY_MAX_LEVELS + 1];
  const uint32_t levels = poly_plan(n, tile_log, len);
  Fr* part[POLY_MAX_LEVELS + 1];   // part[j]: the totals of the tiles of level j - 1 (the vector of level j); part[j] + len[j]: the carries into level j - 1
  Fr* at = work + 2;
  for (uint32_t j = 1; j < levels; j++) {
    part[j] = at;
    at += 2 * len[j];
  }
  const ScanTile first{PolyTile{src, n, tile_log, 0, normal ? 1u : 0u}, mul};
  for (uint32_t j = 0; j + 1 < levels; j++) {
    ScanUp u;
    u.s = j == 0 ? first : ScanTile{PolyTile{(const uint32_t*)part[j], len[j], tile_log, 1, 0}, nullptr};
    u.dst = part[j + 1];
    run.template up<OP>(u);
  }
  for (uint32_t j = levels; j-- > 0;) {
    ScanDown d;
    d.s = j == 0 ? first : ScanTile{PolyTile{(const uint32_t*)part[j], len[j], tile_log, 1, 0}, nullptr};
    d.dst = j == 0 ? dst : (uint32_t*)(part[j] + len[j]);
    d.dst_internal = j != 0;
    d.inclusive = j == 0 && inclusive;
    d.carry = j + 1 < levels ? part[j + 1] + len[j + 1] : nullptr;
    d.total = j + 1 == levels ? work : nullptr;
    run.template down<OP>(d);
  }
  return work;
}

#if defined(__HIPCC__)
// (every thread of a block reaches every barrier: the lanes of a small tile are the first threads, the others only load and store)

template <class FR, unsigned OP>
__global__ void __launch_bounds__(POLY_THREADS) k_scan_up(ScanUp p) {
  __shared__ Fr lds[POLY_MAX_TILE];
  const uint32_t T = 1u << p.s.t.tile_log, lanes = poly_lanes(p.s.t.tile_log);
  const uint64_t base = (uint64_t)blockIdx.x << p.s.t.tile_log;
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS) scan_load<FR, OP>(lds[i], p.s, base + i);
  __syncthreads();
  if (threadIdx.x < lanes) scan_up_lane<FR, OP>(lds, threadIdx.x);
#pragma unroll 1
  for (uint32_t s = 0; (2u << s) <= lanes; s++) {
    __syncthreads();
    if (threadIdx.x < (lanes >> (s + 1))) scan_up_tree<FR, OP>(lds, s, threadIdx.x);
  }
  if (threadIdx.x == 0) scan_store_m<FR, OP>(p.dst + blockIdx.x, lds[0]);
}

template <class FR, unsigned OP>
__global__ void __launch_bounds__(POLY_THREADS) k_scan_down(ScanDown p) {
  __shared__ Fr lds[POLY_MAX_TILE];
  __shared__ Fr sc[POLY_MAX_LANES];
  const uint32_t T = 1u << p.s.t.tile_log, lanes = poly_lanes(p.s.t.tile_log), l = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x << p.s.t.tile_log;
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS) scan_load<FR, OP>(lds[i], p.s, base + i);
  __syncthreads();
  ScanLane st;
  if (l < lanes) scan_down_lane<FR, OP>(st, lds, sc, l);
#pragma unroll 1
  for (uint32_t s = 0; (1u << s) < lanes; s++) {
    __syncthreads();
    Fr nv;
    if (l < lanes) scan_down_step<FR, OP>(nv, sc, s, l);
    __syncthreads();
    if (l < lanes) sc[l] = nv;
  }
  __syncthreads();
  if (l < lanes) scan_down_finish<FR, OP>(st, lds, sc, p, blockIdx.x, lanes, l);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS) scan_down_store<FR, OP>(lds, p, blockIdx.x, i);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_scan_perm(ScanPerm p) {
  const uint32_t j = blockIdx.x * POLY_THREADS + threadIdx.x;
  if ((j >> p.k) == 0) scan_perm_row<FR>(p, j);
}
#endif

}  // namespace msm
