// mle.hpp -- dense multilinear extensions over the scalar fields and the prover's side of the sumcheck protocol, on the arithmetic of
// fr.hpp: fixing variables of a table of 2^nv evaluations, the table of eq(x, point), and one prover round for
// g(x) = sum_j c_j prod_{k in S_j} f_k(x).
//
// Reference behaviour: ark-poly's DenseMultilinearExtension (poly/src/evaluations/multivariate/multilinear/dense.rs: fix_variables,
// evaluate) and the prover of ark-linear-sumcheck's ListOfProductsOfPolynomials.  Index b of a table is the point (b_0, .., b_{nv-1}),
// b_0 the lowest bit; variables are fixed from x_1 (the lowest bit) upward: out[b] = in[2b] + r (in[2b+1] - in[2b]).
//
// The form a product accepts.  fr_mul(a, b) takes a lazy first operand (limbs below 2^31, any value below R) and wants b normalised
// with r + a b / R below 2r.  Every product here is ordered so that the lazy value is the FIRST operand:
//   fixing a variable   out = (1 - r) x + r y: two products by canonical constants and one limb-wise sum, value below 4r, limbs below
//                       2^30 -- no subtraction, so no operand ever has to be brought back to class M between two levels.  On the
//                       first level of a pass that reads the caller's table the constants carry the conversion of the call as well
//                       ((1 - r) CIN, r CIN), so any 256-bit input goes straight into the product.
//   extrapolation       a pair (lo, hi) is converted to class M (one product each).  diff = hi - lo + 4r is carried once; e_0 = lo,
//                       e_1 = hi, e_t = e_{t-1} + diff with ONE carry pass after e_3: limbs stay below 3 * 2^29 + 24 and the value
//                       below 2r + 4 * 6r = 26r at t = 5.
//   a term              the running product starts as the canonical coefficient c_j and is always the SECOND operand:
//                       P <- fr_mul(e_t, P).  P is class M (normalised, below 2r), and r + 26r * 2r / R stays below 2r because
//                       R / r >= 70.6 (BLS12-381).  So only the factor is lazy, never the running product: a term of n factors costs
//                       n products per evaluation point, the coefficient included, and no conditional subtraction anywhere.
//   sums                a lane adds the class-M products of MLE_PTS = 4 points times at most 8 terms into one accumulator per
//                       evaluation point, one carry pass after each: below 64r < R.  One product by 1 brings the lane sum to class M;
//                       the block tree adds two neighbours per level with a carry pass and multiplies by 1 after its fourth level
//                       (2r -> 32r), so at most 32r reaches the last product by 1.
// tools/limb_bounds_fr.py --mle carries all of this out; the host build runs every step under MSM_CHECK.
//
// Where a lane keeps its values.  The term list is data, so nothing is indexed by it in registers: the kernel walks the terms and the
// factors of a term in rolled loops and keeps, with static indices only, D + 1 accumulators, D + 1 running products (D the largest
// factor count, a template parameter: five kernels per field) and the one pair (lo, diff) of the factor at hand, which it loads from
// the table when it meets it.  A table that stands in several terms is loaded and converted once per occurrence (from L2 after the
// first); no LDS is spent on pairs, so the only LDS is the 256 elements of the block tree.
//
// The fused round.  With r_prev the lane first folds its points of every table (four inputs -> two outputs per point and table, 128
// contiguous bytes in, 64 out) and writes the canonical folded tables; then it runs the plain round on what it wrote -- every lane
// reads back only its own stores, which are still in the cache.  One read of every input, one write of half of it, one launch.
//
// Reductions: lane sums, the block tree through LDS, one class-M partial per block and evaluation point; then k_mle_sum reduces the
// partial vectors tile by tile in further launches until one row is left.  Sums in Fr are exact, nothing is atomic, no block waits on
// another.
#pragma once
#include <vector>

#include "poly.hpp"

namespace msm {

constexpr unsigned kMleNormal = 1u, kMleDevice = 2u;   // the flags of a call: plain integers; device pointers
constexpr uint32_t MLE_MAX_VARS = 30;
constexpr uint32_t MLE_MAX_TABLES = 12, MLE_MAX_TERMS = 8, MLE_MAX_FACTORS = 5;
constexpr uint32_t MLE_EVALS = MLE_MAX_FACTORS + 1;    // the row of partial sums a block leaves
constexpr uint32_t MLE_PTS = POLY_RUN;                 // the points of a round a lane sums
constexpr uint32_t MLE_TREE_REDUCE = 4;                // the block tree multiplies by 1 after this many levels
constexpr uint32_t MLE_THREADS = POLY_THREADS;

// one pass of fix_variables: a block reads 2^tile_log elements and fixes kk <= tile_log variables
struct MleFix {
  const uint32_t* src;
  uint32_t* dst;
  uint64_t n;                          // elements read, a power of two >= 2^tile_log
  uint32_t tile_log, kk;
  uint32_t src_internal, dst_internal;   // lazy limbs (value below 4r) of work memory rather than the 32 bytes of the call
  Fr a[POLY_TILE_LOG_MAX], b[POLY_TILE_LOG_MAX];   // level s: a[s] x + b[s] y, canonical; level 0 of the caller's table times CIN
  Fr cin, cout;                        // cin: read when kk == 0 only
};

struct MleEq {
  const Fr *lo, *hi;                   // the half tables, canonical; hi times COUT
  uint32_t* dst;
  uint64_t n;
  uint32_t lo_log;
};

struct MleTerm {
  Fr c;                                // canonical
  uint32_t nf;
  uint32_t f[MLE_MAX_FACTORS];
};

struct MleRound {
  const uint32_t* tab[MLE_MAX_TABLES];   // the tables of the round: the caller's, or (fused) the folded ones
  const uint32_t* src[MLE_MAX_TABLES];   // fused: the tables to fold
  uint32_t* folded[MLE_MAX_TABLES];
  uint64_t npts;                       // pairs of the round: half the elements of a table of the round
  uint32_t m, n_terms, tile_log, fused;
  MleTerm term[MLE_MAX_TERMS];
  Fr fa, fb;                           // (1 - r_prev) CIN and r_prev CIN
  Fr cin, cout;
  Fr* part;                            // per block MLE_EVALS class-M sums
};

struct MleSum {
  const Fr* src;                       // n rows of MLE_EVALS class-M elements
  Fr* dst;
  uint64_t n;
  uint32_t tile_log, ne;
};

// ---- loads and stores ---------------------------------------------------------------------------------------------------------------

// two neighbouring elements of the call, 64 contiguous bytes, as normalised limbs of whatever 256-bit values they hold
MSM_HD void mle_load_pair(Fr& x0, Fr& x1, const uint32_t* src, uint64_t pair) {
  const uint32_t* s = src + pair * 16;
  uint32_t w0[8], w1[8];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    w0[q] = s[q];
    w1[q] = s[8 + q];
  }
  fr_unpack(x0, w0);
  fr_unpack(x1, w1);
}

template <class FR>
MSM_HD void mle_store_abi(uint32_t* dst, uint64_t idx, const Fr& a, const Fr& cout) {
  Fr x;
  uint32_t o[8];
  fr_mul<FR>(x, a, cout);
  fr_pack(o, x);
  fr_canon<FR>(o);
#pragma unroll
  for (int q = 0; q < 8; q++) dst[idx * 8 + q] = o[q];
}

// a x + b y for lazy x, y and canonical a, b: limbs below 2^30, value below 4r
template <class FR>
MSM_HD void mle_fold(Fr& out, const Fr& x, const Fr& y, const Fr& a, const Fr& b) {
  Fr t, u;
  fr_mul<FR>(t, x, a);
  fr_mul<FR>(u, y, b);
  fr_add(out, t, u);
}

// ---- fix_variables: one tile ----------------------------------------------------------------------------------------------------------

template <class FR>
MSM_HD void mle_fix_load(Fr* lds, const MleFix& p, uint64_t base, uint32_t i) {
  Fr x;
  if (p.src_internal) {
#pragma unroll
    for (int q = 0; q < FR_NL; q++) x.v[q] = p.src[(base + i) * FR_NL + q];
  } else {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.src[(base + i) * 8 + q];
    fr_unpack(x, w);
    if (p.kk == 0) fr_mul<FR>(x, x, p.cin);
  }
  lds[i] = x;
}

// level s, pair j: the values stand 2^s apart
template <class FR>
MSM_HD void mle_fix_level(Fr* lds, const MleFix& p, uint32_t s, uint32_t j) {
  const uint32_t l = j << (s + 1);
  Fr o;
  mle_fold<FR>(o, lds[l], lds[l + (1u << s)], p.a[s], p.b[s]);
  lds[l] = o;
}

template <class FR>
MSM_HD void mle_fix_store(const Fr* lds, const MleFix& p, uint64_t tile, uint32_t i) {
  const uint64_t g = (tile << (p.tile_log - p.kk)) + i;
  const Fr& x = lds[(uint64_t)i << p.kk];
  if (p.dst_internal) {
#pragma unroll
    for (int q = 0; q < FR_NL; q++) p.dst[g * FR_NL + q] = x.v[q];
    return;
  }
  mle_store_abi<FR>(p.dst, g, x, p.cout);
}

// ---- the eq table -----------------------------------------------------------------------------------------------------------------------

template <class FR>
MSM_HD void mle_eq_elem(const MleEq& p, uint64_t b) {
  Fr x;
  uint32_t o[8];
  fr_mul<FR>(x, p.lo[b & (((uint64_t)1 << p.lo_log) - 1)], p.hi[b >> p.lo_log]);
  fr_pack(o, x);
  fr_canon<FR>(o);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[b * 8 + q] = o[q];
}

// ---- a sumcheck round -------------------------------------------------------------------------------------------------------------------

// the points of lane l of block blk: base + l + j lanes, j < MLE_PTS
MSM_HD uint64_t mle_point(uint64_t blk, uint32_t tile_log, uint32_t l, uint32_t j) {
  return (blk << tile_log) + l + (uint64_t)j * poly_lanes(tile_log);
}

// fused: the two folded elements of point pt of every table
template <class FR>
MSM_HD void mle_round_fold(const MleRound& p, uint64_t pt) {
#pragma unroll 1
  for (uint32_t k = 0; k < p.m; k++) {
#pragma unroll 1
    for (uint32_t h = 0; h < 2; h++) {
      Fr x, y, s;
      mle_load_pair(x, y, p.src[k], 2 * pt + h);
      mle_fold<FR>(s, x, y, p.fa, p.fb);
      mle_store_abi<FR>(p.folded[k], 2 * pt + h, s, p.cout);
    }
  }
}

// the terms of one point into the accumulators, t = 0 .. D
template <class FR, int D>
MSM_HD void mle_round_point(Fr (&acc)[D + 1], const MleRound& p, uint64_t pt) {
#pragma unroll 1
  for (uint32_t j = 0; j < p.n_terms; j++) {
    const MleTerm& tm = p.term[j];
    Fr P[D + 1];
#pragma unroll
    for (int t = 0; t <= D; t++) P[t] = tm.c;
#pragma unroll 1
    for (uint32_t k = 0; k < tm.nf; k++) {
      Fr lo, hi, diff, e;
      mle_load_pair(lo, hi, p.tab[tm.f[k]], pt);
      fr_mul<FR>(lo, lo, p.cin);
      fr_mul<FR>(hi, hi, p.cin);
      fr_sub<FR>(diff, hi, lo);
      fr_carry(diff);
      fr_mul<FR>(P[0], lo, P[0]);
      e = hi;
#pragma unroll
      for (int t = 1; t <= D; t++) {
        if (t > 1) fr_add(e, e, diff);
        fr_mul<FR>(P[t], e, P[t]);
        if (t == 3 && D > 3) fr_carry(e);
      }
    }
#pragma unroll
    for (int t = 0; t <= D; t++) {
      fr_add(acc[t], acc[t], P[t]);
      fr_carry(acc[t]);
    }
  }
}

// lane l of block blk: its points, folded first when the round is fused; the lane sums come back in class M
template <class FR, int D>
MSM_HD void mle_round_lane(Fr (&acc)[D + 1], const MleRound& p, uint64_t blk, uint32_t l) {
  Fr one;
  fr_set<FR>(one, FR::ONE);
#pragma unroll
  for (int t = 0; t <= D; t++) fr_zero(acc[t]);
  if (p.fused) {
#pragma unroll 1
    for (uint32_t j = 0; j < MLE_PTS; j++) {
      const uint64_t pt = mle_point(blk, p.tile_log, l, j);
      if (pt < p.npts) mle_round_fold<FR>(p, pt);
    }
  }
#pragma unroll 1
  for (uint32_t j = 0; j < MLE_PTS; j++) {
    const uint64_t pt = mle_point(blk, p.tile_log, l, j);
    if (pt < p.npts) mle_round_point<FR, D>(acc, p, pt);
  }
#pragma unroll
  for (int t = 0; t <= D; t++) fr_mul<FR>(acc[t], acc[t], one);
}

// level s of the block tree over `lanes` class-M values: lane l < lanes >> (s + 1) takes its neighbour half the live width away
template <class FR>
MSM_HD void mle_tree_level(Fr* red, uint32_t lanes, uint32_t s, uint32_t l) {
  const uint32_t half = lanes >> (s + 1);
  Fr a;
  fr_add(a, red[l], red[l + half]);
  fr_carry(a);
  if (s + 1 == MLE_TREE_REDUCE) poly_store_m<FR>(&a, a);
  red[l] = a;
}

// lane l of block blk of a further level: the sum of its MLE_PTS rows at evaluation point t, class M
template <class FR>
MSM_HD void mle_sum_lane(Fr& acc, const MleSum& p, uint64_t blk, uint32_t l, uint32_t t) {
  fr_zero(acc);
#pragma unroll 1
  for (uint32_t j = 0; j < MLE_PTS; j++) {
    const uint64_t row = mle_point(blk, p.tile_log, l, j);
    if (row < p.n) {
      fr_add(acc, acc, p.src[row * MLE_EVALS + t]);
      fr_carry(acc);
    }
  }
  poly_store_m<FR>(&acc, acc);
}

// ---- what a call derives on the host ------------------------------------------------------------------------------------------------

// 1 - x, canonical, for a canonical x
template <class FR>
MSM_HD void mle_one_minus(Fr& r, const Fr& x) {
  Fr one, t;
  fr_set<FR>(one, FR::ONE);
  fr_sub<FR>(t, one, x);
  fr_carry(t);
  poly_store_m<FR>(&r, t);
  fr_reduce<FR>(r);
}

template <class FR>
MSM_HD void mle_mul_canon(Fr& r, const Fr& a, const Fr& b) {
  fr_mul<FR>(r, a, b);
  fr_reduce<FR>(r);
}

// the table of eq(x, point[0 .. k)) over 2^k points, canonical, times `scale`
template <class FR>
void mle_eq_half(std::vector<Fr>& out, const Fr* point, uint32_t k, const Fr& scale) {
  out.assign((size_t)1 << k, scale);
  for (uint32_t i = 0; i < k; i++) {
    Fr q;
    mle_one_minus<FR>(q, point[i]);
    for (size_t b = 0; b < ((size_t)1 << i); b++) {
      mle_mul_canon<FR>(out[b + ((size_t)1 << i)], out[b], point[i]);
      mle_mul_canon<FR>(out[b], out[b], q);
    }
  }
}

MSM_HD uint64_t mle_blocks(uint64_t n, uint32_t tile_log) { return (n + ((uint64_t)1 << tile_log) - 1) >> tile_log; }

// launches of a round over npts pairs: the round itself and the further sums down to one row
MSM_HD uint32_t mle_round_levels(uint64_t npts, uint32_t tile_log) {
  uint32_t levels = 1;
  for (uint64_t n = mle_blocks(npts, tile_log); n > 1; n = mle_blocks(n, tile_log)) levels++;
  return levels;
}

// elements of work memory a round needs: every level's rows
MSM_HD uint64_t mle_round_work_elems(uint64_t npts, uint32_t tile_log) {
  uint64_t n = mle_blocks(npts, tile_log), total = n * MLE_EVALS;
  while (n > 1) {
    n = mle_blocks(n, tile_log);
    total += n * MLE_EVALS;
  }
  return total;
}

// elements of work memory fix_variables needs: the outputs of the first and of the second pass (the later ones ping-pong in them)
MSM_HD uint64_t mle_fix_work_elems(uint32_t nv, uint32_t k, uint32_t tile_log) {
  if (k <= tile_log) return 0;
  uint64_t total = (uint64_t)1 << (nv - tile_log);
  if (k > 2 * tile_log) total += (uint64_t)1 << (nv - 2 * tile_log);
  return total;
}

// The chains of launches, shared by the engine (launchers on a stream) and the host build (loops).  RUN has fix(MleFix), eq(MleEq),
// round<D>(MleRound) and sum(MleSum).

// point: k canonical elements; work: mle_fix_work_elems elements
template <class FR, class RUN>
void mle_chain_fix(RUN& run, uint32_t* out, const uint32_t* in, uint32_t nv, const Fr* point, uint32_t k, bool normal, uint32_t tile_log, Fr* work) {
  MleFix p{};
  fr_const<FR>(p.cin, normal ? 1 : 0);
  fr_const<FR>(p.cout, normal ? 3 : 2);
  Fr* buf[2] = {work, work + ((uint64_t)1 << (nv > tile_log ? nv - tile_log : 0))};
  const uint32_t* src = in;
  uint32_t have = nv, done = 0, pass = 0;
  do {
    const uint32_t kk = k - done < tile_log ? k - done : tile_log;
    p.src = src;
    p.src_internal = pass != 0;
    p.n = (uint64_t)1 << have;
    p.tile_log = have < tile_log ? have : tile_log;
    p.kk = kk;
    for (uint32_t s = 0; s < kk; s++) {
      mle_one_minus<FR>(p.a[s], point[done + s]);
      p.b[s] = point[done + s];
      if (pass == 0 && s == 0) {
        mle_mul_canon<FR>(p.a[s], p.a[s], p.cin);
        mle_mul_canon<FR>(p.b[s], p.b[s], p.cin);
      }
    }
    const bool last = done + kk == k;
    p.dst = last ? out : (uint32_t*)buf[pass & 1];
    p.dst_internal = !last;
    run.fix(p);
    src = p.dst;
    have -= kk;
    done += kk;
    pass++;
  } while (done < k);
}

// lo, hi: device memory for 2^ceil(k/2) and 2^floor(k/2) elements, already filled
template <class FR, class RUN>
void mle_chain_eq(RUN& run, uint32_t* out, const Fr* lo, const Fr* hi, uint32_t k) {
  const MleEq p{lo, hi, out, (uint64_t)1 << k, (k + 1) / 2};
  run.eq(p);
}

template <class FR, class RUN>
void mle_dispatch_round(RUN& run, const MleRound& p, uint32_t D) {
  switch (D) {
    case 1: run.template round<1>(p); break;
    case 2: run.template round<2>(p); break;
    case 3: run.template round<3>(p); break;
    case 4: run.template round<4>(p); break;
    default: run.template round<5>(p); break;
  }
}

// the round and its further sums; returns the row of D + 1 class-M elements in work memory.  p holds everything but part.
template <class FR, class RUN>
const Fr* mle_chain_round(RUN& run, MleRound& p, uint32_t D, Fr* work) {
  p.part = work;
  mle_dispatch_round<FR>(run, p, D);
  uint64_t n = mle_blocks(p.npts, p.tile_log);
  Fr* at = work;
  while (n > 1) {
    const uint64_t nn = mle_blocks(n, p.tile_log);
    const MleSum s{at, at + n * MLE_EVALS, n, p.tile_log, D + 1};
    run.sum(s);
    at += n * MLE_EVALS;
    n = nn;
  }
  return at;
}

#if defined(__HIPCC__)
// (every thread of a block reaches every barrier: the lanes of a small tile are the first threads)

template <class FR>
__global__ void __launch_bounds__(MLE_THREADS) k_mle_fix(MleFix p) {
  __shared__ Fr lds[POLY_MAX_TILE];
  const uint32_t T = 1u << p.tile_log;
  const uint64_t base = (uint64_t)blockIdx.x << p.tile_log;
  for (uint32_t i = threadIdx.x; i < T; i += MLE_THREADS) mle_fix_load<FR>(lds, p, base, i);
  for (uint32_t s = 0; s < p.kk; s++) {
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < (T >> (s + 1)); j += MLE_THREADS) mle_fix_level<FR>(lds, p, s, j);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < (T >> p.kk); i += MLE_THREADS) mle_fix_store<FR>(lds, p, blockIdx.x, i);
}

template <class FR>
__global__ void __launch_bounds__(MLE_THREADS) k_mle_eq(MleEq p) {
  const uint64_t b = (uint64_t)blockIdx.x * MLE_THREADS + threadIdx.x;
  if (b < p.n) mle_eq_elem<FR>(p, b);
}

// the tree over red[0 .. lanes): the sum is left in red[0]
template <class FR>
__device__ void mle_block_tree(Fr* red, uint32_t lanes) {
  for (uint32_t s = 0; (2u << s) <= lanes; s++) {
    __syncthreads();
    if (threadIdx.x < (lanes >> (s + 1))) mle_tree_level<FR>(red, lanes, s, threadIdx.x);
  }
}

// evaluation point T and the ones after it: the lane sums through the tree, one at a time in the same 256 elements of LDS.  (A
// recursion, not a loop over acc[t]: the compiler keeps the accumulators in registers only when no loop indexes them.)
template <class FR, int D, int T>
__device__ __forceinline__ void mle_round_reduce(const Fr (&acc)[D + 1], Fr* red, const MleRound& p, uint32_t lanes, uint32_t l) {
  __syncthreads();
  if (l < lanes) red[l] = acc[T];
  mle_block_tree<FR>(red, lanes);
  if (l == 0) poly_store_m<FR>(p.part + (uint64_t)blockIdx.x * MLE_EVALS + T, red[0]);
  if constexpr (T < D) mle_round_reduce<FR, D, T + 1>(acc, red, p, lanes, l);
}

template <class FR, int D>
__global__ void __launch_bounds__(MLE_THREADS) k_mle_round(MleRound p) {
  __shared__ Fr red[POLY_MAX_LANES];
  const uint32_t lanes = poly_lanes(p.tile_log), l = threadIdx.x;
  Fr acc[D + 1];
  if (l < lanes) mle_round_lane<FR, D>(acc, p, blockIdx.x, l);
  mle_round_reduce<FR, D, 0>(acc, red, p, lanes, l);
}

template <class FR>
__global__ void __launch_bounds__(MLE_THREADS) k_mle_sum(MleSum p) {
  __shared__ Fr red[POLY_MAX_LANES];
  const uint32_t lanes = poly_lanes(p.tile_log), l = threadIdx.x;
#pragma unroll 1
  for (uint32_t t = 0; t < p.ne; t++) {
    __syncthreads();
    if (l < lanes) mle_sum_lane<FR>(red[l], p, blockIdx.x, l, t);
    mle_block_tree<FR>(red, lanes);
    if (l == 0) poly_store_m<FR>(p.dst + (uint64_t)blockIdx.x * MLE_EVALS + t, red[0]);
  }
}
#endif

}  // namespace msm
