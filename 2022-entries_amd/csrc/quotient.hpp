// quotient.hpp -- the row loop of a TurboPlonk prover's third round (the coset evaluations of the quotient polynomial) and the linear
// combination of polynomials with host scalars of its fourth and fifth, on the arithmetic of fr.hpp.
//
// Reference behaviour: Jellyfish's compute_quotient_polynomial (plonk/src/proof_system/prover.rs:368-395, 414-447, 457-500).  All
// vectors hold M = 2^K evaluations on g H_M in natural order; n = M / ratio is the size of the constraint domain.  Row i, with
// x = g omega_M^i:
//
//   t_circ  = q_c + pi + sum_(j<4) q_lc[j] w_j + q_mul[0] w0 w1 + q_mul[1] w2 w3 + q_ecc w0 w1 w2 w3 w4 + sum_(j<4) q_hash[j] w_j^5 - q_o w4
//   t_perm1 = alpha (z[i] prod_j (w_j + beta ks[j] x + gamma) - z[(i + ratio) mod M] prod_j (w_j + beta sigma_j + gamma))
//   t_perm2 = alpha^2 (z[i] - 1) / (n (x - 1))
//   out[i]  = (t_circ + t_perm1) / ((g omega_M^(i mod ratio))^n - 1) + t_perm2
//
// Three steps, separate launches on one stream; nothing is atomic or polled.  (1) k_quot_xm1, one lane per row: x - 1 into work
// memory.  (2) the batch inversion of poly.hpp, in place, with the factor alpha^2 / n: its three launches.  x - 1 is never zero (the
// call refuses an offset inside the domain), so the inversion's zero convention is not reached.  (3) k_quot_rows, one lane per row: x
// from the handle's two-level tables as scan_perm_row reads them, times g; ONE rolled loop over the m columns that carries the two
// permutation products (started from z[i] and z[i + ratio]) and, with selectors, the gate: q_lc[j] w_j + q_hash[j] w_j^5 for j < 4,
// q_mul[j / 2] w_(j-1) w_j at odd j, the running product of all wires for q_ecc, and q_o w4 at j = 4.  No wire is kept past its
// iteration but the previous one, so nothing is indexed by a lane-variable and nothing spills.  The host prepares what is constant:
// the `ratio` inverses of Z_H, alpha, alpha^2 / n, beta ks[j], beta, gamma, g -- canonical elements in the launch's arguments; a lane
// picks its inverse of Z_H by a rolled loop of selects.
//
// The linear combination is one launch and one pass: one lane per element, a rolled loop over the m columns, a column that has ended
// contributes nothing.
//
// Lazy bounds (tools/limb_bounds_fr.py --quotient; the host build runs every row under MSM_CHECK).  Products are class M (normalised
// limbs, value < 2r).  The gate accumulator starts as q_c + pi (limbs < 2^30, < 4r); an iteration adds at most three class-M products
// and ends with one carry pass (limbs < 2^29 + 8 in, < 2^31 + 8 before it), so after the eleven added products it is below 26r; the
// subtraction of q_o w4 adds 4r (30r), t_perm1 -- one class-M product -- 2r more: 32r, R / r = 70.6 for BLS12-381, into the product
// by 1 / Z_H.  A permutation factor is two class-M values and one canonical one (below 5r, limbs below 3 * 2^29), as in scan.hpp.  The
// linear combination adds one class-M product per column and carries: at most 32 columns, 64r < R.
#pragma once
#include "poly.hpp"

namespace msm {

constexpr unsigned kQuotNormal = 1u;                                  // the one flag of a call: plain integers
constexpr uint32_t QUOT_MAX_COLUMNS = 8, QUOT_GATE_WIRES = 5, QUOT_SELECTORS = 13, QUOT_MAX_RATIO = 16;
constexpr uint32_t QUOT_Q_MUL = 4, QUOT_Q_HASH = 6, QUOT_Q_O = 10, QUOT_Q_C = 11, QUOT_Q_ECC = 12;   // q_lc is 0 .. 3
constexpr uint32_t LINCOMB_MAX_COLUMNS = 32;

// step 1: x_i - 1, as arkworks images (the work memory of a call is in that form whatever the form of the call)
struct QuotXm1 {
  uint32_t* dst;          // 2^k elements
  uint32_t k;
  NttTable w;             // the tables of omega_M
  Fr g;                   // canonical
};

// step 3, one row per lane
struct QuotRows {
  const uint32_t *wires, *sigmas, *selectors;   // m, m and 13 (or NULL) columns `stride` elements apart, the ABI form
  const uint32_t *z, *pi;                       // pi may be NULL
  const uint32_t* l1;                           // alpha^2 / (n (x_i - 1)), arkworks images: what steps 1 and 2 left in work memory
  uint32_t* dst;
  uint64_t stride;
  uint32_t k, m, ratio;
  NttTable w;                                   // the tables of omega_M
  Fr cin, cout;                                 // the conversion constants of the form of the call (quot_form)
  Fr g, alpha, beta, gamma;                     // canonical
  Fr bks[QUOT_MAX_COLUMNS];                     // beta ks[j], canonical
  Fr zh_inv[QUOT_MAX_RATIO];                    // 1 / ((g omega_M^i)^n - 1), i < ratio, canonical
};

struct LinComb {
  const uint32_t* cols[LINCOMB_MAX_COLUMNS];
  uint32_t lens[LINCOMB_MAX_COLUMNS];
  Fr coeffs[LINCOMB_MAX_COLUMNS];               // canonical
  uint32_t* dst;
  uint32_t n, m;                                // n = max(lens)
  Fr cin, cout;                                 // the conversion constants of the form of the call (quot_form)
};

// the constants that take ABI words of the form of the call to class M and back: they travel with the launch, so the kernels hold one
// product per conversion whatever the form
template <class FR>
MSM_HD void quot_form(Fr& cin, Fr& cout, bool normal) {
  fr_const<FR>(cin, normal ? 1 : 0);
  fr_const<FR>(cout, normal ? 3 : 2);
}

// x = g omega^i, class M
template <class FR>
MSM_HD void quot_x(Fr& x, const NttTable& w, const Fr& g, uint32_t k, uint32_t i) {
  const uint32_t h = ntt_lo_log(k);
  x = w.lo[i & ((1u << h) - 1)];
  fr_mul<FR>(x, x, w.hi[i >> h]);
  fr_mul<FR>(x, x, g);
}

// ABI words (any 256-bit value) -> class M, as fr_from_abi does it
template <class FR>
MSM_HD void quot_load(Fr& x, const uint32_t* src, uint64_t idx, const Fr& cin) {
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = src[idx * 8 + q];
  fr_unpack(x, w);
  fr_mul<FR>(x, x, cin);
}

// any mul input -> canonical ABI words, as fr_to_abi does it
template <class FR>
MSM_HD void quot_store(uint32_t* dst, uint64_t idx, const Fr& a, const Fr& cout) {
  Fr x;
  uint32_t o[8];
  fr_mul<FR>(x, a, cout);
  fr_pack(o, x);
  fr_canon<FR>(o);
#pragma unroll
  for (int q = 0; q < 8; q++) dst[idx * 8 + q] = o[q];
}

template <class FR>
MSM_HD void quot_xm1_row(const QuotXm1& p, uint32_t i) {
  Fr x, one;
  quot_x<FR>(x, p.w, p.g, p.k, i);
  fr_set<FR>(one, FR::ONE);
  fr_sub<FR>(x, x, one);
  fr_carry(x);
  uint32_t o[8];
  fr_to_abi<FR>(o, x, false);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[(size_t)i * 8 + q] = o[q];
}

// row i of the quotient; the column loop stays rolled
template <class FR>
MSM_HD void quot_row(const QuotRows& p, uint32_t i) {
  const Fr& cin = p.cin;
  const uint32_t mask = (1u << p.k) - 1;
  Fr x, num, den, t2, acc, t;
  quot_x<FR>(x, p.w, p.g, p.k, i);
  quot_load<FR>(num, p.z, i, cin);
  quot_load<FR>(den, p.z, (i + p.ratio) & mask, cin);
  // t_perm2 = (z[i] - 1) * alpha^2 / (n (x - 1))
  fr_set<FR>(t, FR::ONE);
  fr_sub<FR>(t2, num, t);
  fr_carry(t2);
  {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.l1[(size_t)i * 8 + q];
    fr_from_abi<FR>(t, w, false);
  }
  fr_mul<FR>(t2, t2, t);
  // the gate starts as q_c + pi
  fr_zero(acc);
  if (p.pi) quot_load<FR>(acc, p.pi, i, cin);
  if (p.selectors) {
    quot_load<FR>(t, p.selectors, QUOT_Q_C * p.stride + i, cin);
    fr_add(acc, acc, t);
  }
  Fr prev, ecc;
  fr_set<FR>(ecc, FR::ONE);
  prev = ecc;
#pragma unroll 1
  for (uint32_t j = 0; j < p.m; j++) {
    Fr wv, wg, sg;
    const uint64_t at = j * p.stride + i;
    quot_load<FR>(wv, p.wires, at, cin);
    quot_load<FR>(sg, p.sigmas, at, cin);
    fr_add(wg, wv, p.gamma);
    fr_mul<FR>(t, x, p.bks[j]);
    fr_add(t, t, wg);
    fr_mul<FR>(num, t, num);
    fr_mul<FR>(t, sg, p.beta);
    fr_add(t, t, wg);
    fr_mul<FR>(den, t, den);
    if (p.selectors) {
      Fr q;
      fr_mul<FR>(ecc, ecc, wv);
      if (j + 1 < QUOT_GATE_WIRES) {
        quot_load<FR>(q, p.selectors, j * p.stride + i, cin);
        fr_mul<FR>(t, q, wv);
        fr_add(acc, acc, t);
        fr_mul<FR>(t, wv, wv);
        fr_mul<FR>(t, t, t);
        fr_mul<FR>(t, t, wv);
        quot_load<FR>(q, p.selectors, (QUOT_Q_HASH + j) * p.stride + i, cin);
        fr_mul<FR>(t, q, t);
        fr_add(acc, acc, t);
        if (j & 1) {
          fr_mul<FR>(t, prev, wv);
          quot_load<FR>(q, p.selectors, (QUOT_Q_MUL + (j >> 1)) * p.stride + i, cin);
          fr_mul<FR>(t, q, t);
          fr_add(acc, acc, t);
        }
        fr_carry(acc);
      } else {
        quot_load<FR>(q, p.selectors, QUOT_Q_ECC * p.stride + i, cin);
        fr_mul<FR>(t, q, ecc);
        fr_add(acc, acc, t);
        fr_carry(acc);
        quot_load<FR>(q, p.selectors, QUOT_Q_O * p.stride + i, cin);
        fr_mul<FR>(t, q, wv);
        fr_sub<FR>(acc, acc, t);
        fr_carry(acc);
      }
      prev = wv;
    }
  }
  // t_perm1 = alpha (num - den)
  fr_sub<FR>(t, num, den);
  fr_carry(t);
  fr_mul<FR>(t, t, p.alpha);
  fr_add(acc, acc, t);
  // 1 / Z_H of the row: a rolled loop of selects over the launch's constants
  Fr zh = p.zh_inv[0];
#pragma unroll 1
  for (uint32_t q = 1; q < p.ratio; q++) {
    const bool mine = (i & (p.ratio - 1)) == q;
#pragma unroll
    for (int l = 0; l < FR_NL; l++) zh.v[l] = mine ? p.zh_inv[q].v[l] : zh.v[l];
  }
  fr_mul<FR>(t, acc, zh);
  fr_add(t, t, t2);
  quot_store<FR>(p.dst, i, t, p.cout);
}

// element i of the linear combination; the column loop stays rolled
template <class FR>
MSM_HD void lincomb_elem(const LinComb& p, uint32_t i) {
  Fr acc;
  fr_zero(acc);
#pragma unroll 1
  for (uint32_t j = 0; j < p.m; j++) {
    if (i < p.lens[j]) {
      Fr x;
      quot_load<FR>(x, p.cols[j], i, p.cin);
      fr_mul<FR>(x, x, p.coeffs[j]);
      fr_add(acc, acc, x);
      fr_carry(acc);
    }
  }
  quot_store<FR>(p.dst, i, acc, p.cout);
}

// ---- what a call derives on the host ----------------------------------------------------------------------------------------------

// elements of 36 bytes of work memory the rows of a domain of M points need: the M values x_i - 1 and their inverses in place (32
// bytes each) and the tile products of the inversion
MSM_HD uint64_t quot_work_elems(uint64_t M, uint32_t tile_log) { return poly_work_elems(M, tile_log) + (M * 32 + sizeof(Fr) - 1) / sizeof(Fr); }

// the constants of a call from canonical alpha, beta, gamma, g and ks (in p.bks): returns false when some (g omega_M^i)^n = 1, i < ratio
template <class FR>
MSM_HD bool quot_constants(QuotRows& p, Fr& a2n, const Fr& alpha, uint32_t log_n) {
  const uint32_t ratio_log = p.k - log_n;
  Fr gn, rho, one, zero, cur, zn;
  fr_zero(zero);
  fr_set<FR>(one, FR::ONE);
  ntt_hi_base<FR>(gn, p.g, log_n);          // g^n
  ntt_root<FR>(rho, ratio_log);             // omega_M^n: the root of unity of order `ratio`
  cur = gn;
  bool ok = true;
  for (uint32_t i = 0; i < p.ratio; i++) {
    Fr zh;
    fr_sub<FR>(zh, cur, one);
    fr_carry(zh);
    poly_store_m<FR>(&zh, zh);
    fr_reduce<FR>(zh);
    uint32_t any = 0;
    for (int q = 0; q < FR_NL; q++) any |= zh.v[q];
    if (!any) ok = false;
    fr_inv<FR>(p.zh_inv[i], zh);
    fr_mul<FR>(cur, cur, rho);
    fr_reduce<FR>(cur);
  }
  for (uint32_t i = p.ratio; i < QUOT_MAX_RATIO; i++) p.zh_inv[i] = zero;
  p.alpha = alpha;
  for (uint32_t j = 0; j < QUOT_MAX_COLUMNS; j++) {
    if (j < p.m) {
      fr_mul<FR>(p.bks[j], p.bks[j], p.beta);
      fr_reduce<FR>(p.bks[j]);
    } else {
      p.bks[j] = zero;
    }
  }
  ntt_size_inv<FR>(zn, log_n);
  fr_mul<FR>(a2n, alpha, alpha);
  fr_reduce<FR>(a2n);
  fr_mul<FR>(a2n, a2n, zn);
  fr_reduce<FR>(a2n);
  return ok;
}

// The chain of launches of the quotient's rows, shared by the engine (launchers on a stream) and the host build (loops).  RUN has
// xm1(QuotXm1), rows(QuotRows) and the inversion of poly_chain_inverse.  `work`: quot_work_elems elements.
template <class FR, class RUN>
void quot_chain(RUN& run, QuotRows& p, const Fr& a2n, uint32_t tile_log, Fr* work) {
  const uint64_t M = (uint64_t)1 << p.k;
  const uint64_t inv_elems = poly_work_elems(M, tile_log);
  uint32_t* l1 = (uint32_t*)(work + inv_elems);
  run.xm1(QuotXm1{l1, p.k, p.w, p.g});
  poly_chain_inverse<FR>(run, l1, l1, M, false, tile_log, a2n, work);
  p.l1 = l1;
  run.rows(p);
}

#if defined(__HIPCC__)
template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_quot_xm1(QuotXm1 p) {
  const uint32_t i = blockIdx.x * POLY_THREADS + threadIdx.x;
  if ((i >> p.k) == 0) quot_xm1_row<FR>(p, i);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_quot_rows(QuotRows p) {
  const uint32_t i = blockIdx.x * POLY_THREADS + threadIdx.x;
  if ((i >> p.k) == 0) quot_row<FR>(p, i);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_lincomb(LinComb p) {
  const uint32_t i = blockIdx.x * POLY_THREADS + threadIdx.x;
  if (i < p.n) lincomb_elem<FR>(p, i);
}
#endif

}  // namespace msm
