// poly.hpp -- the steps between a transform and an MSM over the scalar fields, on the arithmetic of fr.hpp: batch inversion
// (arkworks' batch_inversion_and_mul), polynomial evaluation (DensePolynomial::evaluate), division by X - z (the KZG witness), the
// Lagrange coefficients of a radix-2 domain and the element-wise sum, difference, a*b - c and scaling.
//
// Reference behaviour: ARK ff/src/fields/mod.rs:811-873 (batch inversion; zeros are skipped), poly/src/polynomial/univariate/dense.rs:41-94
// (evaluate), poly/src/polynomial/univariate/mod.rs:102 (divide_with_q_and_r), poly/src/domain/radix2/mod.rs:141-216 (Lagrange
// coefficients, vanishing polynomial), poly/src/domain/mod.rs:190-197 (divide_by_vanishing_poly_on_coset_in_place).
//
// One tiled scheme.  A block takes a tile of T = 2^tile_log consecutive elements (T = 1024 by default) through LDS as k_ntt_pass does:
// thread i loads elements i, i + 256, .. (runs of 32 bytes next to each other), converts them to class M and puts the nine limbs in
// LDS; then lane l owns the POLY_RUN = 4 neighbours 4l .. 4l + 3, so a tile has T / 4 lanes (256 at the default).  A lane works through
// its run in registers, the lanes are combined in LDS, and the stores run like the loads.  Levels are separate launches on one stream:
// no block waits on another, nothing is polled and nothing is atomic -- field arithmetic is exact, so every order gives the same bytes.
//
//   evaluate       lane: Horner over its run (3 products); tile: a tree over the lanes, level s adds v[l + 2^s] z^(4 2^s) into v[l]
//                  (the powers z^(2^s) are constants of the launch); one partial per tile, P_t = sum_i c[tT + i] z^i.  The vector of
//                  partials is a polynomial in z^T of length ceil(n / T): the same kernel runs on it until one element is left, p(z).
//   division       q[i] = S[i + 1] with S[i] = sum_(j >= i) c[j] z^(j - i) (the suffix Horner values; S[0] = p(z) is the remainder).
//                  Inside a tile S is a suffix scan; what enters a tile from the right is S[(t + 1) T] = sum_(u > t) P_u (z^T)^(u - t - 1):
//                  the quotient of the partials by X - z^T.  So the call recurses on the partial vectors (up: the evaluate kernel) and,
//                  on the way down, each tile is read again, takes its carry into its last element (c' = c + z carry) and is stored
//                  one position to the left.  Lane: suffix Horner (3 products); tile: a Hillis-Steele suffix scan over the lane values
//                  with the constant z^(4 2^s) of step s; lane again: S = s_j + z^(4 - j) * (the scan value of the lane to the right).
//   inversion      three launches.  (1) the product of every tile, zeros and the elements past n replaced by 1: lane run, then a tree.
//                  (2) one lane per TILE inverts its product by Fermat (x^(r - 2), a rolled loop of 256 squarings whose bit tests are
//                  wave-uniform because the exponent is a constant) and multiplies by coeff.  (3) Montgomery's trick in its parallel
//                  form inside the tile: 1 / x_i = (product before i) (product after i) / (product of the tile); the products before
//                  and after come from the lane's run and from a prefix and a suffix Hillis-Steele scan over the lane totals.
//
// Lazy bounds (tools/limb_bounds_fr.py --poly; the host build runs every step under MSM_CHECK).  Class M (normalised limbs, value
// < 2r) is closed under fr_mul: r + (2r)(2r) / R < 2r for both fields, so products of products -- the runs, the trees, the scans, the
// powers -- never leave it.  A Horner step acc' = acc z + c is a class-M product plus a class-M element: value < 4r, limbs < 2^30,
// which fr_mul takes as its first operand without a carry pass.  A tree or scan level of the sums adds one class-M product (2r) and
// is followed by one carry pass: from 4r a tile of 256 lanes (8 levels) ends below 20r, R / r = 70.6 for BLS12-381.  A partial is
// brought back to class M (one product by 1) before it is stored, so every level starts from the same bounds.
#pragma once
#include "ntt.hpp"

namespace msm {

constexpr uint32_t POLY_TILE_LOG_MIN = 4, POLY_TILE_LOG_MAX = 10, POLY_DEFAULT_TILE_LOG = 10;
constexpr uint32_t POLY_RUN_LOG = 2, POLY_RUN = 1u << POLY_RUN_LOG;   // the neighbours a lane owns
constexpr uint32_t POLY_THREADS = 256;
constexpr uint32_t POLY_MAX_TILE = 1u << POLY_TILE_LOG_MAX;
constexpr uint32_t POLY_MAX_LANES = POLY_MAX_TILE / POLY_RUN;
constexpr uint32_t POLY_MAX_LOG = 30;
constexpr uint32_t POLY_MAX_LEVELS = 8;                                // 30 / 4, rounded up
constexpr uint32_t POLY_POWERS = POLY_MAX_LEVELS * POLY_TILE_LOG_MAX;

constexpr unsigned kPolyNormal = 1u;                                   // the one flag of a call: plain integers
constexpr unsigned kPolyAdd = 0, kPolySub = 1, kPolyMulSub = 2, kPolyScale = 3;

// z^(2^s), s < tile_log, and z^3: canonical
struct PolyZ {
  Fr p[POLY_TILE_LOG_MAX];
  Fr z3;
};

// the vector a tiled launch reads: 8 words per element in the ABI form of `normal`, or 9 (class-M limbs: a partial vector)
struct PolyTile {
  const uint32_t* src;
  uint64_t n;
  uint32_t tile_log, internal, normal;
};

struct PolyEval {
  PolyTile t;
  Fr* dst;                // one partial per tile, class M
  PolyZ z;
};

struct PolyDiv {
  PolyTile t;
  uint32_t* dst;          // S[i] goes to position i - 1: 8 words canonical in the ABI form (dst_internal == 0) or 9 words class M
  uint32_t dst_internal;
  const Fr* carry;        // what enters tile t from the right, at position t (the last tile takes none); NULL at the top level
  Fr* rem;                // S[0], class M; may be NULL
  PolyZ z;
};

struct PolyInv {
  PolyTile t;
  Fr* tiles;              // launch 1 writes the tile products, launch 2 turns them into coeff / product, launch 3 reads them
  uint32_t* dst;          // launch 3: the ABI form
};

struct PolyLagrange {
  uint32_t* dst;
  uint32_t k, normal, in_domain;
  NttTable w, wi;         // the tables of omega and of its inverse
  Fr tau, c;              // canonical: tau, and n / Z(tau) (unused when tau is in the domain)
};

struct PolyVecOp {
  const uint32_t *a, *b, *c;
  uint32_t* dst;
  uint64_t n;
  uint32_t op, normal;
  Fr s;                   // kPolyScale: the factor, canonical
};

struct PolyDivLane {
  Fr s[POLY_RUN];
};

struct PolyInvLane {
  Fr a, ab, abc, bcd, cd, d;
};

MSM_HD uint32_t poly_lanes(uint32_t tile_log) { return 1u << (tile_log - POLY_RUN_LOG); }
MSM_HD uint64_t poly_tiles(uint64_t n, uint32_t tile_log) { return (n + ((uint64_t)1 << tile_log) - 1) >> tile_log; }

// the lengths of the partial vectors of n elements: len[0] = n, len[j + 1] = ceil(len[j] / T), down to one tile; returns the number
// of levels (>= 1).  The work memory of a call holds, per level j >= 1, the partials and the carries into level j - 1.
MSM_HD uint32_t poly_plan(uint64_t n, uint32_t tile_log, uint64_t (&len)[POLY_MAX_LEVELS + 1]) {
  uint32_t levels = 0;
  len[0] = n;
  while (len[levels] > ((uint64_t)1 << tile_log)) {
    len[levels + 1] = poly_tiles(len[levels], tile_log);
    levels++;
  }
  return levels + 1;
}

// elements of work memory a call on n elements needs: two vectors per level above the first (partials and carries), and a few single ones
MSM_HD uint64_t poly_work_elems(uint64_t n, uint32_t tile_log) {
  uint64_t len[POLY_MAX_LEVELS + 1];
  const uint32_t levels = poly_plan(n, tile_log, len);
  uint64_t total = 8;   // (the remainder; the tile product of a one-tile inversion; the last partial of an evaluation)
  for (uint32_t j = 1; j < levels; j++) total += 2 * len[j];
  return total;
}

template <class FR>
MSM_HD bool fr_is_zero_m(const Fr& a) {   // a class-M value that is 0 modulo r
  Fr t = a;
  fr_reduce<FR>(t);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; i++) o |= t.v[i];
  return o == 0;
}

// word j of r - 2 (j is wave-uniform; the words are immediates)
template <class FR>
MSM_HD uint32_t fr_inv_exp_word(uint32_t j) {
  uint32_t w = 0;
  int64_t b = -2;
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) {
    b += FR::P32[q];
    if (q == j) w = (uint32_t)b;
    b >>= 32;
  }
  return w;
}

// x^(r - 2) for a class-M x, class M: one rolled loop, two product bodies
template <class FR>
MSM_HD void fr_inv_m(Fr& r, const Fr& x) {
  Fr acc;
  fr_set<FR>(acc, FR::ONE);
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    fr_mul<FR>(acc, acc, acc);
    if ((fr_inv_exp_word<FR>((uint32_t)i >> 5) >> (i & 31)) & 1) fr_mul<FR>(acc, acc, x);
  }
  r = acc;
}

// ---- loads and stores of a tile ---------------------------------------------------------------------------------------------------

template <class FR>
MSM_HD void poly_load(Fr& x, const PolyTile& t, uint64_t idx) {
  if (idx >= t.n) {
    fr_zero(x);
    return;
  }
  if (t.internal) {
#pragma unroll
    for (int q = 0; q < FR_NL; q++) x.v[q] = t.src[idx * FR_NL + q];
    return;
  }
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = t.src[idx * 8 + q];
  fr_from_abi<FR>(x, w, t.normal != 0);
}

// the element as the inversion takes it: zeros and what lies past n are 1, and `zero` says which the zeros were
template <class FR>
MSM_HD void poly_inv_load(Fr& x, bool& zero, const PolyTile& t, uint64_t idx) {
  zero = false;
  if (idx < t.n) {
    poly_load<FR>(x, t, idx);
    zero = fr_is_zero_m<FR>(x);
  }
  if (idx >= t.n || zero) fr_set<FR>(x, FR::ONE);
}

template <class FR>
MSM_HD void poly_store_m(Fr* dst, const Fr& x) {   // any first operand -> class M, as limbs
  Fr one, y;
  fr_set<FR>(one, FR::ONE);
  fr_mul<FR>(y, x, one);
  *dst = y;
}

// ---- evaluation: the way up -------------------------------------------------------------------------------------------------------

// lane l: lds[4l] = e0 + z (e1 + z (e2 + z e3))
template <class FR>
MSM_HD void poly_eval_lane(Fr* lds, const PolyZ& z, uint32_t l) {
  Fr acc = lds[POLY_RUN * l + POLY_RUN - 1], t;
#pragma unroll
  for (int j = POLY_RUN - 2; j >= 0; j--) {
    fr_mul<FR>(t, acc, z.p[0]);
    fr_add(acc, t, lds[POLY_RUN * l + j]);
  }
  lds[POLY_RUN * l] = acc;
}

// level s of the tree, pair j: v[l] += v[l + 2^s] z^(4 2^s), l = j 2^(s + 1)
template <class FR>
MSM_HD void poly_eval_tree(Fr* lds, const PolyZ& z, uint32_t s, uint32_t j) {
  const uint32_t l = j << (s + 1);
  Fr t, a = lds[POLY_RUN * l];
  fr_mul<FR>(t, lds[POLY_RUN * (l + (1u << s))], z.p[POLY_RUN_LOG + s]);
  fr_add(a, a, t);
  fr_carry(a);
  lds[POLY_RUN * l] = a;
}

// ---- division by X - z: the way down ----------------------------------------------------------------------------------------------

// lane l: the suffix Horner values of its run (the tile's last element takes the carry first); sc[l] = the run's value
template <class FR>
MSM_HD void poly_div_lane(PolyDivLane& st, const Fr* lds, Fr* sc, const PolyDiv& p, uint64_t tile, uint32_t l) {
  const uint32_t lanes = poly_lanes(p.t.tile_log);
  Fr acc = lds[POLY_RUN * l + POLY_RUN - 1], t;
  if (l + 1 == lanes && p.carry && tile + 1 < poly_tiles(p.t.n, p.t.tile_log)) {
    fr_mul<FR>(t, p.carry[tile], p.z.p[0]);
    fr_add(acc, acc, t);
  }
  st.s[POLY_RUN - 1] = acc;
#pragma unroll
  for (int j = POLY_RUN - 2; j >= 0; j--) {
    fr_mul<FR>(t, acc, p.z.p[0]);
    fr_add(acc, t, lds[POLY_RUN * l + j]);
    st.s[j] = acc;
  }
  sc[l] = acc;
}

// step s of the suffix scan: the new sc[l] (written after a barrier)
template <class FR>
MSM_HD void poly_div_scan(Fr& nv, const Fr* sc, const PolyZ& z, uint32_t lanes, uint32_t s, uint32_t l) {
  nv = sc[l];
  if (l + (1u << s) < lanes) {
    Fr t;
    fr_mul<FR>(t, sc[l + (1u << s)], z.p[POLY_RUN_LOG + s]);
    fr_add(nv, nv, t);
    fr_carry(nv);
  }
}

// lane l: S = s_j + z^(4 - j) * (what the lanes to the right amount to), back into the tile
template <class FR>
MSM_HD void poly_div_finish(const PolyDivLane& st, Fr* lds, const Fr* sc, const PolyZ& z, uint32_t lanes, uint32_t l) {
#pragma unroll
  for (int j = 0; j < (int)POLY_RUN; j++) {
    Fr x = st.s[j];
    if (l + 1 < lanes) {
      Fr t;
      fr_mul<FR>(t, sc[l + 1], j == 0 ? z.p[2] : j == 1 ? z.z3 : j == 2 ? z.p[1] : z.p[0]);
      fr_add(x, x, t);
    }
    fr_carry(x);
    lds[POLY_RUN * l + j] = x;
  }
}

// element i of tile `tile` on the way out: S[g] to position g - 1, S[0] to the remainder
template <class FR>
MSM_HD void poly_div_store(const Fr* lds, const PolyDiv& p, uint64_t tile, uint32_t i) {
  const uint64_t g = (tile << p.t.tile_log) + i;
  if (g >= p.t.n) return;
  if (g == 0) {
    if (p.rem) poly_store_m<FR>(p.rem, lds[i]);
    return;
  }
  if (p.dst_internal) {
    poly_store_m<FR>((Fr*)p.dst + (g - 1), lds[i]);
    return;
  }
  uint32_t w[8];
  fr_to_abi<FR>(w, lds[i], p.t.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[(g - 1) * 8 + q] = w[q];
}

// ---- batch inversion --------------------------------------------------------------------------------------------------------------

template <class FR>
MSM_HD void poly_prod_lane(Fr* lds, uint32_t l) {
  Fr acc = lds[POLY_RUN * l];
#pragma unroll
  for (int j = 1; j < (int)POLY_RUN; j++) fr_mul<FR>(acc, acc, lds[POLY_RUN * l + j]);
  lds[POLY_RUN * l] = acc;
}

template <class FR>
MSM_HD void poly_prod_tree(Fr* lds, uint32_t s, uint32_t j) {
  const uint32_t l = j << (s + 1);
  Fr a = lds[POLY_RUN * l];
  fr_mul<FR>(a, a, lds[POLY_RUN * (l + (1u << s))]);
  lds[POLY_RUN * l] = a;
}

// launch 2, tile t: tiles[t] = coeff / tiles[t]
template <class FR>
MSM_HD void poly_inv_tile(Fr* tiles, const Fr& coeff, uint64_t t) {
  Fr x = tiles[t], y;
  fr_inv_m<FR>(y, x);
  fr_mul<FR>(y, y, coeff);
  tiles[t] = y;
}

// lane l: the products inside its run; pre[l] = suf[l] = the run's product
template <class FR>
MSM_HD void poly_inv_lane(PolyInvLane& st, const Fr* lds, Fr* pre, Fr* suf, uint32_t l) {
  st.a = lds[POLY_RUN * l];
  const Fr b = lds[POLY_RUN * l + 1], c = lds[POLY_RUN * l + 2];
  st.d = lds[POLY_RUN * l + 3];
  Fr tot;
  fr_mul<FR>(st.ab, st.a, b);
  fr_mul<FR>(st.cd, c, st.d);
  fr_mul<FR>(st.abc, st.ab, c);
  fr_mul<FR>(st.bcd, b, st.cd);
  fr_mul<FR>(tot, st.ab, st.cd);
  pre[l] = tot;
  suf[l] = tot;
}

// step s of the two scans: the new pre[l] and suf[l] (written after a barrier)
template <class FR>
MSM_HD void poly_inv_scan(Fr& npre, Fr& nsuf, const Fr* pre, const Fr* suf, uint32_t lanes, uint32_t s, uint32_t l) {
  npre = pre[l];
  nsuf = suf[l];
  if (l >= (1u << s)) fr_mul<FR>(npre, npre, pre[l - (1u << s)]);
  if (l + (1u << s) < lanes) fr_mul<FR>(nsuf, nsuf, suf[l + (1u << s)]);
}

// lane l: coeff / x for its run, from coeff / (the tile's product), the lanes before and the lanes after
template <class FR>
MSM_HD void poly_inv_finish(const PolyInvLane& st, Fr* lds, const Fr* pre, const Fr* suf, const Fr& tile_inv, uint32_t lanes, uint32_t l) {
  Fr c = tile_inv, t;
  if (l > 0) fr_mul<FR>(c, c, pre[l - 1]);
  if (l + 1 < lanes) fr_mul<FR>(c, c, suf[l + 1]);
  fr_mul<FR>(t, c, st.bcd);
  lds[POLY_RUN * l] = t;
  fr_mul<FR>(t, c, st.a);
  fr_mul<FR>(t, t, st.cd);
  lds[POLY_RUN * l + 1] = t;
  fr_mul<FR>(t, c, st.ab);
  fr_mul<FR>(t, t, st.d);
  lds[POLY_RUN * l + 2] = t;
  fr_mul<FR>(t, c, st.abc);
  lds[POLY_RUN * l + 3] = t;
}

template <class FR>
MSM_HD void poly_inv_store(const Fr* lds, const PolyInv& p, uint64_t tile, uint32_t i, bool zero) {
  const uint64_t g = (tile << p.t.tile_log) + i;
  if (g >= p.t.n) return;
  uint32_t w[8];
  fr_to_abi<FR>(w, lds[i], p.t.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[g * 8 + q] = zero ? 0u : w[q];
}

// ---- Lagrange coefficients and the element-wise calls -------------------------------------------------------------------------------

// entry i of the vector the inversion turns into L_i(tau): (tau - w^i) (n / Z(tau)) w^-i; with tau in the domain, L_i(tau) itself
template <class FR>
MSM_HD void poly_lagrange_entry(const PolyLagrange& p, uint32_t i) {
  const uint32_t h = ntt_lo_log(p.k);
  Fr w = p.w.lo[i & ((1u << h) - 1)], x;
  fr_mul<FR>(w, w, p.w.hi[i >> h]);
  if (p.in_domain) {
    fr_reduce<FR>(w);
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < FR_NL; q++) diff |= w.v[q] ^ p.tau.v[q];
    fr_set<FR>(x, FR::ONE);
    if (diff) fr_zero(x);
  } else {
    fr_sub<FR>(x, p.tau, w);
    fr_carry(x);
    fr_mul<FR>(x, x, p.c);
    ntt_table_mul<FR>(x, p.wi, p.k, i);
  }
  uint32_t o[8];
  fr_to_abi<FR>(o, x, p.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[(size_t)i * 8 + q] = o[q];
}

template <class FR>
MSM_HD void poly_vec_op(const PolyVecOp& p, uint64_t i) {
  uint32_t w[8];
  Fr x, y, t;
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = p.a[i * 8 + q];
  fr_from_abi<FR>(x, w, p.normal != 0);
  if (p.op == kPolyScale) {
    fr_mul<FR>(x, x, p.s);
  } else {
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.b[i * 8 + q];
    fr_from_abi<FR>(y, w, p.normal != 0);
    if (p.op == kPolyAdd) {
      fr_add(x, x, y);
    } else if (p.op == kPolySub) {
      fr_sub<FR>(x, x, y);
    } else {
      fr_mul<FR>(t, x, y);
#pragma unroll
      for (int q = 0; q < 8; q++) w[q] = p.c[i * 8 + q];
      fr_from_abi<FR>(y, w, p.normal != 0);
      fr_sub<FR>(x, t, y);
    }
    fr_carry(x);
  }
  fr_to_abi<FR>(w, x, p.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[i * 8 + q] = w[q];
}

// ---- what a call derives on the host ----------------------------------------------------------------------------------------------

// one host element in the form of the call -> canonical limbs
template <class FR>
MSM_HD void poly_scalar(Fr& x, const void* bytes32, bool normal) {
  uint32_t w[8];
  const uint8_t* b = (const uint8_t*)bytes32;
  for (int q = 0; q < 8; q++) w[q] = (uint32_t)b[4 * q] | ((uint32_t)b[4 * q + 1] << 8) | ((uint32_t)b[4 * q + 2] << 16) | ((uint32_t)b[4 * q + 3] << 24);
  fr_from_abi<FR>(x, w, normal);
  fr_reduce<FR>(x);
}

template <class FR>
MSM_HD void poly_scalar_out(void* bytes32, const Fr& x, bool normal) {
  uint32_t w[8];
  fr_to_abi<FR>(w, x, normal);
  uint8_t* b = (uint8_t*)bytes32;
  for (int q = 0; q < 32; q++) b[q] = (uint8_t)(w[q >> 2] >> (8 * (q & 3)));
}

// pw[i] = z^(2^i), canonical
template <class FR>
MSM_HD void poly_powers(Fr (&pw)[POLY_POWERS], const Fr& z) {
  pw[0] = z;
  for (uint32_t i = 1; i < POLY_POWERS; i++) {
    fr_mul<FR>(pw[i], pw[i - 1], pw[i - 1]);
    fr_reduce<FR>(pw[i]);
  }
}

// the constants of level j: powers of z^(T^j)
template <class FR>
MSM_HD void poly_level_z(PolyZ& z, const Fr (&pw)[POLY_POWERS], uint32_t tile_log, uint32_t level) {
  for (uint32_t s = 0; s < POLY_TILE_LOG_MAX; s++) z.p[s] = pw[level * tile_log + (s < tile_log ? s : 0)];
  fr_mul<FR>(z.z3, z.p[0], z.p[1]);
  fr_reduce<FR>(z.z3);
}

// tau^(2^k) - 1, canonical
template <class FR>
MSM_HD void poly_vanishing(Fr& r, const Fr& tau, uint32_t k) {
  Fr x = tau, one;
  ntt_hi_base<FR>(x, tau, k);
  fr_set<FR>(one, FR::ONE);
  fr_sub<FR>(x, x, one);
  fr_carry(x);
  poly_store_m<FR>(&r, x);
  fr_reduce<FR>(r);
}

// The chains of launches, shared by the engine (launchers on a stream) and the host build (loops).  RUN has eval(PolyEval),
// div(PolyDiv), inv_prod(PolyInv), inv_tiles(Fr*, uint64_t count, Fr coeff), inv_apply(PolyInv).

// p(z) as one class-M element in work memory; n >= 1
template <class FR, class RUN>
const Fr* poly_chain_evaluate(RUN& run, const uint32_t* src, uint64_t n, bool normal, uint32_t tile_log, const Fr& z, Fr* work) {
  Fr pw[POLY_POWERS];
  poly_powers<FR>(pw, z);
  PolyEval e;
  e.t = PolyTile{src, n, tile_log, 0, normal ? 1u : 0u};
  Fr* at = work + 2;
  for (uint32_t level = 0;; level++) {
    poly_level_z<FR>(e.z, pw, tile_log, level);
    const uint64_t m = poly_tiles(e.t.n, tile_log);
    e.dst = at;
    run.eval(e);
    if (m == 1) return at;
    e.t = PolyTile{(const uint32_t*)at, m, tile_log, 1, 0};
    at += 2 * m;
  }
}

// the quotient by X - z into dst (n - 1 elements, ABI form) and the remainder as a class-M element in work memory; n >= 1
template <class FR, class RUN>
const Fr* poly_chain_divide(RUN& run, uint32_t* dst, const uint32_t* src, uint64_t n, bool normal, uint32_t tile_log, const Fr& z, Fr* work) {
  Fr pw[POLY_POWERS];
  poly_powers<FR>(pw, z);
  uint64_t len[POLY_MAX_LEVELS + 1];
  const uint32_t levels = poly_plan(n, tile_log, len);
  Fr* part[POLY_MAX_LEVELS + 1];   // part[j]: the partials of level j - 1 (the vector of level j); part[j] + len[j]: the carries into level j - 1
  Fr* at = work + 2;
  for (uint32_t j = 1; j < levels; j++) {
    part[j] = at;
    at += 2 * len[j];
  }
  for (uint32_t j = 0; j + 1 < levels; j++) {
    PolyEval e;
    e.t = j == 0 ? PolyTile{src, n, tile_log, 0, normal ? 1u : 0u} : PolyTile{(const uint32_t*)part[j], len[j], tile_log, 1, 0};
    poly_level_z<FR>(e.z, pw, tile_log, j);
    e.dst = part[j + 1];
    run.eval(e);
  }
  for (uint32_t j = levels; j-- > 0;) {
    PolyDiv d;
    d.t = j == 0 ? PolyTile{src, n, tile_log, 0, normal ? 1u : 0u} : PolyTile{(const uint32_t*)part[j], len[j], tile_log, 1, 0};
    poly_level_z<FR>(d.z, pw, tile_log, j);
    d.dst = j == 0 ? dst : (uint32_t*)(part[j] + len[j]);
    d.dst_internal = j != 0;
    d.carry = j + 1 < levels ? part[j + 1] + len[j + 1] : nullptr;
    d.rem = j + 1 == levels ? work : nullptr;
    run.div(d);
  }
  return work;
}

// dst[i] = coeff / src[i] (0 for 0), the ABI form on both sides; dst == src is allowed; n >= 1
template <class FR, class RUN>
void poly_chain_inverse(RUN& run, uint32_t* dst, const uint32_t* src, uint64_t n, bool normal, uint32_t tile_log, const Fr& coeff, Fr* work) {
  PolyInv p;
  p.t = PolyTile{src, n, tile_log, 0, normal ? 1u : 0u};
  p.tiles = work + 2;
  p.dst = dst;
  run.inv_prod(p);
  run.inv_tiles(p.tiles, poly_tiles(n, tile_log), coeff);
  run.inv_apply(p);
}

#if defined(__HIPCC__)
// (every thread of a block reaches every barrier: the lanes of a small tile are the first threads, the others only load and store)

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_eval(PolyEval p) {
  __shared__ Fr lds[POLY_MAX_TILE];
  const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log);
  const uint64_t base = (uint64_t)blockIdx.x << p.t.tile_log;
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS) poly_load<FR>(lds[i], p.t, base + i);
  __syncthreads();
  if (threadIdx.x < lanes) poly_eval_lane<FR>(lds, p.z, threadIdx.x);
  for (uint32_t s = 0; (2u << s) <= lanes; s++) {
    __syncthreads();
    if (threadIdx.x < (lanes >> (s + 1))) poly_eval_tree<FR>(lds, p.z, s, threadIdx.x);
  }
  if (threadIdx.x == 0) poly_store_m<FR>(p.dst + blockIdx.x, lds[0]);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_div(PolyDiv p) {
  __shared__ Fr lds[POLY_MAX_TILE];
  __shared__ Fr sc[POLY_MAX_LANES];
  const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log), l = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x << p.t.tile_log;
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS) poly_load<FR>(lds[i], p.t, base + i);
  __syncthreads();
  PolyDivLane st;
  if (l < lanes) poly_div_lane<FR>(st, lds, sc, p, blockIdx.x, l);
  for (uint32_t s = 0; (1u << s) < lanes; s++) {
    __syncthreads();
    Fr nv;
    if (l < lanes) poly_div_scan<FR>(nv, sc, p.z, lanes, s, l);
    __syncthreads();
    if (l < lanes) sc[l] = nv;
  }
  __syncthreads();
  if (l < lanes) poly_div_finish<FR>(st, lds, sc, p.z, lanes, l);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS) poly_div_store<FR>(lds, p, blockIdx.x, i);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_inv_prod(PolyInv p) {
  __shared__ Fr lds[POLY_MAX_TILE];
  const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log);
  const uint64_t base = (uint64_t)blockIdx.x << p.t.tile_log;
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS) {
    bool zero;
    poly_inv_load<FR>(lds[i], zero, p.t, base + i);
  }
  __syncthreads();
  if (threadIdx.x < lanes) poly_prod_lane<FR>(lds, threadIdx.x);
  for (uint32_t s = 0; (2u << s) <= lanes; s++) {
    __syncthreads();
    if (threadIdx.x < (lanes >> (s + 1))) poly_prod_tree<FR>(lds, s, threadIdx.x);
  }
  if (threadIdx.x == 0) p.tiles[blockIdx.x] = lds[0];
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_inv_tiles(Fr* tiles, uint64_t count, Fr coeff) {
  const uint64_t t = (uint64_t)blockIdx.x * POLY_THREADS + threadIdx.x;
  if (t < count) poly_inv_tile<FR>(tiles, coeff, t);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_inv_apply(PolyInv p) {
  __shared__ Fr lds[POLY_MAX_TILE];
  __shared__ Fr pre[POLY_MAX_LANES];
  __shared__ Fr suf[POLY_MAX_LANES];
  const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log), l = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x << p.t.tile_log;
  uint32_t zeros = 0, it = 0;
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS, it++) {
    bool zero;
    poly_inv_load<FR>(lds[i], zero, p.t, base + i);
    zeros |= (zero ? 1u : 0u) << it;
  }
  __syncthreads();
  PolyInvLane st;
  if (l < lanes) poly_inv_lane<FR>(st, lds, pre, suf, l);
  for (uint32_t s = 0; (1u << s) < lanes; s++) {
    __syncthreads();
    Fr npre, nsuf;
    if (l < lanes) poly_inv_scan<FR>(npre, nsuf, pre, suf, lanes, s, l);
    __syncthreads();
    if (l < lanes) {
      pre[l] = npre;
      suf[l] = nsuf;
    }
  }
  __syncthreads();
  if (l < lanes) poly_inv_finish<FR>(st, lds, pre, suf, p.tiles[blockIdx.x], lanes, l);
  __syncthreads();
  it = 0;
  for (uint32_t i = threadIdx.x; i < T; i += POLY_THREADS, it++) poly_inv_store<FR>(lds, p, blockIdx.x, i, ((zeros >> it) & 1u) != 0);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_lagrange(PolyLagrange p) {
  const uint32_t i = blockIdx.x * POLY_THREADS + threadIdx.x;
  if ((i >> p.k) == 0) poly_lagrange_entry<FR>(p, i);
}

template <class FR>
__global__ void __launch_bounds__(POLY_THREADS) k_poly_vec_op(PolyVecOp p) {
  const uint64_t i = (uint64_t)blockIdx.x * POLY_THREADS + threadIdx.x;
  if (i < p.n) poly_vec_op<FR>(p, i);
}
#endif

}  // namespace msm
