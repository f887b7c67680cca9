// poseidon.hpp -- Poseidon sponges over the scalar fields on the arithmetic of fr.hpp: n independent duplex sponges of one shape, one
// lane each, and what a parameter handle derives on the host (the sparse form of the partial rounds and the schedule of reductions).
//
// Reference behaviour: snarkVM's PoseidonSponge (console/algorithms/src/poseidon/helpers/sponge.rs) -- the state is [capacity | rate]
// with capacity 1, an absorbed element is ADDED to a rate cell, a round is ark, S-box, mds, the rounds Rf/2 .. Rf/2 + Rp - 1 are
// partial (their S-box acts on element 0 alone) -- and its callers hash_many (a header [domain, length, 0 ..] of `rate` elements in
// front of the input) and the Poseidon Merkle tree (console/collections/src/merkle_tree: a leading 0 or 1 in front of a row).
// Nothing about alpha = 17 or 8 + 31 rounds is in the code: rate, alpha and the round numbers are run-time values of the table.
//
// One lane per sponge.  The state, t = rate + 1 elements of nine limbs, lives in LDS, lane-interleaved (limb q of element e of lane
// l at word (e * 9 + q) * POS_LANES + l: the 64 lanes of a wave read 64 neighbours, no bank conflict, and no lane reads another's), in two
// copies between which a dense matrix moves it.  Every loop -- rounds, elements, matrix rows and columns, the bits of alpha, the
// elements of a row -- is rolled: the code holds each kind of product once and is the same for every t.  Round constants and matrices
// are indexed by the round counter alone, which is wave-uniform, so they are read on the scalar unit.
//
// Sparse partial rounds (pos_build).  Write the linear layer N of partial round k as N = N'' N' with N' = [[1, 0], [0, N^]] (N^: N
// without row and column 0) and N'' = [[N00, v^], [w, I]], v^ = N[0, 1:] N^^-1, w = N[1:, 0].  N' commutes with the partial S-box, so it
// moves backward: the constant of round k becomes N' c_k and the linear layer of the round before becomes N' M, which is factored in
// turn, starting from the last partial round with N = M; the dense matrix left over replaces M in the last full round of the first
// half.  A partial round then costs the S-box and 2t - 1 products (out_0 = N00 s_0 + sum v^_j s_j, out_i = w_i s_0 + s_i) instead of
// t^2.  A singular N^ is refused at create.
//
// Lazy bounds (tools/limb_bounds_fr.py --poseidon; the host build checks every product, MSM_CHECK).  In units of r, with K = 2^261 / r
// (447 for BLS12-377, 70.6 for BLS12-381): a product a * b / R of a lazy a below B r and a canonical b is below (1 + B / K) r, a sum
// of t of them below t (1 + B / K) r.  The first square of an S-box has the lazy element on both sides and needs B^2 < K for a class-M
// result; an element that skips the product in a sparse partial round grows by about 2r per round (the product w_i s_0 and the
// constant).  pos_build follows these bounds round by round and sets, per round, bit 0 (bring the S-box inputs to class M by a product
// with 1 first) and bit 1 (the same for the elements 1 .. t - 1 of a sparse partial round) where a bound would otherwise be passed:
// nowhere for BLS12-377; for BLS12-381 in the first round when t >= 6, in the full rounds when t >= 8 and every few partial
// rounds.  These products are counted in "products_per_permutation".
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#include "ntt.hpp"

namespace msm {

constexpr unsigned kPosNormal = 1u, kPosDevice = 2u;        // the flags of a call: plain integers; device pointers
constexpr uint32_t POS_LANES = 64;                          // lanes per block: one wave
constexpr uint32_t POS_MAX_RATE = 8, POS_MAX_T = POS_MAX_RATE + 1;
constexpr uint32_t POS_MAX_LEN = 1u << 16, POS_MAX_N_LOG = 30, POS_MAX_ROUNDS = 1u << 12;
constexpr uint32_t kPosRedSbox = 1u, kPosRedLazy = 2u;      // the reductions of a round
constexpr uint32_t kPosLeadNone = 0, kPosLeadZero = 1, kPosLeadOne = 2;

// the table of a handle on the device (or the host): canonical Montgomery limbs
struct PosTab {
  const Fr* ark;            // (rf + rp) * t: the caller's constants
  const Fr* mds;            // t * t, row-major
  const Fr* ark_s;          // (rf + rp) * t: the constants of the sparse form (N' c_k in the partial rounds)
  const Fr* pre;            // t * t: the dense matrix of the last full round of the first half in the sparse form
  const Fr* sp;             // rp * (2t - 1): N00, v^[1 .. t), w[1 .. t) of each partial round
  const uint32_t* red_d;    // rf + rp: the reductions of each round, dense form
  const uint32_t* red_s;    //          and sparse form
  uint32_t t, rate, alpha, rf, rp;
};

struct PosRun {
  PosTab tab;
  const uint32_t* in;       // row i: the elements i * row_stride .. , in the form of the call
  uint32_t* out;            // row i: n_out elements
  uint64_t n, row_stride;
  uint32_t in_len;          // elements absorbed per row, the leading constant included
  uint32_t n_out, sparse, lead, has_header;
  Fr hdr[POS_MAX_RATE];     // canonical: absorbed before every row
  Fr cin, cout;
};

// bytes of LDS a block needs: two copies of the state per lane
MSM_HD uint32_t pos_lds_bytes(uint32_t t) { return 2 * t * FR_NL * 4 * POS_LANES; }

// the state of one lane: L = POS_LANES in LDS, 1 on the host
template <uint32_t L>
struct PosState {
  uint32_t* base;
  MSM_HD void load(Fr& x, uint32_t slot) const {
#pragma unroll
    for (int q = 0; q < FR_NL; q++) x.v[q] = base[(slot * FR_NL + q) * L];
  }
  MSM_HD void store(uint32_t slot, const Fr& x) const {
#pragma unroll
    for (int q = 0; q < FR_NL; q++) base[(slot * FR_NL + q) * L] = x.v[q];
  }
};

MSM_HD int pos_top_bit(uint32_t alpha) {
  int top = 0;
  for (int b = 1; b < 16; b++)
    if ((alpha >> b) & 1) top = b;
  return top;
}

// x (lazy, carried, value^2 < 2^261 r) -> x^alpha, class M: square and multiply on a uniform exponent
template <class FR>
MSM_HD void pos_sbox(Fr& x, uint32_t alpha, int top) {
  Fr acc = x;
#pragma unroll 1
  for (int b = top - 1; b >= 0; b--) {
    fr_mul<FR>(acc, acc, acc);
    if ((alpha >> b) & 1) fr_mul<FR>(acc, x, acc);
  }
  x = acc;
}

// s + c (a canonical constant), carried; to class M first where the round asks for it; then the S-box
template <class FR>
MSM_HD void pos_ark_sbox(Fr& x, const Fr& c, bool sbox, bool reduce, const Fr& one, uint32_t alpha, int top) {
  fr_add(x, x, c);
  fr_carry(x);
  if (sbox) {
    if (reduce) fr_mul<FR>(x, x, one);
    pos_sbox<FR>(x, alpha, top);
  }
}

// one permutation of the state in copy `cur`; returns the copy that holds the result
template <class FR, class ST>
MSM_HD uint32_t pos_permute(const ST& st, const PosTab& tb, bool sparse, uint32_t cur) {
  const uint32_t t = tb.t, h = tb.rf / 2, rounds = tb.rf + tb.rp;
  const int top = pos_top_bit(tb.alpha);
  const Fr* ark = sparse ? tb.ark_s : tb.ark;
  const uint32_t* red = sparse ? tb.red_s : tb.red_d;
  Fr one;
  fr_set<FR>(one, FR::ONE);
#pragma unroll 1
  for (uint32_t r = 0; r < rounds; r++) {
    const bool full = r < h || r >= h + tb.rp;
    const uint32_t flags = red[r];
    const Fr* c = ark + (size_t)r * t;
    if (full || !sparse) {
      const uint32_t nsb = full ? t : 1;
#pragma unroll 1
      for (uint32_t e = 0; e < t; e++) {
        Fr x;
        st.load(x, cur * t + e);
        pos_ark_sbox<FR>(x, c[e], e < nsb, (flags & kPosRedSbox) != 0, one, tb.alpha, top);
        st.store(cur * t + e, x);
      }
      const Fr* m = (sparse && tb.rp && r + 1 == h) ? tb.pre : tb.mds;
#pragma unroll 1
      for (uint32_t i = 0; i < t; i++) {
        Fr acc;
        fr_zero(acc);
#pragma unroll 1
        for (uint32_t j = 0; j < t; j++) {
          Fr s, p;
          st.load(s, cur * t + j);
          fr_mul<FR>(p, s, m[i * t + j]);
          fr_add(acc, acc, p);
          fr_carry(acc);
        }
        st.store((cur ^ 1) * t + i, acc);
      }
      cur ^= 1;
    } else {
      const Fr* sp = tb.sp + (size_t)(r - h) * (2 * t - 1);
      Fr sb, acc;
      st.load(sb, cur * t);
      pos_ark_sbox<FR>(sb, c[0], true, (flags & kPosRedSbox) != 0, one, tb.alpha, top);
      fr_mul<FR>(acc, sb, sp[0]);
#pragma unroll 1
      for (uint32_t j = 1; j < t; j++) {
        Fr y, p;
        st.load(y, cur * t + j);
        if (flags & kPosRedLazy) fr_mul<FR>(y, y, one);
        fr_add(y, y, c[j]);
        fr_carry(y);
        fr_mul<FR>(p, y, sp[j]);
        fr_add(acc, acc, p);
        fr_carry(acc);
        fr_mul<FR>(p, sb, sp[t - 1 + j]);
        fr_add(y, y, p);
        fr_carry(y);
        st.store(cur * t + j, y);
      }
      st.store(cur * t, acc);
    }
  }
  return cur;
}

// sponge i of a call: the header, the row (a leading constant first), then n_out squeezed elements
template <class FR, class ST>
MSM_HD void pos_lane(const ST& st, const PosRun& p, uint64_t i) {
  const uint32_t t = p.tab.t, rate = p.tab.rate;
  const bool sparse = p.sparse != 0;
  uint32_t cur = 0, idx = p.has_header ? rate : 0;
  {
    Fr z;
    fr_zero(z);
    st.store(0, z);
#pragma unroll 1
    for (uint32_t e = 0; e < rate; e++) st.store(1 + e, p.has_header ? p.hdr[e] : z);
  }
  const uint32_t* row = p.in + i * p.row_stride * 8;
  uint32_t* dst = p.out + i * (uint64_t)p.n_out * 8;
  const uint32_t skip = p.lead != kPosLeadNone ? 1 : 0, steps = p.in_len + p.n_out;
  // one loop over the absorbed and the squeezed elements, so that the code holds the permutation once
#pragma unroll 1
  for (uint32_t k = 0; k < steps; k++) {
    if (k == p.in_len) idx = rate;          // the first squeeze always permutes
    if (idx == rate) {
      cur = pos_permute<FR>(st, p.tab, sparse, cur);
      idx = 0;
    }
    Fr s;
    st.load(s, cur * t + 1 + idx);
    if (k < p.in_len) {
      Fr x;
      if (k < skip) {
        if (p.lead == kPosLeadOne) fr_set<FR>(x, FR::ONE); else fr_zero(x);
      } else {
        uint32_t w[8];
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = row[(uint64_t)(k - skip) * 8 + q];
        fr_unpack(x, w);
        fr_mul<FR>(x, x, p.cin);
      }
      fr_add(s, s, x);
      fr_carry(s);
      st.store(cur * t + 1 + idx, s);
    } else {
      uint32_t o[8];
      fr_mul<FR>(s, s, p.cout);
      fr_pack(o, s);
      fr_canon<FR>(o);
#pragma unroll
      for (int q = 0; q < 8; q++) dst[(uint64_t)(k - p.in_len) * 8 + q] = o[q];
    }
    idx++;
  }
}

// ---- what create derives on the host ----------------------------------------------------------------------------------------------

// canonical host arithmetic
template <class FR>
struct PosField {
  static Fr one() {
    Fr o;
    fr_set<FR>(o, FR::ONE);
    return o;
  }
  static Fr mul(const Fr& a, const Fr& b) {
    Fr r;
    fr_mul<FR>(r, a, b);
    fr_reduce<FR>(r);
    return r;
  }
  static Fr canon(Fr x) {   // lazy, limbs below 2^31 -> canonical
    fr_carry(x);
    fr_mul<FR>(x, x, one());
    fr_reduce<FR>(x);
    return x;
  }
  static Fr add(const Fr& a, const Fr& b) {
    Fr r;
    fr_add(r, a, b);
    return canon(r);
  }
  static Fr sub(const Fr& a, const Fr& b) {
    Fr r;
    fr_sub<FR>(r, a, b);
    return canon(r);
  }
  static bool is_zero(const Fr& a) {
    uint32_t x = 0;
    for (int i = 0; i < FR_NL; i++) x |= a.v[i];
    return x == 0;
  }
  static Fr inv(const Fr& a) {
    Fr r;
    fr_inv<FR>(r, a);
    return r;
  }
};

// the inverse of the m x m matrix a (row-major) by Gauss-Jordan elimination; false when a is singular
template <class FR>
bool pos_invert(std::vector<Fr>& out, std::vector<Fr> a, uint32_t m) {
  using F = PosField<FR>;
  Fr zero;
  fr_zero(zero);
  out.assign((size_t)m * m, zero);
  for (uint32_t i = 0; i < m; i++) out[(size_t)i * m + i] = F::one();
  for (uint32_t col = 0; col < m; col++) {
    uint32_t piv = col;
    while (piv < m && F::is_zero(a[(size_t)piv * m + col])) piv++;
    if (piv == m) return false;
    for (uint32_t j = 0; j < m; j++) {
      std::swap(a[(size_t)piv * m + j], a[(size_t)col * m + j]);
      std::swap(out[(size_t)piv * m + j], out[(size_t)col * m + j]);
    }
    const Fr s = F::inv(a[(size_t)col * m + col]);
    for (uint32_t j = 0; j < m; j++) {
      a[(size_t)col * m + j] = F::mul(a[(size_t)col * m + j], s);
      out[(size_t)col * m + j] = F::mul(out[(size_t)col * m + j], s);
    }
    for (uint32_t i = 0; i < m; i++) {
      if (i == col || F::is_zero(a[(size_t)i * m + col])) continue;
      const Fr f = a[(size_t)i * m + col];
      for (uint32_t j = 0; j < m; j++) {
        a[(size_t)i * m + j] = F::sub(a[(size_t)i * m + j], F::mul(f, a[(size_t)col * m + j]));
        out[(size_t)i * m + j] = F::sub(out[(size_t)i * m + j], F::mul(f, out[(size_t)col * m + j]));
      }
    }
  }
  return true;
}

// everything a handle keeps: the caller's parameters, the sparse form, the reductions and the product counts of both forms
struct PosPlan {
  uint32_t t = 0, rate = 0, alpha = 0, rf = 0, rp = 0;
  std::vector<Fr> ark, mds, ark_s, pre, sp;
  std::vector<uint32_t> red_d, red_s;
  uint64_t products_d = 0, products_s = 0;
};

// 2^261 / r
template <class FR>
double pos_headroom() {
  double r = 0;
  for (int i = FR_NL - 1; i >= 0; i--) r = r * (double)(1u << FR_LB) + (double)FR::P[i];
  double k = 1;
  for (int i = 0; i < FR_NL * FR_LB; i++) k *= 2;
  return k / r;
}

// The bounds of one permutation, in units of r, round by round; sets the reductions of each round and counts the products.  The
// state enters below t (1 + 2 / K) + 2 per element (the sums of the last matrix and an absorbed class-M element) and must leave below
// t (1 + 2 / K): the margins 0.95 and 0.9 cover the carried form's excess.  False when a bound cannot be kept (no field here).
inline bool pos_schedule(std::vector<uint32_t>& red, uint64_t& products, uint32_t t, uint32_t alpha, uint32_t rf, uint32_t rp, bool sparse, double K) {
  const uint32_t h = rf / 2, rounds = rf + rp;
  const double sq_limit = 0.95 * K, lazy_limit = 0.9 * K, leave = t * (1 + 2 / K);
  uint32_t sbox_products = 0;
  for (int b = pos_top_bit(alpha) - 1; b >= 0; b--) sbox_products += 1 + ((alpha >> b) & 1);
  double b[POS_MAX_T];
  for (uint32_t e = 0; e < t; e++) b[e] = leave + 2;
  red.assign(rounds, 0);
  products = 0;
  auto sbox = [&](double x, uint32_t& flags, bool may_flag) {   // the bound after ark, reduction and S-box
    if (x * x >= sq_limit) {
      if (may_flag) flags |= kPosRedSbox;
      x = 1 + x / K;
    }
    return 1 + 2 * x / K;
  };
  for (uint32_t r = 0; r < rounds; r++) {
    const bool full = r < h || r >= h + rp;
    uint32_t flags = 0;
    if (full || !sparse) {
      const uint32_t nsb = full ? t : 1;
      for (uint32_t e = 0; e < nsb; e++)
        if ((b[e] + 1) * (b[e] + 1) >= sq_limit) flags |= kPosRedSbox;
      double sum = 0;
      for (uint32_t e = 0; e < t; e++) {
        double x = b[e] + 1;
        if (x >= lazy_limit) return false;
        if (e < nsb) {
          if (flags & kPosRedSbox) x = 1 + x / K;
          if (x * x >= sq_limit) return false;
          x = 1 + 2 * x / K;
        }
        sum += 1 + x / K;
      }
      products += (uint64_t)nsb * (sbox_products + ((flags & kPosRedSbox) ? 1 : 0)) + (uint64_t)t * t;
      for (uint32_t e = 0; e < t; e++) b[e] = sum;
    } else {
      // what the elements 1 .. t - 1 reach in this round without a reduction: y = s + c, then y + w sb
      for (uint32_t e = 1; e < t; e++)
        if (b[e] + 3 >= lazy_limit) flags |= kPosRedLazy;
      double x0 = b[0] + 1;
      if (x0 >= lazy_limit) return false;
      // the sum out_0 of the NEXT round's S-box input is judged there; here only this round's
      uint32_t f0 = 0;
      const double sb = sbox(x0, f0, true);
      flags |= f0;
      double out0 = 1 + sb / K;
      for (uint32_t e = 1; e < t; e++) {
        double y = b[e];
        if (flags & kPosRedLazy) y = 1 + y / K;
        y += 1;
        out0 += 1 + y / K;
        b[e] = y + 1 + sb / K;
        if (b[e] >= lazy_limit) return false;
      }
      b[0] = out0;
      products += sbox_products + ((flags & kPosRedSbox) ? 1 : 0) + (2 * t - 1) + ((flags & kPosRedLazy) ? t - 1 : 0);
    }
    red[r] = flags;
  }
  for (uint32_t e = 0; e < t; e++)
    if (b[e] > leave) return false;
  return true;
}

// ark: (rf + rp) * t and mds: t * t canonical elements.  False with a message when some N^ is singular.
template <class FR>
bool pos_build(PosPlan& pl, uint32_t rate, uint32_t alpha, uint32_t rf, uint32_t rp, const Fr* ark, const Fr* mds, char* msg, size_t msg_len) {
  using F = PosField<FR>;
  const uint32_t t = rate + 1, h = rf / 2, rounds = rf + rp, m = t - 1;
  pl.t = t;
  pl.rate = rate;
  pl.alpha = alpha;
  pl.rf = rf;
  pl.rp = rp;
  pl.ark.assign(ark, ark + (size_t)rounds * t);
  pl.mds.assign(mds, mds + (size_t)t * t);
  pl.ark_s = pl.ark;
  pl.pre = pl.mds;
  pl.sp.assign((size_t)rp * (2 * t - 1), Fr{});
  std::vector<Fr> N = pl.mds, hat((size_t)m * m), inv, next((size_t)t * t);
  for (uint32_t k = h + rp; k-- > h;) {
    for (uint32_t i = 0; i < m; i++)
      for (uint32_t j = 0; j < m; j++) hat[(size_t)i * m + j] = N[(size_t)(i + 1) * t + j + 1];
    if (!pos_invert<FR>(inv, hat, m)) {
      snprintf(msg, msg_len, "partial round %u: the matrix without row and column 0 is singular, the sparse form does not exist", k);
      return false;
    }
    Fr* sp = pl.sp.data() + (size_t)(k - h) * (2 * t - 1);
    sp[0] = N[0];
    for (uint32_t j = 0; j < m; j++) {
      Fr acc;
      fr_zero(acc);
      for (uint32_t q = 0; q < m; q++) acc = F::add(acc, F::mul(N[q + 1], inv[(size_t)q * m + j]));
      sp[1 + j] = acc;
      sp[t + j] = N[(size_t)(j + 1) * t];
    }
    // N' c_k and N' M
    Fr* c = pl.ark_s.data() + (size_t)k * t;
    std::vector<Fr> c1(m);
    for (uint32_t i = 0; i < m; i++) {
      Fr acc;
      fr_zero(acc);
      for (uint32_t q = 0; q < m; q++) acc = F::add(acc, F::mul(hat[(size_t)i * m + q], c[q + 1]));
      c1[i] = acc;
    }
    for (uint32_t i = 0; i < m; i++) c[i + 1] = c1[i];
    for (uint32_t j = 0; j < t; j++) next[j] = pl.mds[j];
    for (uint32_t i = 0; i < m; i++)
      for (uint32_t j = 0; j < t; j++) {
        Fr acc;
        fr_zero(acc);
        for (uint32_t q = 0; q < m; q++) acc = F::add(acc, F::mul(hat[(size_t)i * m + q], pl.mds[(size_t)(q + 1) * t + j]));
        next[(size_t)(i + 1) * t + j] = acc;
      }
    N = next;
  }
  pl.pre = N;
  const double K = pos_headroom<FR>();
  if (!pos_schedule(pl.red_d, pl.products_d, t, alpha, rf, rp, false, K) || !pos_schedule(pl.red_s, pl.products_s, t, alpha, rf, rp, true, K)) {
    snprintf(msg, msg_len, "the lazy bounds of the rounds cannot be kept for this field and state width");
    return false;
  }
  return true;
}

// the table in one buffer: the five vectors of elements, then the two lists of reductions
MSM_HD size_t pos_table_elems(uint32_t t, uint32_t rf, uint32_t rp) { return (size_t)2 * (rf + rp) * t + (size_t)2 * t * t + (size_t)rp * (2 * t - 1); }
MSM_HD size_t pos_table_bytes(uint32_t t, uint32_t rf, uint32_t rp) { return pos_table_elems(t, rf, rp) * sizeof(Fr) + (size_t)2 * (rf + rp) * 4; }

inline void pos_table_fill(std::vector<uint8_t>& img, const PosPlan& pl) {
  img.assign(pos_table_bytes(pl.t, pl.rf, pl.rp), 0);
  uint8_t* at = img.data();
  for (const std::vector<Fr>* v : {&pl.ark, &pl.mds, &pl.ark_s, &pl.pre, &pl.sp}) {
    if (!v->empty()) memcpy(at, v->data(), v->size() * sizeof(Fr));
    at += v->size() * sizeof(Fr);
  }
  for (const std::vector<uint32_t>* v : {&pl.red_d, &pl.red_s}) {
    memcpy(at, v->data(), v->size() * 4);
    at += v->size() * 4;
  }
}

// the pointers of a table that lies at `base` in the layout of pos_table_fill
inline PosTab pos_table_at(const void* base, const PosPlan& pl) {
  const uint32_t t = pl.t, rounds = pl.rf + pl.rp;
  PosTab tb{};
  const Fr* e = (const Fr*)base;
  tb.ark = e;
  tb.mds = tb.ark + (size_t)rounds * t;
  tb.ark_s = tb.mds + (size_t)t * t;
  tb.pre = tb.ark_s + (size_t)rounds * t;
  tb.sp = tb.pre + (size_t)t * t;
  tb.red_d = (const uint32_t*)(tb.sp + (size_t)pl.rp * (2 * t - 1));
  tb.red_s = tb.red_d + rounds;
  tb.t = t;
  tb.rate = pl.rate;
  tb.alpha = pl.alpha;
  tb.rf = pl.rf;
  tb.rp = pl.rp;
  return tb;
}

// the argument limits of create, in the order of the header: 0 or the message
inline const char* pos_check_shape(uint32_t rate, uint32_t alpha, uint32_t rf, uint32_t rp) {
  if (rate < 1 || rate > POS_MAX_RATE) return "the rate must be 1 .. 8";
  if (alpha < 3 || alpha >= (1u << 16) || !(alpha & 1)) return "alpha must be odd, 3 .. 65535";
  if (rf < 2 || (rf & 1) || rf > POS_MAX_ROUNDS) return "full_rounds must be even, 2 .. 4096";
  if (rp > POS_MAX_ROUNDS) return "partial_rounds exceed 4096";
  return nullptr;
}

// The launches of a Merkle tree of n_leaves >= 1 leaves of leaf_len elements, shared by the engine and the host build.  RUN has
// hash(PosRun) and fill(uint32_t* first, uint64_t count) -- copy element `first` to the count - 1 elements behind it.  `base` holds the
// table, cin / cout and sparse; hdr_leaf / hdr_node are the two headers [domain, length, 0 ..].
template <class RUN>
void pos_merkle_chain(RUN& run, const PosRun& base, uint32_t* tree, const uint32_t* leaves, uint64_t n_leaves, uint32_t leaf_len, const Fr* hdr_leaf,
                      const Fr* hdr_node, const uint32_t* zeros) {
  uint64_t P = 1;
  while (P < n_leaves) P *= 2;
  PosRun p = base;
  p.n_out = 1;
  p.has_header = 1;
  // the leaf hashes
  for (uint32_t e = 0; e < base.tab.rate; e++) p.hdr[e] = hdr_leaf[e];
  p.in = leaves;
  p.out = tree + (P - 1) * 8;
  p.n = n_leaves;
  p.row_stride = leaf_len;
  p.in_len = leaf_len + 1;
  p.lead = kPosLeadZero;
  run.hash(p);
  for (uint32_t e = 0; e < base.tab.rate; e++) p.hdr[e] = hdr_node[e];
  p.in_len = 3;
  p.lead = kPosLeadOne;
  if (P > n_leaves) {   // the empty hash, once, then copied
    p.in = zeros;
    p.out = tree + (P - 1 + n_leaves) * 8;
    p.n = 1;
    p.row_stride = 0;
    run.hash(p);
    run.fill(p.out, P - n_leaves);
  }
  // one launch per level, from the level above the leaves to the root
  p.row_stride = 2;
  for (uint64_t m = P / 2; m >= 1; m /= 2) {
    p.in = tree + (2 * m - 1) * 8;
    p.out = tree + (m - 1) * 8;
    p.n = m;
    run.hash(p);
  }
}

#if defined(__HIPCC__)
template <class FR>
__global__ void __launch_bounds__(POS_LANES) k_poseidon_hash(PosRun p) {
  extern __shared__ uint32_t pos_lds[];
  const uint64_t i = (uint64_t)blockIdx.x * POS_LANES + threadIdx.x;
  if (i >= p.n) return;
  const PosState<POS_LANES> st{pos_lds + threadIdx.x};
  pos_lane<FR>(st, p, i);
}
#endif

}  // namespace msm
