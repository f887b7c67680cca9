// fr.hpp -- arithmetic of the two scalar fields (BLS12-377 Fr, 253 bits; BLS12-381 Fr, 255 bits) for gfx950 and the host.
//
// Shape: 9 limbs of 29 bits, Montgomery radix R = 2^261, by the argument of fp28.hpp: v_mad_u64_u32 issues like an add-with-carry,
// so an unsaturated radix whose product-scanning column (9 a*b + 9 m*r terms of < 2^60) fits one 64-bit accumulator needs no carry
// instruction at all.  9 x 29 takes 81 + 72 multiply-adds per product (r = 1 mod 2^29 for both fields, so the nine m_k * r_0 terms
// are plain adds); 10 x 28 would take 100 + 90, and saturated 8 x 32 CIOS 64 + 64 + 8 but two carry instructions per multiply-add.
//
// Representation.  value(a) = sum a.v[i] * 2^(29 i); an element x is held as x * R mod r, lazily reduced.
//   "normalised": v[0..7] < 2^29 (v[8] holds what is left).   "carried": v[0..7] < 2^29 + 8 (fr_carry of limbs < 2^32).
//   fr_mul(a, b): limbs of a < 2^31, b normalised and value(b) < r (a table entry or a constant), value(a) < 2^261.
//       result normalised, value < r + value(a) * value(b) / R < 2r      ("class M").
//   fr_sub(a, t) = a + BIAS4 - t for a class-M t: limb-wise, no borrow; the value grows by 4r.
// BLS12-381's r is 7.25 * 2^252, so 2^261 / r = 70.6 (BLS12-377: 447): a butterfly chain t = w * b; a' = a + t; b' = a - t + 4r adds at
// most 4r per level, and a pass of up to 10 levels that starts below 2r stays below 42r -- inside what fr_mul accepts, for both
// fields (tools/limb_bounds_fr.py prints the margins; the host build checks every product and subtraction, MSM_CHECK).
// Between passes an element is stored as 256 bits: always a class-M value, 2r < 2^256.
//
// The 32-byte ABI is arkworks' (a * 2^256 mod r) or the plain integer; either is read for ANY 256-bit input (one product by
// CIN_* brings it to class M) and written canonical (one product by COUT_*, then one conditional subtraction).
#pragma once
#include "fp28.hpp"   // MSM_HD, MSM_CHECK

namespace msm {

constexpr int FR_NL = 9;
constexpr int FR_LB = 29;
constexpr uint32_t FR_MASK = (1u << FR_LB) - 1;

#include "fr_consts.inc"

struct Fr {
  uint32_t v[FR_NL];
};

template <class FR, class A>
MSM_HD void fr_set(Fr& r, const A& limbs) {
#pragma unroll
  for (int i = 0; i < FR_NL; i++) r.v[i] = limbs[i];
}

MSM_HD void fr_zero(Fr& r) {
#pragma unroll
  for (int i = 0; i < FR_NL; i++) r.v[i] = 0;
}

// r = a * b / R (mod r), class M.  Product scanning: one 64-bit accumulator per column, m_k = -col mod 2^29 because r_0 = 1.
template <class FR>
MSM_HD void fr_mul(Fr& r, const Fr& a, const Fr& b) {
  static_assert(FR::P[0] == 1 && FR::NINV == FR_MASK, "the Montgomery step relies on r = 1 (mod 2^29)");
  constexpr int N = FR_NL;
  uint32_t m[N];
  Fr t;
  uint64_t col = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    MSM_CHECK(a.v[i] < (1u << 31) && b.v[i] < (1u << 29) + 8);
  }
#pragma unroll
  for (int k = 0; k < N; k++) {
    MSM_CHECK_COL_BEGIN();
#pragma unroll
    for (int i = 0; i <= k; i++) {
      col += (uint64_t)a.v[i] * b.v[k - i];
      MSM_CHECK_COL_ADD((unsigned __int128)a.v[i] * b.v[k - i]);
    }
#pragma unroll
    for (int i = 0; i < k; i++) {
      col += (uint64_t)m[i] * FR::P[k - i];
      MSM_CHECK_COL_ADD((unsigned __int128)m[i] * FR::P[k - i]);
    }
    m[k] = (0u - (uint32_t)col) & FR_MASK;
    col += m[k];
    MSM_CHECK_COL_ADD(m[k]);
    MSM_CHECK_COL_END(col);
    MSM_CHECK(((uint32_t)col & FR_MASK) == 0);
    col >>= FR_LB;
  }
#pragma unroll
  for (int k = N; k < 2 * N - 1; k++) {
    MSM_CHECK_COL_BEGIN();
#pragma unroll
    for (int i = k - (N - 1); i < N; i++) {
      col += (uint64_t)a.v[i] * b.v[k - i];
      MSM_CHECK_COL_ADD((unsigned __int128)a.v[i] * b.v[k - i]);
    }
#pragma unroll
    for (int i = k - (N - 1); i < N; i++) {
      col += (uint64_t)m[i] * FR::P[k - i];
      MSM_CHECK_COL_ADD((unsigned __int128)m[i] * FR::P[k - i]);
    }
    MSM_CHECK_COL_END(col);
    t.v[k - N] = (uint32_t)col & FR_MASK;
    col >>= FR_LB;
  }
  MSM_CHECK(col <= 2 * (uint64_t)FR::P[N - 1] + 1);   // value < 2r
  t.v[N - 1] = (uint32_t)col;
  r = t;
}

// limb-wise sum; the caller carries before limbs can reach 2^31
MSM_HD void fr_add(Fr& r, const Fr& a, const Fr& b) {
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    MSM_CHECK((uint64_t)a.v[i] + b.v[i] < (1ull << 32));
    r.v[i] = a.v[i] + b.v[i];
  }
}

// a - t + 4r for a class-M t (normalised, value < 2r): every limb of BIAS4 covers the limb of t it meets
template <class FR>
MSM_HD void fr_sub(Fr& r, const Fr& a, const Fr& t) {
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    MSM_CHECK(FR::BIAS4[i] >= t.v[i]);
    MSM_CHECK((uint64_t)a.v[i] + FR::BIAS4[i] - t.v[i] < (1ull << 32));
    r.v[i] = a.v[i] + (FR::BIAS4[i] - t.v[i]);
  }
}

// one parallel carry pass: limbs < 2^32 in, limbs 0..7 < 2^29 + 8 out, the value unchanged
MSM_HD void fr_carry(Fr& a) {
  uint32_t hi[FR_NL];
#pragma unroll
  for (int i = 0; i < FR_NL - 1; i++) hi[i] = a.v[i] >> FR_LB;
  MSM_CHECK((uint64_t)a.v[FR_NL - 1] + hi[FR_NL - 2] < (1ull << 31));
  a.v[FR_NL - 1] += hi[FR_NL - 2];
#pragma unroll
  for (int i = FR_NL - 2; i > 0; i--) a.v[i] = (a.v[i] & FR_MASK) + hi[i - 1];
  a.v[0] &= FR_MASK;
}

// 8 x 32-bit words (any 256-bit value) <-> 9 normalised limbs
MSM_HD void fr_unpack(Fr& r, const uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < FR_NL; i++) {
    const int bit = FR_LB * i, j = bit >> 5, sh = bit & 31;
    uint64_t x = w[j];
    if (j + 1 < 8) x |= (uint64_t)w[j + 1] << 32;
    r.v[i] = (uint32_t)(x >> sh) & FR_MASK;
  }
}

// normalised limbs, value < 2^256
MSM_HD void fr_pack(uint32_t (&w)[8], const Fr& a) {
  MSM_CHECK(a.v[FR_NL - 1] < (1u << 24));
#pragma unroll
  for (int j = 0; j < 8; j++) {
    // word j holds bits 32 j .. 32 j + 31: the tail of limb i0 and the head of limb i0 + 1 (and of i0 + 2 when limb i0 ends early)
    const int i0 = (32 * j) / FR_LB, sh = 32 * j - FR_LB * i0;
    MSM_CHECK(a.v[i0] <= FR_MASK || i0 == FR_NL - 1);
    uint64_t x = (uint64_t)a.v[i0] >> sh;
    if (i0 + 1 < FR_NL) x |= (uint64_t)a.v[i0 + 1] << (FR_LB - sh);
    if (i0 + 2 < FR_NL && 2 * FR_LB - sh < 32) x |= (uint64_t)a.v[i0 + 2] << (2 * FR_LB - sh);
    w[j] = (uint32_t)x;
  }
}

// value < 2r -> value < r
template <class FR>
MSM_HD void fr_canon(uint32_t (&w)[8]) {
  int64_t b = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    b += (int64_t)w[j] - FR::P32[j];
    b >>= 32;
  }
  const uint32_t keep = b ? 0u : 0xffffffffu;   // 0: w < r
  b = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    b += (int64_t)w[j] - (FR::P32[j] & keep);
    w[j] = (uint32_t)b;
    b >>= 32;
  }
  MSM_CHECK(b == 0);
}

template <class FR>
MSM_HD void fr_const(Fr& c, int which) {   // 0 CIN_MONT, 1 CIN_NORM, 2 COUT_MONT, 3 COUT_NORM
#pragma unroll
  for (int i = 0; i < FR_NL; i++)
    c.v[i] = which == 0 ? FR::CIN_MONT[i] : which == 1 ? FR::R2[i] : which == 2 ? FR::COUT_MONT[i] : FR::COUT_NORM[i];
}

// ABI words (any 256-bit value; normal != 0: a plain integer, else an arkworks image) -> class M
template <class FR>
MSM_HD void fr_from_abi(Fr& r, const uint32_t (&w)[8], bool normal) {
  Fr x, c;
  fr_unpack(x, w);
  fr_const<FR>(c, normal ? 1 : 0);
  fr_mul<FR>(r, x, c);
}

// any mul input -> canonical ABI words
template <class FR>
MSM_HD void fr_to_abi(uint32_t (&w)[8], const Fr& a, bool normal) {
  Fr x, c;
  fr_const<FR>(c, normal ? 3 : 2);
  fr_mul<FR>(x, a, c);
  fr_pack(w, x);
  fr_canon<FR>(w);
}

// class M -> the canonical representative, still limbs of x * R (what a table holds)
template <class FR>
MSM_HD void fr_reduce(Fr& a) {
  uint32_t w[8];
  fr_pack(w, a);
  fr_canon<FR>(w);
  fr_unpack(a, w);
}

// base^e for e < 2^32, canonical; base canonical
template <class FR>
MSM_HD void fr_pow_u32(Fr& r, const Fr& base, uint32_t e) {
  Fr acc, sq = base;
  fr_set<FR>(acc, FR::ONE);
  for (; e; e >>= 1) {
    if (e & 1) {
      fr_mul<FR>(acc, acc, sq);
      fr_reduce<FR>(acc);
    }
    fr_mul<FR>(sq, sq, sq);
    fr_reduce<FR>(sq);
  }
  r = acc;
}

}  // namespace msm
