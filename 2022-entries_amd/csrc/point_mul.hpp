// point_mul.hpp -- batch variable-base scalar multiplication: out[i] = s_i * P_i, every point with a scalar of its own, or one
// scalar k for all points.
//
// What it replaces: ARK ec/src/lib.rs:188,294,305-319 (AffineRepr::mul_bigint, mul_by_cofactor, mul_by_cofactor_inv) and
// ec/src/models/short_weierstrass.rs:413-422, one CPU double-and-add per point, followed by batch_normalization_into_affine -- what
// a ceremony contribution runs over a transcript.  Only the names and the contract are arkworks'; the algorithm is the device's:
//
//   table    one lane per point: 1P .. 2^(w-1) P in XYZZ (one xyzz_dbl, then xyzz_madd of P per further entry: P is affine), entry e
//            of point i at [e * n + i] so that the lanes of a wave touch neighbouring records.  A flagged infinity gives infinities;
//            a point of small order runs into acc == +-P and into infinity here, which the general xyzz_madd handles.
//            Launch<E>::pre_normalize as it stands turns the entries into AffineDev records (all-zero = infinity, fixed_base.hpp).
//   mul      one lane per point: the scalar as ceil(257 / w) SIGNED w-bit digits, |d| <= 2^(w-1), walked from the top with a rolled
//            loop -- w doublings, then xyzz_madd(acc, table[|d|], d < 0).  The digits are Booth's: digit j is a function of the
//            w + 1 bits [w j - 1, w j + w) alone (pm_digit), so the walk from the top needs no carry chain from the bottom and the
//            digit comes out of the scalar's registers by wave-uniform word selects (check_scalar_word).  The 257th bit is the sign
//            position of the top window.  The loop starts at the highest window that is non-zero in any lane of the wave (one
//            wave-wide maximum of the scalars' bit lengths), so a batch of 64- or 128-bit challenges costs what its length costs.
//   uniform  one scalar k of up to 512 bits for all points: the host recodes k into non-adjacent form (at most 513 signed digits, two
//            bit arrays in the kernel arguments), the kernel runs `dbl; if digit: madd(+-P)` rolled from the top digit.  Every test
//            is wave-uniform; no table, no work memory beyond the output staging.
//   output   k_fb_normalize of fixed_base.hpp as it stands.
//
// No curve test and no subgroup test (mul_bigint has none).  A record that is on no curve gives an unspecified result, but every
// memory access is a function of the lane index and the digits alone, so the call finishes without a fault.
// Every per-element step is an MSM_HD function, so the host build (host_test_api.cpp, ht_pm_*) runs the same code under MSM_CHECK.
// Limb bounds: as in fixed_base.hpp -- xyzz_dbl / xyzz_madd re-establish the stored-point invariants from those invariants alone and
// the table records are canonical, so chains of any length hold them.
#pragma once
#include "fixed_base.hpp"   // fb_record_is_inf, the output normalisation; check_scalar_word, CheckConsts, fr_from_montgomery through it

namespace msm {

constexpr uint32_t PM_MAX_WINDOW = 6;
constexpr uint32_t PM_DEFAULT_WINDOW = 4;
constexpr uint32_t PM_NAF_WORDS = 17;   // 513 digits of the non-adjacent form of a 512-bit scalar

MSM_HD uint32_t pm_digits(uint32_t w) { return (257 + w - 1) / w; }
MSM_HD uint32_t pm_table_entries(uint32_t w) { return 1u << (w - 1); }

// Signed digit j of the 256-bit scalar s for window size w <= 6 (Booth recoding):
//   d_j = b(w j - 1) + sum_{k < w - 1} b(w j + k) 2^k - b(w j + w - 1) 2^(w - 1),   b(-1) = b(256...) = 0,
// so sum_j d_j 2^(w j) = s (the -2^(w j + w - 1) of window j and the +2^(w (j + 1)) of window j + 1 leave +2^(w j + w - 1)), and
// |d_j| <= 2^(w-1).  j is wave-uniform: the two words come out of the register array by uniform selects, never through memory.
MSM_HD int32_t pm_digit(const uint32_t (&s)[8], uint32_t j, uint32_t w) {
  uint64_t v;
  if (j == 0) {
    v = (uint64_t)s[0] << 1;
  } else {
    const uint32_t bit = j * w - 1, wi = bit >> 5, sh = bit & 31;
    const uint32_t lo = check_scalar_word<8>(s, (int)wi), hi = check_scalar_word<8>(s, (int)wi + 1);   // word 8 and up do not exist: 0
    v = (((uint64_t)hi << 32) | lo) >> sh;
  }
  const uint32_t t = (uint32_t)v & ((2u << w) - 1);   // w + 1 bits
  return (int32_t)((t + 1) >> 1) - (int32_t)(((t >> w) & 1) << w);
}

// bits of s: 0 for s == 0, else 1 + the index of the top set bit
MSM_HD uint32_t pm_bit_length(const uint32_t (&s)[8]) {
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t b = 0;
    for (uint32_t x = s[k]; x; x >>= 1) b++;
    if (s[k]) n = 32u * k + b;
  }
  return n;
}
// the highest window a scalar of `bits` bits can have a non-zero digit in (its top bit is the carry-in b(w j - 1) of window
// bits / w, or lies inside a lower one); the loop of pm_windowed_mul starts there
MSM_HD uint32_t pm_top_window(uint32_t bits, uint32_t w) { return bits / w; }

// The point as the caller holds it: coordinates by from_abi, the flag byte authoritative.
template <class E>
MSM_HD void pm_load_point(AffineT<typename E::T>& P, const uint32_t* img, const typename E::Md& md) {
  E::from_abi(P.x, img, md);
  E::from_abi(P.y, img + E::WORDS, md);
}

// ---- table build -----------------------------------------------------------------------------------------------------------
// out[e * pitch] = (e + 1) P, e < entries
template <class E>
MSM_HD void pm_table(XyzzT<typename E::T>* out, size_t pitch, const uint32_t* img, uint8_t flag, uint32_t entries, const typename E::Md& md) {
  using El = typename E::T;
  XyzzT<El> acc;
  if (flag) {
    xyzz_set_inf<E>(acc);
    for (uint32_t e = 0; e < entries; e++) out[e * pitch] = acc;
    return;
  }
  AffineT<El> P;
  pm_load_point<E>(P, img, md);
  xyzz_from_affine<E>(acc, P, false);
  out[0] = acc;
  if (entries < 2) return;
  xyzz_dbl<E>(acc, md);   // (a point of order 2 has y = 0: ZZ = 0, infinity, with no special case)
  out[pitch] = acc;
#pragma unroll 1
  for (uint32_t e = 2; e < entries; e++) {
    xyzz_madd<E>(acc, P, false, false, md);
    out[e * pitch] = acc;
  }
}

// ---- the hot path --------------------------------------------------------------------------------------------------------------
// acc = s * P through P's table: records table[e * pitch], e < 2^(w-1).  `top`: the window the walk starts at, at least
// pm_top_window of this scalar (the kernel passes the maximum over the wave; the host build the scalar's own).  The record of the
// next window is fetched while the doublings and the addition of the current one run where the register file has room for it
// (E::PREFETCH_BASE, as in fb_windowed_mul).
template <class E>
MSM_HD void pm_windowed_mul(XyzzT<typename E::T>& acc, const AffineDevT<typename E::T>* __restrict__ table, size_t pitch, const uint32_t (&s)[8],
                            uint32_t w, uint32_t top, const typename E::Md& md) {
  using El = typename E::T;
  xyzz_set_inf<E>(acc);
  if constexpr (E::PREFETCH_BASE) {
    int32_t d = pm_digit(s, top, w);
    uint32_t a = d < 0 ? (uint32_t)-d : (uint32_t)d;
    AffineT<El> cur = table[(a ? a - 1 : 0) * pitch].p;   // (a zero digit fetches entry 0: an address inside the table, a value nobody uses)
#pragma unroll 1
    for (int j = (int)top; j >= 0; j--) {
      const int32_t dn = j > 0 ? pm_digit(s, (uint32_t)j - 1, w) : 0;
      const uint32_t an = dn < 0 ? (uint32_t)-dn : (uint32_t)dn;
      const AffineT<El> nxt = table[(an ? an - 1 : 0) * pitch].p;
      if (!xyzz_is_inf<E>(acc)) {
#pragma unroll 1
        for (uint32_t k = 0; k < w; k++) xyzz_dbl<E>(acc, md);
      }
      if (d != 0 && !fb_record_is_inf(cur)) xyzz_madd<E>(acc, cur, d < 0, false, md);
      cur = nxt;
      d = dn;
    }
  } else {
#pragma unroll 1
    for (int j = (int)top; j >= 0; j--) {
      if (!xyzz_is_inf<E>(acc)) {
#pragma unroll 1
        for (uint32_t k = 0; k < w; k++) xyzz_dbl<E>(acc, md);
      }
      const int32_t d = pm_digit(s, (uint32_t)j, w);
      if (d == 0) continue;
      const AffineT<El> a = table[((d < 0 ? (uint32_t)-d : (uint32_t)d) - 1) * pitch].p;
      if (!fb_record_is_inf(a)) xyzz_madd<E>(acc, a, d < 0, false, md);
    }
  }
}

// ---- one scalar for all points -------------------------------------------------------------------------------------------------
// k in non-adjacent form: digit i is non-zero iff bit i of nz, negative iff bit i of neg; top = index of the highest non-zero digit,
// -1 for k = 0.  Passed by value in the kernel arguments.
struct PmNaf {
  uint32_t nz[PM_NAF_WORDS];
  uint32_t neg[PM_NAF_WORDS];
  int32_t top;
};

// k = sum w[i] 2^(32 i), nw <= 16 words -> NAF: k = sum_i d_i 2^i, d_i in {-1, 0, 1}, no two adjacent digits non-zero
inline void pm_naf_recode(PmNaf& out, const uint32_t* w, uint32_t nw) {
  uint32_t k[PM_NAF_WORDS + 1] = {0};
  for (uint32_t i = 0; i < nw && i < 16; i++) k[i] = w[i];
  for (uint32_t i = 0; i < PM_NAF_WORDS; i++) out.nz[i] = out.neg[i] = 0;
  out.top = -1;
  for (uint32_t i = 0; i < 32 * PM_NAF_WORDS; i++) {
    // k holds the rest of the scalar, shifted right by i; odd: the digit is 2 - (k mod 4), and k -= digit
    if (k[0] & 1) {
      out.nz[i >> 5] |= 1u << (i & 31);
      out.top = (int32_t)i;
      if (k[0] & 2) {   // digit -1: k += 1
        out.neg[i >> 5] |= 1u << (i & 31);
        for (uint32_t j = 0; j <= PM_NAF_WORDS; j++)
          if (++k[j]) break;
      } else {
        k[0] &= ~1u;
      }
    }
    for (uint32_t j = 0; j < PM_NAF_WORDS; j++) k[j] = (k[j] >> 1) | (k[j + 1] << 31);
    k[PM_NAF_WORDS] >>= 1;
  }
}

// acc = k * P for the point image `img`; the digit tests are the same for every point
template <class E>
MSM_HD void pm_mul_uniform(XyzzT<typename E::T>& acc, const uint32_t* img, uint8_t flag, const PmNaf& naf, const typename E::Md& md) {
  using El = typename E::T;
  if (flag || naf.top < 0) {
    xyzz_set_inf<E>(acc);
    return;
  }
  AffineT<El> P;
  pm_load_point<E>(P, img, md);
  xyzz_from_affine<E>(acc, P, ((naf.neg[naf.top >> 5] >> (naf.top & 31)) & 1) != 0);
#pragma unroll 1
  for (int i = naf.top - 1; i >= 0; i--) {
    xyzz_dbl<E>(acc, md);   // (infinity stays infinity: ZZ = 0 is absorbing)
    if ((naf.nz[i >> 5] >> (i & 31)) & 1) xyzz_madd<E>(acc, P, ((naf.neg[i >> 5] >> (i & 31)) & 1) != 0, false, md);
  }
}

#if defined(__HIPCC__)
// one lane per point; in: Affine images `stride` bytes apart; out: entries * n XYZZ, entry-major
template <class E>
__global__ void __launch_bounds__(256) k_pm_table(const uint8_t* __restrict__ in, size_t stride, uint32_t n, uint32_t entries,
                                                  XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  constexpr int W = E::WORDS;
  const uint8_t* p = in + (size_t)i * stride;
  uint32_t rec[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) rec[k] = reinterpret_cast<const uint32_t*>(p)[k];
  pm_table<E>(reinterpret_cast<XyzzT<typename E::T>*>(out + i), n, rec, p[8 * W], entries, md);
}

// one lane per point; table: 2^(w-1) * n records, entry-major.  Lanes past n keep the wave whole for the maximum and do nothing else.
template <class E>
__global__ void __launch_bounds__(256) k_pm_mul(const AffineDevT<typename E::T>* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n,
                                                uint32_t w, uint32_t from_mont, XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = live ? scalars[8 * (size_t)i + k] : 0u;
  if (from_mont) fr_from_montgomery<typename CheckConsts<E>::FR>(s);
  // bit length by leading-zero counts, then the maximum over the wave, made uniform
  uint32_t bits = 0;
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (s[k]) bits = 32u * k + 32u - (uint32_t)__clz((int)s[k]);
  if (!live) bits = 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)bits, off, 64);
    bits = o > bits ? o : bits;
  }
  const uint32_t top = pm_top_window((uint32_t)__builtin_amdgcn_readfirstlane((int)bits), w);
  if (!live) return;
  typename E::Md md;
  XyzzDevT<typename E::T> o;
  pm_windowed_mul<E>(o.p, table + i, n, s, w, top, md);
  out[i] = o;
}

// one lane per point, one scalar for all
template <class E>
__global__ void __launch_bounds__(256) k_pm_mul_uniform(const uint8_t* __restrict__ in, size_t stride, uint32_t n, const PmNaf naf,
                                                        XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  constexpr int W = E::WORDS;
  const uint8_t* p = in + (size_t)i * stride;
  uint32_t rec[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) rec[k] = reinterpret_cast<const uint32_t*>(p)[k];
  XyzzDevT<typename E::T> o;
  pm_mul_uniform<E>(o.p, rec, p[8 * W], naf, md);
  out[i] = o;
}
#endif

}  // namespace msm
