// fixed_base.hpp -- batch fixed-base scalar multiplication: out[i] = s_i * g for ONE base g and many scalars.
//
// What it replaces: ARK ec/src/msm/fixed_base.rs:8-97 (FixedBase::get_mul_window_size, get_window_table, windowed_mul, msm) -- the
// call a KZG / Groth16 setup makes for [tau^i] G -- followed by batch_normalization_into_affine of its result.  Only the names and the
// contract are arkworks'; the algorithm is the device's:
//
//   table    level j, entry d: d * 2^(w j) * g as a normalised AffineDevT record, j < ceil(256 / w), d < 2^w (unsigned digits; entry 0
//            and every entry a small-order g sends to infinity are all-zero records -- (0, 0) is on no curve with b != 0, so the record
//            itself says "infinity" and the hot loop needs no second gather for a flag byte; the flag array k_pre_normalize writes
//            exists next to the table all the same).  Built in parallel over entries: the level bases 2^(w j) g by one lane (256
//            doublings), then one lane per run of FB_TABLE_RUN consecutive digits (double-and-add to the first, xyzz_madd of the level
//            base for the rest), then Launch<E>::pre_normalize as it stands.
//   mul      one lane per scalar: sum_j table[j][digit_j(s)], the general xyzz_madd, loop over the levels ROLLED.  All 256 bits of
//            the scalar count (an integer multiple: g need not have order r); with `from_mont` the 32 bytes are an arkworks Fr image
//            and pass through fr_from_montgomery first (FixedBase::msm takes &[ScalarField] and calls into_bigint, fixed_base.rs:66-67).
//   output   Montgomery's trick over FB_NORM_RUN consecutive results per lane, written as arkworks Affine images (x, y canonical,
//            flag byte, pad bytes zero; infinity = zeros with flag 1) or normalised Projective images ((x, y, 1) / (1, 1, 0)).
//
// Every per-element step is an MSM_HD function, so the host build (host_test_api.cpp, ht_fb_*) runs the same code under MSM_CHECK.
// Limb bounds: xyzz_dbl / xyzz_madd re-establish the stored-point invariants of curve.hpp from those invariants alone, table records
// are canonical (class M), so chains of any length hold them.
#pragma once
#include "check_points.hpp"   // check_scalar_word, CheckConsts (the scalar field of a coordinate-field policy)
#include "digits.hpp"
#include "msm_types.hpp"

namespace msm {

constexpr uint32_t FB_TABLE_RUN = 16;   // consecutive digits of one level per lane of the table build
constexpr uint32_t FB_NORM_RUN = 64;    // results per inversion of the output normalisation (k_pre_normalize's J in the engine)
constexpr uint32_t FB_MAX_WINDOW = 20;

MSM_HD uint32_t fb_levels(uint32_t w) { return (256 + w - 1) / w; }

// digit j of the 256-bit scalar s for window size w <= 20: bits [w j, w j + w).  j is wave-uniform, so the two words come out of
// the register array by uniform selects (check_scalar_word), never through memory.
MSM_HD uint32_t fb_digit(const uint32_t (&s)[8], uint32_t j, uint32_t w) {
  const uint32_t bit = j * w, wi = bit >> 5, sh = bit & 31;
  const uint32_t lo = check_scalar_word<8>(s, (int)wi), hi = check_scalar_word<8>(s, (int)wi + 1);   // word 8 does not exist: 0
  const uint64_t v = (((uint64_t)hi << 32) | lo) >> sh;
  return (uint32_t)v & ((1u << w) - 1);
}

// a table record that stands for the point at infinity: both coordinates all-zero (records are canonical)
MSM_HD bool fb_coord_zero(const Fe& a) {
  uint32_t z = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) z |= a.v[i];
  return z == 0;
}
MSM_HD bool fb_coord_zero(const Fe2& a) { return fb_coord_zero(a.c0) && fb_coord_zero(a.c1); }
template <class T>
MSM_HD bool fb_record_is_inf(const AffineT<T>& p) {
  return fb_coord_zero(p.x) && fb_coord_zero(p.y);
}

// ---- table build -----------------------------------------------------------------------------------------------------------
// The base as the caller holds it (arkworks Affine image; the flag byte is authoritative) -> the level bases 2^(w j) g, XYZZ.
template <class E>
MSM_HD void fb_level_bases(XyzzT<typename E::T>* out, const uint32_t* img, uint8_t flag, uint32_t w, uint32_t levels, const typename E::Md& md) {
  XyzzT<typename E::T> acc;
  if (flag) {
    xyzz_set_inf<E>(acc);
  } else {
    AffineT<typename E::T> g;
    E::from_abi(g.x, img, md);
    E::from_abi(g.y, img + E::WORDS, md);
    xyzz_from_affine<E>(acc, g, false);
  }
  for (uint32_t j = 0; j < levels; j++) {
    out[j] = acc;
    if (j + 1 < levels) {
#pragma unroll 1
      for (uint32_t k = 0; k < w; k++) xyzz_dbl<E>(acc, md);   // (infinity stays infinity: ZZ = 0 is absorbing)
    }
  }
}

// Entries [d0, d0 + count) of one level from its base B (normalised; `b_inf`: the level base is the point at infinity):
// d0 * B by double-and-add, then + B per entry.  Passes through infinity and through acc == +-B for a base of small order.
template <class E>
MSM_HD void fb_table_run(XyzzT<typename E::T>* out, const AffineT<typename E::T>& B, bool b_inf, uint32_t d0, uint32_t count, const typename E::Md& md) {
  XyzzT<typename E::T> acc;
  xyzz_set_inf<E>(acc);
  if (!b_inf) {
#pragma unroll 1
    for (int bit = (int)FB_MAX_WINDOW - 1; bit >= 0; bit--) {
      if (!xyzz_is_inf<E>(acc)) xyzz_dbl<E>(acc, md);
      if ((d0 >> bit) & 1) xyzz_madd<E>(acc, B, false, false, md);
    }
  }
#pragma unroll 1
  for (uint32_t k = 0; k < count; k++) {
    out[k] = acc;
    if (!b_inf) xyzz_madd<E>(acc, B, false, false, md);
  }
}

// ---- the hot path --------------------------------------------------------------------------------------------------------------
// acc = sum_j table[j][digit_j(s)].  `table`: levels << w records.  The record of level j + 1 is fetched while the addition of
// level j runs where the register file has room for it (E::PREFETCH_BASE: Fp yes, Fp2 no -- an Fp2 record is 56 VGPRs).
template <class E>
MSM_HD void fb_windowed_mul(XyzzT<typename E::T>& acc, const AffineDevT<typename E::T>* __restrict__ table, uint32_t (&s)[8], bool from_mont, uint32_t w,
                            uint32_t levels, const typename E::Md& md) {
  using El = typename E::T;
  if (from_mont) fr_from_montgomery<typename CheckConsts<E>::FR>(s);
  xyzz_set_inf<E>(acc);
  if constexpr (E::PREFETCH_BASE) {
    AffineT<El> cur = table[fb_digit(s, 0, w)].p;
#pragma unroll 1
    for (uint32_t j = 0; j < levels; j++) {
      // (the last turn re-reads a record of the last level: an address inside the table, a value nobody uses)
      const uint32_t jn = j + 1 < levels ? j + 1 : j;
      const AffineT<El> nxt = table[((size_t)jn << w) + fb_digit(s, jn, w)].p;
      if (!fb_record_is_inf(cur)) xyzz_madd<E>(acc, cur, false, false, md);
      cur = nxt;
    }
  } else {
#pragma unroll 1
    for (uint32_t j = 0; j < levels; j++) {
      const uint32_t d = fb_digit(s, j, w);
      if (d == 0) continue;
      const AffineT<El> a = table[((size_t)j << w) + d].p;
      if (!fb_record_is_inf(a)) xyzz_madd<E>(acc, a, false, false, md);
    }
  }
}

// ---- output ----------------------------------------------------------------------------------------------------------------
// bytes of one output image
template <class E, bool PROJECTIVE>
constexpr uint32_t fb_image_bytes() { return PROJECTIVE ? 12 * E::WORDS : 8 * E::WORDS + 8; }

// Results [lo, hi) -> images `out_stride` bytes apart (a multiple of 4), one inversion for the run.  prefix: one element per result.
template <class E, bool PROJECTIVE>
MSM_HD void fb_normalize_run(const XyzzDevT<typename E::T>* __restrict__ in, uint64_t lo, uint64_t hi, typename E::T* __restrict__ prefix,
                             uint8_t* __restrict__ out, size_t out_stride, const typename E::Md& md) {
  using El = typename E::T;
  constexpr int W = E::WORDS;
  El run;
  E::set_one(run);
  for (uint64_t j = lo; j < hi; j++) {
    const XyzzT<El> v = in[j].p;
    prefix[j] = run;
    if (!xyzz_is_inf<E>(v)) {
      El z;
      E::mul(z, v.zz, v.zzz, md);
      E::mul(run, run, z, md);
    }
  }
  El inv, one;
  el_inv(inv, run, md, (E*)nullptr);
  E::set_one(one);
  for (uint64_t j = hi; j-- > lo;) {
    const XyzzT<El> v = in[j].p;
    uint32_t* o = reinterpret_cast<uint32_t*>(out + j * out_stride);
    if (xyzz_is_inf<E>(v)) {
      if (PROJECTIVE) {
        uint32_t w1[W];
        E::to_abi(w1, one, md);
#pragma unroll
        for (int k = 0; k < W; k++) {
          o[k] = w1[k];
          o[W + k] = w1[k];
          o[2 * W + k] = 0;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 2 * W; k++) o[k] = 0;
        o[2 * W] = 1;       // flag byte 1, the three bytes behind it 0
        o[2 * W + 1] = 0;
      }
      continue;
    }
    El z, ti, zzi, zzzi, x, y;
    const El pre = prefix[j];
    E::mul(ti, inv, pre, md);          // (zz_j zzz_j)^-1
    E::mul(z, v.zz, v.zzz, md);
    E::mul(inv, inv, z, md);
    E::mul(zzi, ti, v.zzz, md);
    E::mul(zzzi, ti, v.zz, md);
    E::mul(x, v.x, zzi, md);
    E::mul(y, v.y, zzzi, md);
    uint32_t wx[W], wy[W];
    E::to_abi(wx, x, md);
    E::to_abi(wy, y, md);
#pragma unroll
    for (int k = 0; k < W; k++) {
      o[k] = wx[k];
      o[W + k] = wy[k];
    }
    if (PROJECTIVE) {
      uint32_t w1[W];
      E::to_abi(w1, one, md);
#pragma unroll
      for (int k = 0; k < W; k++) o[2 * W + k] = w1[k];
    } else {
      o[2 * W] = 0;
      o[2 * W + 1] = 0;
    }
  }
}

#if defined(__HIPCC__)
// one lane in all: the level bases of the table
template <class E>
__global__ void __launch_bounds__(64) k_fb_level_bases(const uint8_t* __restrict__ img, uint32_t w, uint32_t levels, XyzzDevT<typename E::T>* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  typename E::Md md;
  constexpr int W = E::WORDS;
  uint32_t rec[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) rec[k] = reinterpret_cast<const uint32_t*>(img)[k];
  fb_level_bases<E>(reinterpret_cast<XyzzT<typename E::T>*>(out), rec, img[8 * W], w, levels, md);
}

// one lane per run of FB_TABLE_RUN digits of a level; runs_per_level = ceil(2^w / FB_TABLE_RUN)
template <class E>
__global__ void __launch_bounds__(256) k_fb_table(const AffineDevT<typename E::T>* __restrict__ lbase, const uint8_t* __restrict__ lbase_inf, uint32_t w,
                                                  uint32_t levels, uint32_t runs_per_level, XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= levels * runs_per_level) return;
  const uint32_t j = t / runs_per_level, d0 = (t % runs_per_level) * FB_TABLE_RUN;
  const uint32_t per = 1u << w, count = d0 + FB_TABLE_RUN <= per ? FB_TABLE_RUN : per - d0;
  typename E::Md md;
  const AffineDevT<typename E::T> B = lbase[j];
  fb_table_run<E>(reinterpret_cast<XyzzT<typename E::T>*>(out + ((size_t)j << w) + d0), B.p, lbase_inf[j] != 0, d0, count, md);
}

// one lane per scalar
template <class E>
__global__ void __launch_bounds__(256) k_fb_mul(const AffineDevT<typename E::T>* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n,
                                                uint32_t w, uint32_t levels, uint32_t from_mont, XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  uint32_t s[8];
#pragma unroll
  for (int k = 0; k < 8; k++) s[k] = scalars[8 * (size_t)i + k];
  XyzzDevT<typename E::T> o;
  fb_windowed_mul<E>(o.p, table, s, from_mont != 0, w, levels, md);
  out[i] = o;
}

// one lane per FB_NORM_RUN results
template <class E, bool PROJECTIVE>
__global__ void __launch_bounds__(256) k_fb_normalize(const XyzzDevT<typename E::T>* __restrict__ in, uint32_t n, typename E::T* __restrict__ prefix,
                                                      uint8_t* __restrict__ out, size_t out_stride) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  const uint64_t lo = (uint64_t)t * FB_NORM_RUN;
  if (lo >= n) return;
  const uint64_t hi = (lo + FB_NORM_RUN < n) ? lo + FB_NORM_RUN : n;
  typename E::Md md;
  fb_normalize_run<E, PROJECTIVE>(in, lo, hi, prefix, out, out_stride, md);
}
#endif

}  // namespace msm
