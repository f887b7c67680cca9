// sqrt.hpp -- square roots in Fp and Fp2 and arkworks' "larger of y and -y" rule, for both moduli.  All MSM_HD: the host build runs
// the same functions under the limb-bound checker (tests/test_point_codec_host.py).
//
//   BLS12-381  p = 3 (mod 4):  r = a^((p + 1)/4), then r^2 == a decides (ARK ff/src/fields/mod.rs:656-724, the `(p+1)/4` case).
//   BLS12-377  p = 1 (mod 4), p - 1 = 2^46 t:  Tonelli-Shanks.  One lane runs one point and a wave runs 64, so no trip count depends
//              on the data: the bit-by-bit form (RFC 9380 appendix I.4) -- w = a^((t-1)/2), z = a w, b = a w^2 = a^t, and for
//              i = 46 .. 2: square b a fixed i - 2 times, and where the result is not one multiply z by c = zeta^(2^(46-i)) under a
//              select -- 990 squarings + 3 products a round.  Again r^2 == a decides, so "no root" needs no Legendre symbol.
//   Fp2 = Fp[u]/(u^2 + NB): the complex method (ARK ff/src/fields/models/quadratic_extension.rs:370-428): with N = a0^2 + NB a1^2
//              and alpha = sqrt N (none: no root), delta = (a0 + alpha)/2, or (a0 - alpha)/2 when that one is no square;
//              c0 = sqrt delta, c1 = a1 / (2 c0).  a1 == 0: (sqrt a0, 0), or (0, sqrt(a0 / u^2)) when a0 is no square (u^2 is none
//              either, so the quotient is one).  The three Fp roots run through ONE call site in a rolled loop of three trips.
//
// Which of the two roots comes out is the algorithm's business; the point codec picks by lex_largest, so its output is
// bit-exact whatever root is found here.
//
// Constant exponents run through a rolled square-and-multiply with 2-bit digits (fe_pow_const): the digits are the same for
// every lane, so the test and the operand select are wave-uniform -- the manner of check_mul_affine.  Nothing is unrolled into the
// 64-KB instruction cache: a square root is about ten inlined field products of code.
//
// Limb bounds.  Every value that enters a product below is class M (strictly normalized limbs, value < 1.5p: the output of a product)
// unless the line says otherwise; a product of two class-M values is within fe_mul's contract with a factor 2^8 to spare, and its
// output is class M again, so a chain of squarings of any length keeps the invariant by the argument of the doubling chain of
// check_points.hpp.  The host build confirms it on every product (MSM_CHECK).
#pragma once
#include "check_points.hpp"

namespace msm {

#include "sqrt_consts.inc"

template <class F>
struct SqrtConsts;
template <>
struct SqrtConsts<Bls12_377_Fq> : Bls12_377_Sqrt {};
template <>
struct SqrtConsts<Bls12_381_Fq> : Bls12_381_Sqrt {};

// a == 1 (mod p) for a class-M value: strictly normalized limbs make the representation of a value unique, and the value is
// R mod p or R mod p + p (both below 1.5p for either modulus)
template <class F>
MSM_HD bool fe_is_one_M(const Fe& a) {
  uint32_t d0 = 0, d1 = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    d0 |= a.v[i] ^ F::ONE[i];
    d1 |= a.v[i] ^ SqrtConsts<F>::ONE_P[i];
  }
  return d0 == 0 || d1 == 0;
}

// r = a^e for the constant e = sum w[i] 2^(32 i) of `bits` bits (bits >= 3), 2-bit digits from the top.  a, r: class M.
template <class F, int NW>
MSM_HD void fe_pow_const(Fe& r, const Fe& a, const uint32_t (&w)[NW], int bits, const Modulus<F>& md) {
  Fe a2, a3, acc;
  fe_sqr<F>(a2, a, md);
  fe_mul<F>(a3, a2, a, md);
  const int top = (bits - 1) >> 1;   // index of the top digit, which holds the top set bit
  {
    const uint32_t d = (check_scalar_word<NW>(w, top >> 4) >> ((top & 15) * 2)) & 3;
    acc = d == 1 ? a : (d == 2 ? a2 : a3);
  }
#pragma unroll 1
  for (int i = top - 1; i >= 0; i--) {
    fe_sqr<F>(acc, acc, md);
    fe_sqr<F>(acc, acc, md);
    const uint32_t d = (check_scalar_word<NW>(w, i >> 4) >> ((i & 15) * 2)) & 3;
    if (d) {   // wave-uniform
      const Fe m = d == 1 ? a : (d == 2 ? a2 : a3);
      fe_mul<F>(acc, acc, m, md);
    }
  }
  r = acc;
}

// r^2 == a (mod p)?  Both class M.
template <class F>
MSM_HD bool fe_is_root(const Fe& r, const Fe& a, const Modulus<F>& md) {
  Fe s, d;
  fe_sqr<F>(s, r, md);
  fe_sub(d, s, a, F::BIAS2_28);   // (0.5p, 3.5p), limbs < 2^28 + 2^29
  return fe_is_zero_slow<F>(d);
}

// r = a square root of a, class M in and out; false (r then holds no root) when a has none.  a == 0 gives 0 and true.
template <class F>
MSM_HD bool fe_sqrt(Fe& r, const Fe& a, const Modulus<F>& md) {
  using K = SqrtConsts<F>;
  if constexpr (K::TWO_ADICITY == 1) {
    fe_pow_const<F, 12>(r, a, K::EXP, K::EXP_BITS, md);
  } else {
    Fe w, z, t, b, c;
    fe_pow_const<F, 12>(w, a, K::EXP, K::EXP_BITS, md);   // a^((t-1)/2)
    fe_mul<F>(z, w, a, md);                               // a^((t+1)/2): the root once its 2-power part is corrected
    fe_mul<F>(t, z, w, md);                               // a^t, of 2-power order
    b = t;
    fe_set(c, K::ZETA);
#pragma unroll 1
    for (int i = K::TWO_ADICITY; i >= 2; i--) {
#pragma unroll 1
      for (int j = 0; j < i - 2; j++) fe_sqr<F>(b, b, md);
      const LaneMask fix = lane_mask(!fe_is_one_M<F>(b));
      Fe zt, tt;
      fe_mul<F>(zt, z, c, md);
      fe_cmov(z, zt, fix);
      fe_sqr<F>(c, c, md);
      fe_mul<F>(tt, t, c, md);
      fe_cmov(t, tt, fix);
      b = t;
    }
    r = z;
  }
  return fe_is_root<F>(r, a, md);
}

// ---- the coordinate-field level, overloaded on the policy like el_inv ------------------------------------------------------------
template <class F>
MSM_HD bool el_sqrt(Fe& r, const Fe& a, const Modulus<F>& md, FpEl<F>*) {
  return fe_sqrt<F>(r, a, md);
}

// a: class M components.  r: class M components, except r.c1 of the general case, which is a product as well (class M).
template <class F, int NB>
MSM_HD bool el_sqrt(Fe2& r, const Fe2& a, const Modulus<F>& md, Fp2El<F, NB>*) {
  using K = SqrtConsts<F>;
  const bool real = fe_is_zero_M<F>(a.c1);   // a1 == 0: the branch the complex method cannot take (c0 might be 0)
  Fe half, x, alpha, c0, c1;
  fe_set(half, K::HALF);
  fe_zero(c0);
  fe_zero(c1);
  fe_zero(alpha);
  {
    Fe n0, n1, n, one;
    fe_sqr<F>(n0, a.c0, md);
    fe_sqr<F>(n1, a.c1, md);
#pragma unroll
    for (int i = 0; i < NL; i++) n.v[i] = n0.v[i] + n1.v[i] * (uint32_t)NB;   // a0^2 + NB a1^2, < 9p, limbs < 6 * 2^28
    fe_carry(n);
    fe_set(one, F::ONE);
    fe_mul<F>(n, n, one, md);   // the same residue, class M
    x = n;
    fe_cmov(x, a.c0, real);
  }
  bool done = false, bad = false;
#pragma unroll 1
  for (int step = 0; step < 3; step++) {
    Fe s, nx;
    const bool ok = fe_sqrt<F>(s, x, md);
    if (step == 0) {
      // general: s = alpha, next (a0 + alpha)/2.  real: a root of a0 ends it, otherwise next a0 / u^2
      Fe t, k;
      fe_add(t, a.c0, s);   // < 3p, limbs < 2^29
      fe_set(k, K::BETA_INV);
      fe_cmov(t, a.c0, real);
      fe_cmov(k, half, !real);
      fe_mul<F>(nx, t, k, md);
      alpha = s;
      if (real && ok) {
        c0 = s;
        done = true;
      }
      if (!real && !ok) bad = true;
    } else if (step == 1) {
      // general: a root is c0, otherwise next (a0 - alpha)/2.  real: the root is c1
      Fe t;
      fe_sub(t, a.c0, alpha, F::BIAS2_28);   // (0.5p, 3.5p), limbs < 2^28 + 2^29
      fe_mul<F>(nx, t, half, md);
      if (!done && !bad) {
        if (ok) {
          if (real) c1 = s; else c0 = s;
          done = true;
        } else if (real) {
          bad = true;
        }
      }
    } else {
      nx = x;
      if (!done && !bad) {
        if (ok) {
          c0 = s;
          done = true;
        } else {
          bad = true;
        }
      }
    }
    x = nx;
  }
  {
    // c1 = a1 / (2 c0) where the complex method ran (c0 != 0 there: c0 = 0 needs alpha = -a0, i.e. a1 = 0)
    Fe inv, t, q;
    fe_inv<F>(inv, c0, md);
    fe_mul<F>(t, a.c1, inv, md);
    fe_mul<F>(q, t, half, md);
    fe_cmov(c1, q, !real);
  }
  r.c0 = c0;
  r.c1 = c1;
  return done && !bad;
}

// 12 plain little-endian words (a canonical integer below p) > (p - 1)/2 ?
template <class F>
MSM_HD bool words_above_half(const uint32_t* w) {
  bool gt = false;   // equal so far => not above
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint32_t h = SqrtConsts<F>::PM1_HALF[i];
    if (w[i] != h) gt = w[i] > h;
  }
  return gt;
}

// arkworks' order on the canonical plain words of a coordinate: y > -y.  Fp: the integer exceeds (p - 1)/2
// (ARK ff/src/fields/models/fp/mod.rs:370-374).  Fp2: c1 decides unless it is zero, then c0 (quadratic_extension.rs:441-447).
template <class F>
MSM_HD bool lex_largest_words(const uint32_t* w, FpEl<F>*) {
  return words_above_half<F>(w);
}
template <class F, int NB>
MSM_HD bool lex_largest_words(const uint32_t* w, Fp2El<F, NB>*) {
  uint32_t nz = 0;
#pragma unroll
  for (int i = 12; i < 24; i++) nz |= w[i];
  return nz ? words_above_half<F>(w + 12) : words_above_half<F>(w);
}

// The same from an internal value (any input of E::to_plain: limbs < 2^30, value < 32p): it needs the canonical representative,
// as check_is_zero does.
template <class E>
MSM_HD bool el_lex_largest(const typename E::T& y, const typename E::Md& md) {
  uint32_t w[E::WORDS];
  E::to_plain(w, y, md);
  return lex_largest_words(w, (E*)nullptr);
}

}  // namespace msm
