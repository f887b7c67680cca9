// check_points.hpp -- is a base a legal input?  One status byte per point:
//
//   0  valid: flagged infinity, or on the curve and in the order-r subgroup
//   1  a coordinate is not below p (in-memory image: the Montgomery limbs; serialized record: the integer after the two flag
//      bits are masked)
//   2  canonical, but y^2 != x^3 + b
//   3  on the curve, outside the order-r subgroup
//
// The infinity flag is authoritative, as everywhere in this ABI: a flagged record is valid whatever its coordinates hold, and
// (0, 0) without the flag is off the curve.  Of a serialized record's two flag bits only bit 6 (infinity) is read; bit 7 (the sign of
// y in a compressed record) is masked and ignored, so a record with BOTH bits set -- an encoding arkworks' SWFlags::from_u8 refuses --
// counts as a flagged infinity here: the one place where the check is more lenient than `deserialize_uncompressed`.
// The lowest applicable status wins.  Both input forms of k_convert_bases are read:
// arkworks in-memory Affine images and uncompressed CanonicalSerialize records.  This is the check arkworks' checked reader
// applies (`deserialize_uncompressed`, ARK ec/src/models/short_weierstrass.rs:1204-1224) and the unchecked one skips.
//
// Two methods decide status 3, with identical verdicts:
//
//   CHECK_EXACT  [r]P == O by double-and-add over the bits of r (R_BITS - 1 = 252 / 254 doublings, 87 / 133 additions for
//                BLS12-377 / BLS12-381): the definition (ARK ec/src/models/short_weierstrass.rs:67-77,
//                which is what BLS12-377 uses there) and the yardstick for the other method.
//   CHECK_ENDO   G1: phi(P) = (beta x, y);  accept iff  phi(P) == -[u^2]P, computed as [u]([u]P)
//                    (ARKC bls12_381/src/curves/g1.rs:47-85, eprint 2021/1130 section 6)
//                G2: psi(P) = (conj(x) PSI_X, conj(y) PSI_Y);  accept iff  psi(P) == [u]P
//                    (ARKC bls12_381/src/curves/g2.rs:58-71, 93-137, eprint 2021/1130 section 4)
//                u = 0x8508c00000000001 (BLS12-377), -0xd201000000010000 (BLS12-381): 63 doublings and 6 / 5 additions per [u].
//
// Why the endomorphism tests are sound AND complete, for both curve families (the reference has them for BLS12-381 only;
// tests/test_check_points_consts.py re-checks every identity with Python integers):
//   G1.  r == u^4 - u^2 + 1.  In End(E), phi^2 + phi + 1 = 0, so deg(phi + [u^2]) = u^4 - u^2 + 1 = r: the kernel of
//        phi + [u^2] has exactly r points.  It contains the generator (that is how tools/subgroup_consts.py picks beta among the
//        two primitive cube roots of unity), hence all of G1, hence it IS G1.
//   G2.  #E(Fp) = p + 1 - t = p - u = h1 r with h1 = (u - 1)^2 / 3, and deg(psi - [u]) = u^2 - t u + p = p - u = h1 r.
//        #E'(Fp2) = h2 r with h2 = (u^8 - 4u^7 + 5u^6 - 4u^4 + 6u^3 - 4u^2 - 4u + 13) / 9, gcd(h1, h2) = gcd(h2, r) = 1.
//        A point of E'(Fp2) in the kernel of psi - [u] has an order that divides both h1 r and h2 r, i.e. r, and the r-torsion
//        of E'(Fp2) is G2.  The kernel contains the G2 generator (how PSI_X, PSI_Y are picked), hence all of G2.
// All identities hold for BLS12-377 and BLS12-381, so both methods exist for all four curves.
//
// The scalar (r or u) is the same for every point, so the bit test of the double-and-add loop is uniform across a wave; the loop
// stays ROLLED (one doubling is thousands of instructions, the instruction cache holds 64 KB).  The accumulator passes through
// infinity and through acc == +-P for points of small order -- (p - 1, 0) of BLS12-377 G1 has order 2 -- so the additions are
// the general xyzz_madd / xyzz_add, and a doubling of infinity stays infinity (ZZ = 0 is absorbing in dbl-2008-s-1).
// Limb bounds: every doubling and addition re-establishes the stored-point invariants of curve.hpp from those invariants
// alone, so a chain of any length holds them; the host build runs the whole chain under MSM_CHECK (tests/test_check_points_host.py).
#pragma once
#include "curve.hpp"

namespace msm {

enum CheckStatus : uint8_t { CHECK_VALID = 0, CHECK_NOT_CANONICAL = 1, CHECK_OFF_CURVE = 2, CHECK_OFF_SUBGROUP = 3 };
enum CheckMethod : int { CHECK_EXACT = 0, CHECK_ENDO = 1 };

// per coordinate-field policy: the curve coefficient, the scalar field, the family's subgroup constants
template <class E>
struct CheckConsts;
template <>
struct CheckConsts<FpEl<Bls12_377_Fq>> {
  using Sub = Bls12_377_Sub;
  using FR = Bls12_377_Fr;
  static constexpr int R_BITS = 253;
};
template <>
struct CheckConsts<FpEl<Bls12_381_Fq>> {
  using Sub = Bls12_381_Sub;
  using FR = Bls12_381_Fr;
  static constexpr int R_BITS = 255;
};
template <>
struct CheckConsts<Fp2El<Bls12_377_Fq, 5>> : CheckConsts<FpEl<Bls12_377_Fq>> {};
template <>
struct CheckConsts<Fp2El<Bls12_381_Fq, 1>> : CheckConsts<FpEl<Bls12_381_Fq>> {};

template <class Sub>
MSM_HD void check_load_b(Fe& b) { fe_set(b, Sub::B1); }
template <class Sub>
MSM_HD void check_load_b(Fe2& b) {
  fe_set(b.c0, Sub::B2_0);
  fe_set(b.c1, Sub::B2_1);
}

// word `wi` of a constant scalar, by selects: `wi` is wave-uniform but not a compile-time constant inside the rolled loop, and a
// table lookup would put the words in memory
template <int NW>
MSM_HD uint32_t check_scalar_word(const uint32_t (&w)[NW], int wi) {
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < NW; k++) r = (wi == k) ? w[k] : r;
  return r;
}

// 12 little-endian words < p ?
template <class F>
MSM_HD bool check_words_below_p(const uint32_t* w) {
  bool lt = false;   // equal so far => not below
#pragma unroll
  for (int i = 0; i < 12; i++) {
    const uint32_t pi = (uint32_t)(F::P64[i >> 1] >> (32 * (i & 1)));
    if (w[i] != pi) lt = w[i] < pi;
  }
  return lt;
}

// canonical representative == 0 ?   Input: any bounded lazy value (limbs < 2^31, value < 64p per component)
template <class F>
MSM_HD bool check_is_zero(const Fe& a, FpEl<F>*) { return fe_is_zero_slow<F>(a); }
template <class F, int NB>
MSM_HD bool check_is_zero(const Fe2& a, Fp2El<F, NB>*) { return fe_is_zero_slow<F>(a.c0) && fe_is_zero_slow<F>(a.c1); }

// a == b (mod p);  a: stored coordinate or class M (limbs < 2^28 + 16, value < 16p), b: class M
template <class E>
MSM_HD bool check_equal(const typename E::T& a, const typename E::T& b) {
  typename E::T d;
  E::sub(d, a, b, E::Fld::BIAS2_28);   // < 18p, limbs < 2^30
  return check_is_zero(d, (E*)nullptr);
}
// a == -b (mod p), same operand classes
template <class E>
MSM_HD bool check_equal_neg(const typename E::T& a, const typename E::T& b) {
  typename E::T d;
  E::add(d, a, b);                     // < 18p, limbs < 2^29 + 16
  return check_is_zero(d, (E*)nullptr);
}

// acc = [k]P for the constant k = sum w[i] 2^(32 i) whose top set bit is bit TOP.  P affine, not infinity.
template <class E, int NW>
MSM_HD void check_mul_affine(XyzzT<typename E::T>& acc, const AffineT<typename E::T>& P, const uint32_t (&w)[NW], int top, const typename E::Md& md) {
  xyzz_from_affine<E>(acc, P, false);
#pragma unroll 1
  for (int bit = top - 1; bit >= 0; bit--) {
    xyzz_dbl<E>(acc, md);
    if ((check_scalar_word<NW>(w, bit >> 5) >> (bit & 31)) & 1) xyzz_madd<E>(acc, P, false, false, md);
  }
}
// the same from an XYZZ point (the second [u] of the G1 test)
template <class E, int NW>
MSM_HD void check_mul_xyzz(XyzzT<typename E::T>& acc, const XyzzT<typename E::T>& Q, const uint32_t (&w)[NW], int top, const typename E::Md& md) {
  acc = Q;
#pragma unroll 1
  for (int bit = top - 1; bit >= 0; bit--) {
    xyzz_dbl<E>(acc, md);
    if ((check_scalar_word<NW>(w, bit >> 5) >> (bit & 31)) & 1) xyzz_add<E>(acc, Q, md);
  }
}

// psi(P) over Fp2; never instantiated for G1 coordinates
template <class E>
MSM_HD void check_psi(AffineT<Fe2>& r, const AffineT<Fe2>& P, const typename E::Md& md) {
  using Sub = typename CheckConsts<E>::Sub;
  using F = typename E::Fld;
  Fe2 cx = P.x, cy = P.y, kx, ky;
  fe_neg(cx.c1, P.x.c1, F::BIAS2_28);   // conj: (0, 2p], limbs < 2^29
  fe_neg(cy.c1, P.y.c1, F::BIAS2_28);
  fe_set(kx.c0, Sub::PSI_X0);
  fe_set(kx.c1, Sub::PSI_X1);
  fe_set(ky.c0, Sub::PSI_Y0);
  fe_set(ky.c1, Sub::PSI_Y1);
  E::mul(r.x, cx, kx, md);
  E::mul(r.y, cy, ky, md);
}

// P (class M coordinates, on the curve, not infinity) in the order-r subgroup?
template <class E, int METHOD>
MSM_HD bool check_in_subgroup(const AffineT<typename E::T>& P, const typename E::Md& md) {
  using CC = CheckConsts<E>;
  using T = typename E::T;
  XyzzT<T> acc;
  if constexpr (METHOD == CHECK_EXACT) {
    check_mul_affine<E, 8>(acc, P, CC::FR::R, CC::R_BITS - 1, md);
    return xyzz_is_inf<E>(acc);
  } else if constexpr (E::WORDS == 12) {
    // G1: [u^2]P == -phi(P) = (beta x, -y)
    XyzzT<T> q1;
    check_mul_affine<E, 2>(q1, P, CC::Sub::U, 63, md);
    check_mul_xyzz<E, 2>(acc, q1, CC::Sub::U, 63, md);
    if (xyzz_is_inf<E>(acc)) return false;
    T beta, bx, ex, ey;
    fe_set(beta, CC::Sub::BETA);
    E::mul(bx, beta, P.x, md);
    E::mul(ex, bx, acc.zz, md);
    E::mul(ey, P.y, acc.zzz, md);
    return check_equal<E>(acc.x, ex) && check_equal_neg<E>(acc.y, ey);
  } else {
    // G2: [|u|]P == +-psi(P)
    check_mul_affine<E, 2>(acc, P, CC::Sub::U, 63, md);
    if (xyzz_is_inf<E>(acc)) return false;
    AffineT<T> s;
    check_psi<E>(s, P, md);
    T ex, ey;
    E::mul(ex, s.x, acc.zz, md);
    E::mul(ey, s.y, acc.zzz, md);
    if (!check_equal<E>(acc.x, ex)) return false;
    return CC::Sub::U_NEG ? check_equal_neg<E>(acc.y, ey) : check_equal<E>(acc.y, ey);
  }
}

// One record as the caller holds it -> status.  `rec`: 2 * E::WORDS u32 words of coordinates; `flag`: the infinity flag byte of an
// in-memory image (SERIALIZED = false; ignored otherwise -- a serialized record carries it in bit 6 of its last byte).
template <class E, bool SERIALIZED, int METHOD>
MSM_HD uint8_t check_point(const uint32_t* rec, uint8_t flag, const typename E::Md& md) {
  using F = typename E::Fld;
  using T = typename E::T;
  constexpr int W = E::WORDS;
  uint32_t w[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) w[k] = rec[k];
  if (SERIALIZED) {
    flag = (w[2 * W - 1] >> 30) & 1;
    w[2 * W - 1] &= 0x3fffffffu;
  }
  if (flag) return CHECK_VALID;
  bool canonical = true;
#pragma unroll
  for (int c = 0; c < 2 * W / 12; c++) canonical = canonical && check_words_below_p<F>(w + 12 * c);
  if (!canonical) return CHECK_NOT_CANONICAL;
  AffineT<T> P;
  if (SERIALIZED) {
    E::from_plain(P.x, w, md);
    E::from_plain(P.y, w + W, md);
  } else {
    E::from_abi(P.x, w, md);
    E::from_abi(P.y, w + W, md);
  }
  {
    T y2, x2, x3, b, rhs, d;
    E::sqr(y2, P.y, md);
    E::sqr(x2, P.x, md);
    E::mul(x3, x2, P.x, md);
    check_load_b<typename CheckConsts<E>::Sub>(b);
    E::add(rhs, x3, b);                // < 4p, limbs < 2^29
    E::sub(d, y2, rhs, F::BIAS4_29);   // (0, 6p), limbs < 2^30
    if (!check_is_zero(d, (E*)nullptr)) return CHECK_OFF_CURVE;
  }
  return check_in_subgroup<E, METHOD>(P, md) ? CHECK_VALID : CHECK_OFF_SUBGROUP;
}

#if defined(__HIPCC__)
// One lane per point: reads the caller's record (in-memory Affine image `stride` bytes apart, or an uncompressed CanonicalSerialize
// record of 2 coordinates), classifies it, writes one status byte with a plain store.  Lanes whose record fails the canonical or the curve test skip
// the scalar multiplication; they are rare, the divergence is harmless.
template <class E, bool SERIALIZED, int METHOD>
__global__ void __launch_bounds__(256) k_check_points(const uint8_t* __restrict__ in, size_t stride, uint32_t n, uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  constexpr int W = E::WORDS;
  const size_t rec = SERIALIZED ? (size_t)8 * W : stride;
  const uint8_t* p = in + (size_t)i * rec;
  const uint8_t flag = SERIALIZED ? (uint8_t)((p[8 * W - 1] >> 6) & 1) : p[8 * W];
  // bit 7 marks a record flagged infinity (the engine counts those and hands the caller bits 0-1)
  status[i] = (uint8_t)(check_point<E, SERIALIZED, METHOD>(reinterpret_cast<const uint32_t*>(p), flag, md) | (flag ? 0x80 : 0));
}
#endif

}  // namespace msm
