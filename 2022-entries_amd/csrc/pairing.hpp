// pairing.hpp -- batch pairings and pairing products on BLS12-377 / BLS12-381: arkworks' Bls12::pairing / product_of_pairings
// (curves/src/templates/bls12/bls12.rs of snarkVM) over Fp2El of curve.hpp.
//
// Scheme.  An Fp12 value is 168 limbs and an inlined Fp12 product some 20 000 multiply-adds of text, so nothing above Fp2 is ever code:
// the tower, the Miller loop and the final exponentiation are PROGRAMS -- lists of operations on Fp2 slots -- that the host writes once
// per handle (PrGen below: plain nested loops, one routine per tower operation) and one small interpreter (pr_exec) runs, one lane per
// pair or group.  The interpreter holds the ONLY Fp2 product of a kernel; its operands are in registers, every tower value lives in a
// lane-interleaved workspace in device memory (word k of a lane at ws[k * pitch + lane]: a wave reads consecutive words).  Global
// memory is enough: an Fp2 product is over 1100 multiply-adds against 84 words moved.  The program counter, the operation and the slot
// numbers are wave-uniform, so the operations are read through the scalar unit and no access is indexed by data.
//
// Fp12 is held FLAT: six Fp2 coefficients of 1, w, ..., w^5 with w^6 = xi (arkworks' c0 = (a0, a2, a4), c1 = (a1, a3, a5) with
// v = w^2), a product is the 6 x 6 convolution with the wrapped terms taken from xi * b (36 products, 21 for a square, 18 against a
// line), a square in the cyclotomic subgroup is Granger-Scott's (6 products).  The line of a doubling or addition step comes out of
// the homogeneous projective step itself, scaled by an element of Fp2 (and by w^3 for the M-type twist) that the final power kills:
//   D-type (BLS12-377, mul_by_034):  l = yP s Z  -  xP w Z * w  +  (w X - R) * w^3      (doubling;  w = 3 X^2, s = 2 Y Z, R = Y s)
//   M-type (BLS12-381, mul_by_014):  the same three values at w^3, w^2 and 1.
// The final exponentiation is bls12.rs' chain (eprint 2016/130 Table 1, exponent 3 (p^4 - p^2 + 1) / r after the easy part); the one
// inversion is conj(f) / N(f) with the norms taken down to Fp and a^(p - 2) there, all through the same product.
//
// Bound classes (fp28.hpp's terms).  Class W: strictly normalized limbs, value < 3p per component.  EVERY slot of the workspace holds a
// class-W value: a product stores class M (a subset), every other operation ends in fe_weak_reduce.  Inside an operation:
//   MUL / MAC   operands W (limbs < 2^28, value < 3p) -- well inside Fp2El::mul's limbs < 2^30, value <= 18p; result class M
//   accumulator up to 6 class-M products: value < 9p, limbs < 6 * 2^28 < 2^31 -- what fe_weak_reduce takes (value < 32p, limbs < 2^31)
//   ADD < 6p;  SUB, CONJ  a + 4p - b < 7p (BIAS4_29: b's limbs <= 2^29, value <= 4p);  MULXI  16p - 5 a1 in (p, 16p] carried, or a0 + 4p - a1
// The host build checks class W on every load and the columns of every product.
#pragma once
#include <utility>
#include <vector>

#include "curve.hpp"
#include "pairing_consts.inc"

namespace msm {

constexpr uint32_t PR_LANES = 64;        // lanes of a block
constexpr uint32_t PR_FE2_WORDS = 2 * NL;
constexpr uint32_t PR_GT_BYTES = 576;
constexpr uint32_t PR_SERIAL_GROUP = 8;  // groups up to here are walked by one lane; larger ones are split over lanes and multiplied as a tree
constexpr uint32_t PR_FAN_IN = 8;        // values one lane of a product level multiplies
constexpr uint32_t PR_MAX_ITEMS = 131072; // lanes in flight of one chunk -- two waves on each of the 1024 SIMDs: the workspace is sized by this, never by n

// ---- the slot map of a lane's workspace (Fp2 slots; an Fp12 region is six in a row) ----
enum : uint16_t {
  PR_F = 0,         // the Miller value of the pair at hand / the value a stage receives
  PR_G = 6,         // its other half (products ping-pong between F and G)
  PR_ACC = 12,      // the product over the lane's run of pairs
  PR_LINE = 18,     // the line: coefficients at w^0 .. w^5, three of them in use
  PR_XI = 24,       // xi * b_j of the product at hand
  PR_TMP = 30,      // 16 temporaries of the step formulas, the squares and the inverse
  PR_TX = 46, PR_TY = 47, PR_TZ = 48,   // T, homogeneous projective
  PR_QX = 49, PR_QY = 50,               // Q, affine
  PR_PX = 51, PR_PY = 52,               // P, affine, as elements of Fp2
  PR_MILLER_SLOTS = 53,
  PR_REGION0 = 53,  // the regions of the final exponentiation: 8 more Fp12 values
  PR_REGIONS = 8,
  PR_SLOTS = PR_REGION0 + 6 * PR_REGIONS,
};
constexpr uint16_t PR_CONST = 0x8000;   // operands from here on are entries of the constant table
enum : uint16_t { PR_C_ZERO = PR_CONST, PR_C_ONE = PR_CONST + 1, PR_C_FROB = PR_CONST + 2, PR_C_IN = PR_CONST + 17, PR_C_OUT = PR_CONST + 18, PR_CONSTS = 19 };

enum PrCode : uint16_t {
  PR_MUL = 0,   // d = a * b                      (class M)
  PR_MULR,      // the same with b a RAW image: normalized limbs of any value below 2^381 <= 19p (a is a constant of Fp: a.c1 = 0)
  PR_MAC,       // acc += a * b
  PR_FIN,       // d = acc, acc = 0
  PR_ADD,       // d = a + b
  PR_SUB,       // d = a - b
  PR_MULXI,     // d = xi * a
  PR_CONJ,      // d = conj(a)  (the Fp2 conjugate)
  PR_COPY,      // d = a
  PR_SELC,      // d = a where the lane's flag is set (a pair with an infinity): else d stays
};
struct PrOp {
  uint16_t op, d, a, b;
};

struct PrWs {
  uint32_t* base;   // the workspace (wave-uniform)
  uint32_t pitch;   // its lanes (at most PR_MAX_ITEMS)
  uint32_t lane;    // this lane's column: word k of a slot at slot_base[k * pitch + lane] -- a uniform address plus a 32-bit offset
};

// what a family adds to its Fp2El: the parameter x, the twist, xi
template <class E>
struct PrFamily;
template <>
struct PrFamily<Fp2El<Bls12_377_Fq, 5>> {
  using K = Bls12_377_Pairing;
  static constexpr uint64_t X = 0x8508c00000000001ull;
  static constexpr bool X_NEG = false, M_TWIST = false, XI_IS_U = true;   // xi = u, u^2 = -5
  static constexpr int NEG_BETA = 5;
};
template <>
struct PrFamily<Fp2El<Bls12_381_Fq, 1>> {
  using K = Bls12_381_Pairing;
  static constexpr uint64_t X = 0xd201000000010000ull;
  static constexpr bool X_NEG = true, M_TWIST = true, XI_IS_U = false;    // xi = 1 + u, u^2 = -1
  static constexpr int NEG_BETA = 1;
};

MSM_HD void pr_check_w(const Fe& a, uint32_t p_top) {
#pragma unroll
  for (int i = 0; i < NL - 1; i++) MSM_CHECK(a.v[i] <= LMASK);
  MSM_CHECK(a.v[NL - 1] <= 3 * p_top + 2);
  (void)a;
  (void)p_top;
}

template <class F>
MSM_HD void pr_load(Fe2& r, const PrWs& ws, const Fe2* __restrict__ consts, uint16_t s, bool raw = false) {
  if (s >= PR_CONST) {
    r = consts[s - PR_CONST];
  } else {
    const uint32_t* at = ws.base + (uint64_t)s * PR_FE2_WORDS * ws.pitch;
#pragma unroll
    for (int i = 0; i < NL; i++) r.c0.v[i] = (at + (uint64_t)i * ws.pitch)[ws.lane];
#pragma unroll
    for (int i = 0; i < NL; i++) r.c1.v[i] = (at + (uint64_t)(NL + i) * ws.pitch)[ws.lane];
  }
  pr_check_w(r.c0, raw ? 43691u : F::P[NL - 1]);   // raw: below 2^381 (pr_miller_lane), top limb < 2^17 <= 3 * 43691 + 2
  pr_check_w(r.c1, raw ? 43691u : F::P[NL - 1]);
}

MSM_HD void pr_store(const PrWs& ws, uint16_t s, const Fe2& r) {
  uint32_t* at = ws.base + (uint64_t)s * PR_FE2_WORDS * ws.pitch;
#pragma unroll
  for (int i = 0; i < NL; i++) (at + (uint64_t)i * ws.pitch)[ws.lane] = r.c0.v[i];
#pragma unroll
  for (int i = 0; i < NL; i++) (at + (uint64_t)(NL + i) * ws.pitch)[ws.lane] = r.c1.v[i];
}

// one component of a slot (h = 0: c0, 1: c1)
MSM_HD void pr_load_fe(Fe& r, const PrWs& ws, uint32_t s, uint32_t h) {
  const uint32_t* at = ws.base + ((uint64_t)s * PR_FE2_WORDS + (uint64_t)h * NL) * ws.pitch;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = (at + (uint64_t)i * ws.pitch)[ws.lane];
}
MSM_HD void pr_store_fe(const PrWs& ws, uint32_t s, uint32_t h, const Fe& r) {
  uint32_t* at = ws.base + ((uint64_t)s * PR_FE2_WORDS + (uint64_t)h * NL) * ws.pitch;
#pragma unroll
  for (int i = 0; i < NL; i++) (at + (uint64_t)i * ws.pitch)[ws.lane] = r.v[i];
}

// r = xi * a for a class-W a: lazy, value <= 16p, limbs < 2^30
template <class E>
MSM_HD void pr_mulxi(Fe2& r, const Fe2& a) {
  using F = typename E::Fld;
  if constexpr (PrFamily<E>::XI_IS_U) {   // (a0 + a1 u) u = beta a1 + a0 u
    Fe s;
#pragma unroll
    for (int i = 0; i < NL; i++) s.v[i] = a.c1.v[i] * (uint32_t)PrFamily<E>::NEG_BETA;   // < 15p, limbs < 5 * 2^28
    fe_neg(r.c0, s, F::BIAS16_31);   // (p, 16p]
    fe_carry(r.c0);
    r.c1 = a.c0;
  } else {                                // (a0 + a1 u)(1 + u) = (a0 - a1) + (a0 + a1) u
    fe_sub(r.c0, a.c0, a.c1, F::BIAS4_29);
    fe_add(r.c1, a.c0, a.c1);
  }
}

// The interpreter.  `flag`: this lane's pair has an infinity (PR_SELC).  Every operation names two operands (the program writes the
// constant 0 where it has none, and d itself for PR_SELC), so the loop holds ONE load of each, one product, one reduction and one
// store.  Every operand number was checked against PR_SLOTS and PR_CONSTS when the program was written (PrGen::check).
template <class E>
MSM_HD void pr_exec(const PrWs& ws, const PrOp* __restrict__ prog, uint32_t len, const Fe2* __restrict__ consts, bool flag, const typename E::Md& md) {
  using F = typename E::Fld;
  Fe2 acc;
  E::zero(acc);
#pragma unroll 1
  for (uint32_t pc = 0; pc < len; pc++) {
    const PrOp o = prog[pc];
    Fe2 a, b, r;
    pr_load<F>(a, ws, consts, o.a);
    pr_load<F>(b, ws, consts, o.b, o.op == PR_MULR);
    if (o.op <= PR_MAC) {
      // operands of class W are carried and below 18p: the product that skips the carries.  a0 b0 + 5 a1 (32p - b1) <= 489 p^2; for
      // PR_MULR a1 = 0, b1 <= 19p <= 32p, and the products are a0 b0 and a0 b1 <= 19 p^2 -- class M either way
      E::template mul_c<true>(r, a, b, md);
      if (o.op == PR_MAC) {
        E::add(acc, acc, r);
        continue;
      }
    } else {
      switch (o.op) {
        case PR_FIN:
          r = acc;
          E::zero(acc);
          break;
        case PR_ADD: E::add(r, a, b); break;
        case PR_SUB: E::sub(r, a, b, F::BIAS4_29); break;
        case PR_MULXI: pr_mulxi<E>(r, a); break;
        case PR_CONJ:
          r.c0 = a.c0;
          fe_neg(r.c1, a.c1, F::BIAS4_29);
          break;
        case PR_SELC:
          r = b;
          E::cmov(r, a, flag);
          break;
        default: r = a; break;
      }
      fe_weak_reduce<F>(r.c0);
      fe_weak_reduce<F>(r.c1);
    }
    pr_store(ws, o.d, r);
  }
}

// ---- the programs (host) -----------------------------------------------------------------------------------------------------------
// One routine per tower operation; regions are slot numbers of six Fp2 in a row.  A product's result region differs from its operands.
template <class E>
struct PrGen {
  using Fam = PrFamily<E>;
  std::vector<PrOp> ops;
  uint64_t products = 0;   // Fp2 products

  void emit(uint16_t op, uint16_t d, uint16_t a, uint16_t b) { ops.push_back(PrOp{op, d, a, b}); }
  void mul(uint16_t d, uint16_t a, uint16_t b) { emit(PR_MUL, d, a, b); products++; }
  void mulr(uint16_t d, uint16_t a, uint16_t b) { emit(PR_MULR, d, a, b); products++; }
  void mac(uint16_t a, uint16_t b) { emit(PR_MAC, 0, a, b); products++; }
  void fin(uint16_t d) { emit(PR_FIN, d, PR_C_ZERO, PR_C_ZERO); }
  void add(uint16_t d, uint16_t a, uint16_t b) { emit(PR_ADD, d, a, b); }
  void sub(uint16_t d, uint16_t a, uint16_t b) { emit(PR_SUB, d, a, b); }
  void neg(uint16_t d, uint16_t a) { emit(PR_SUB, d, PR_C_ZERO, a); }
  void mulxi(uint16_t d, uint16_t a) { emit(PR_MULXI, d, a, PR_C_ZERO); }
  void conj(uint16_t d, uint16_t a) { emit(PR_CONJ, d, a, PR_C_ZERO); }
  void copy(uint16_t d, uint16_t a) { emit(PR_COPY, d, a, PR_C_ZERO); }
  void selc(uint16_t d, uint16_t a) { emit(PR_SELC, d, a, d); }

  bool check() const {
    for (const PrOp& o : ops) {
      if (o.op > PR_SELC) return false;
      for (uint16_t s : {o.d, o.a, o.b})
        if (s >= PR_CONST ? (uint32_t)(s - PR_CONST) >= PR_CONSTS : s >= PR_SLOTS) return false;
      if (o.d >= PR_CONST) return false;
    }
    return true;
  }

  // ---- Fp12, flat ----
  void f12_copy(uint16_t R, uint16_t A) { for (int k = 0; k < 6; k++) copy(R + k, A + k); }
  void f12_one(uint16_t R) { for (int k = 0; k < 6; k++) copy(R + k, k ? PR_C_ZERO : PR_C_ONE); }
  // R = A * B;  bmask: the coefficients of B that are not zero
  void f12_mul(uint16_t R, uint16_t A, uint16_t B, unsigned bmask = 0x3f) {
    for (int j = 1; j < 6; j++)
      if (bmask >> j & 1) mulxi(PR_XI + j, B + j);
    for (int k = 0; k < 6; k++) {
      for (int i = 0; i < 6; i++) {
        const int j = k - i, jj = j < 0 ? j + 6 : j;
        if (!(bmask >> jj & 1)) continue;
        mac(A + i, j < 0 ? PR_XI + jj : B + jj);
      }
      fin(R + k);
    }
  }
  // R = A^2: each cross product once, against the doubled coefficient (21 products)
  void f12_sqr(uint16_t R, uint16_t A) {
    const uint16_t D = PR_TMP, XD = PR_TMP + 6;   // 2 a_j and xi * 2 a_j
    for (int j = 1; j < 6; j++) {
      add(D + j, A + j, A + j);
      mulxi(XD + j, D + j);
      if (j >= 3) mulxi(PR_XI + j, A + j);
    }
    for (int k = 0; k < 6; k++) {
      for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) {
          if ((i + j) % 6 != k) continue;
          const bool wrap = i + j >= 6;
          if (i == j) mac(A + i, wrap ? PR_XI + j : A + j);
          else mac(A + i, wrap ? XD + j : D + j);
        }
      fin(R + k);
    }
  }
  // R = conj(A) = A^(p^6): w -> -w
  void f12_conj(uint16_t R, uint16_t A) {
    for (int k = 0; k < 6; k++) {
      if (k & 1) neg(R + k, A + k);
      else if (R != A) copy(R + k, A + k);
    }
  }
  // R = A^(p^j), j = 1, 2, 3 (R may be A)
  void f12_frobenius(uint16_t R, uint16_t A, int j) {
    for (int k = 0; k < 6; k++) {
      uint16_t src = A + k;
      if (j & 1) {
        conj(R + k, src);
        src = R + k;
      }
      if (k) mul(R + k, src, PR_C_FROB + 5 * (j - 1) + (k - 1));
      else if (src != R + k) copy(R + k, src);
    }
  }
  // Granger-Scott: R = A^2 for A in the cyclotomic subgroup (6 products).  With arkworks' names r0 = a0, r4 = a2, r3 = a4, r2 = a1,
  // r1 = a3, r5 = a5 and (t0, t1) = sq4(r0, r1), (t2, t3) = sq4(r2, r3), (t4, t5) = sq4(r4, r5) where sq4(a, b) = (a^2 + xi b^2, 2 a b):
  //   a0' = 3 t0 - 2 r0, a2' = 3 t2 - 2 r4, a4' = 3 t4 - 2 r3, a1' = 3 xi t5 + 2 r2, a3' = 3 t1 + 2 r1, a5' = 3 t3 + 2 r5
  void sq4(uint16_t t0, uint16_t t1, uint16_t a, uint16_t b) {
    const uint16_t ab = PR_TMP + 12, s1 = PR_TMP + 13, s2 = PR_TMP + 14;
    mul(ab, a, b);
    add(s1, a, b);
    mulxi(s2, b);
    add(s2, s2, a);
    mul(t0, s1, s2);          // (a + b)(a + xi b) = a^2 + xi b^2 + (1 + xi) a b
    sub(t0, t0, ab);
    mulxi(s1, ab);
    sub(t0, t0, s1);
    add(t1, ab, ab);
  }
  void f12_cyclotomic_sqr(uint16_t R, uint16_t A) {
    const uint16_t t = PR_TMP;   // t0 .. t5
    sq4(t + 0, t + 1, A + 0, A + 3);
    sq4(t + 2, t + 3, A + 1, A + 4);
    sq4(t + 4, t + 5, A + 2, A + 5);
    const uint16_t u = PR_TMP + 12, v = PR_TMP + 13;
    auto fin3 = [&](uint16_t d, uint16_t tt, uint16_t r, bool plus) {   // d = 3 tt +- 2 r
      add(u, tt, tt);
      add(u, u, tt);
      add(v, r, r);
      if (plus) add(d, u, v); else sub(d, u, v);
    };
    mulxi(PR_TMP + 14, t + 5);
    fin3(R + 0, t + 0, A + 0, false);
    fin3(R + 2, t + 2, A + 2, false);
    fin3(R + 4, t + 4, A + 4, false);
    fin3(R + 1, PR_TMP + 14, A + 1, true);
    fin3(R + 3, t + 1, A + 3, true);
    fin3(R + 5, t + 3, A + 5, true);
  }
  // R = A^|x| (conjugated when x is negative) for A in the cyclotomic subgroup; S: a spare region; R, S, A distinct
  void f12_cyclotomic_exp(uint16_t R, uint16_t S, uint16_t A) {
    // the squarings alternate between R and S; arrange for the last value to land in R
    int flips = 0;
    for (int b = 62; b >= 0; b--) flips += 1 + (int)(Fam::X >> b & 1);
    uint16_t cur = (flips & 1) ? S : R, oth = (flips & 1) ? R : S;
    f12_copy(cur, A);
    for (int b = 62; b >= 0; b--) {
      f12_cyclotomic_sqr(oth, cur);
      std::swap(cur, oth);
      if (Fam::X >> b & 1) {
        f12_mul(oth, cur, A);
        std::swap(cur, oth);
      }
    }
    if (Fam::X_NEG) f12_conj(cur, cur);
  }
  // the Fp2 inverse: D = A^-1 through the norm to Fp and n^(p - 2) there (t0, t1: temporaries)
  void f2_inv(uint16_t D, uint16_t A, uint16_t t0, uint16_t t1) {
    using F = typename E::Fld;
    conj(t0, A);
    mul(t1, A, t0);           // the norm: an element of Fp (c1 = 0 mod p)
    bool started = false;
    for (int i = NL - 1; i >= 0; i--) {
      const uint32_t e = pm2_limb<F>(i);
      for (int b = LB - 1; b >= 0; b--) {
        if (started) mul(D, D, D);
        if (e >> b & 1) {
          if (started) mul(D, D, t1);
          else {
            copy(D, t1);
            started = true;
          }
        }
      }
    }
    mul(D, D, t0);
  }
  // the inverse in Fp6 = Fp2[v]/(v^3 - xi) of (c0, c1, c2), slots not in a row: the adjugate over the norm
  void f6_inv(uint16_t r0, uint16_t r1, uint16_t r2, uint16_t c0, uint16_t c1, uint16_t c2) {
    const uint16_t t0 = PR_TMP, t1 = PR_TMP + 1, t2 = PR_TMP + 2, x = PR_TMP + 3, y = PR_TMP + 4, d = PR_TMP + 5, di = PR_TMP + 6;
    mul(t0, c0, c0); mul(x, c1, c2); mulxi(x, x); sub(t0, t0, x);      // c0^2 - xi c1 c2
    mul(t1, c2, c2); mulxi(t1, t1); mul(x, c0, c1); sub(t1, t1, x);    // xi c2^2 - c0 c1
    mul(t2, c1, c1); mul(x, c0, c2); sub(t2, t2, x);                   // c1^2 - c0 c2
    mul(x, c2, t1); mul(y, c1, t2); add(x, x, y); mulxi(x, x);
    mul(d, c0, t0); add(d, d, x);                                      // the norm to Fp2
    f2_inv(di, d, PR_TMP + 7, PR_TMP + 8);
    mul(r0, t0, di); mul(r1, t1, di); mul(r2, t2, di);
  }
  // R = A^-1 (S: a spare region): conj(A) / (A conj(A)), the denominator in Fp6
  void f12_inv(uint16_t R, uint16_t S, uint16_t A) {
    f12_conj(S, A);
    f12_mul(R, A, S);   // the odd coefficients are 0
    f6_inv(R + 0, R + 2, R + 4, R + 0, R + 2, R + 4);
    for (int k = 1; k < 6; k += 2) copy(R + k, PR_C_ZERO);
    f12_copy(PR_LINE, R);
    f12_mul(R, S, PR_LINE, 0x15);
  }

  // ---- the steps on the twist: T in (PR_TX, PR_TY, PR_TZ), the line in PR_LINE at the family's three places ----
  static constexpr int L_YP = Fam::M_TWIST ? 3 : 0, L_XP = Fam::M_TWIST ? 2 : 1, L_C = Fam::M_TWIST ? 0 : 3;
  static constexpr unsigned LINE_MASK = (1u << L_YP) | (1u << L_XP) | (1u << L_C);
  void step_double() {
    const uint16_t X = PR_TX, Y = PR_TY, Z = PR_TZ, t = PR_TMP;
    const uint16_t xx = t, s = t + 1, w = t + 2, ss = t + 3, sss = t + 4, r = t + 5, rr = t + 6, b = t + 7, h = t + 8, u = t + 9;
    mul(xx, X, X);
    mul(s, Y, Z); add(s, s, s);
    add(w, xx, xx); add(w, w, xx);
    mul(ss, s, s); mul(sss, s, ss);
    mul(r, Y, s); mul(rr, r, r);
    mul(b, X, r); add(b, b, b);
    mul(h, w, w); sub(h, h, b); sub(h, h, b);
    mul(u, s, Z); mul(PR_LINE + L_YP, u, PR_PY);
    mul(u, w, Z); mul(u, u, PR_PX); neg(PR_LINE + L_XP, u);
    mul(u, w, X); sub(PR_LINE + L_C, u, r);
    mul(X, h, s);
    sub(u, b, h); mul(u, w, u); add(rr, rr, rr); sub(Y, u, rr);
    copy(Z, sss);
  }
  void step_add() {
    const uint16_t X = PR_TX, Y = PR_TY, Z = PR_TZ, t = PR_TMP;
    const uint16_t u = t, v = t + 1, uu = t + 2, vv = t + 3, vvv = t + 4, r = t + 5, a = t + 6, x = t + 7, y = t + 8;
    mul(u, PR_QY, Z); sub(u, u, Y);
    mul(v, PR_QX, Z); sub(v, v, X);
    mul(uu, u, u); mul(vv, v, v); mul(vvv, v, vv); mul(r, vv, X);
    mul(a, uu, Z); sub(a, a, vvv); sub(a, a, r); sub(a, a, r);
    mul(PR_LINE + L_YP, v, PR_PY);
    mul(x, u, PR_PX); neg(PR_LINE + L_XP, x);
    mul(x, u, PR_QX); mul(y, v, PR_QY); sub(PR_LINE + L_C, x, y);
    mul(X, v, a);
    sub(x, r, a); mul(x, u, x); mul(y, vvv, Y); sub(Y, x, y);
    mul(Z, vvv, Z);
  }
  // f_{|x|,Q}(P), conjugated for a negative x, 1 for a flagged pair; then ACC *= it.  P, Q are in their slots.
  void miller() {
    for (uint16_t c : {PR_PX, PR_PY, PR_QX, PR_QY}) mulr(c, PR_C_IN, c);   // the images' Montgomery radix 2^384 to the internal 2^392
    copy(PR_TX, PR_QX);
    copy(PR_TY, PR_QY);
    copy(PR_TZ, PR_C_ONE);
    uint16_t f = PR_F, g = PR_G;
    bool one = true;   // f is still 1: the first square and product are free
    for (int b = 62; b >= 0; b--) {
      if (!one) {
        f12_sqr(g, f);
        std::swap(f, g);
      }
      for (int pass = 0; pass < 1 + (int)(Fam::X >> b & 1); pass++) {
        if (pass) step_add(); else step_double();
        if (one) {
          for (int k = 0; k < 6; k++) copy(f + k, (LINE_MASK >> k & 1) ? PR_LINE + k : PR_C_ZERO);
          one = false;
        } else {
          f12_mul(g, f, PR_LINE, LINE_MASK);
          std::swap(f, g);
        }
      }
    }
    if (Fam::X_NEG) f12_conj(f, f);
    for (int k = 0; k < 6; k++) selc(f + k, k ? PR_C_ZERO : PR_C_ONE);
    f12_mul(g, PR_ACC, f);
    f12_copy(PR_ACC, g);
  }
  // ACC *= F (a level of the product tree)
  void accumulate() {
    f12_mul(PR_G, PR_ACC, PR_F);
    f12_copy(PR_ACC, PR_G);
  }
  // F = F^(3 (p^12 - 1) / r): bls12.rs final_exponentiation, its names kept
  void final_exponentiation() {
    auto reg = [](int i) { return (uint16_t)(PR_REGION0 + 6 * i); };
    const uint16_t f = PR_F, r = reg(0), y0 = reg(1), y1 = reg(2), y2 = reg(3), y3 = reg(4), y4 = reg(5), y5 = reg(6), sp = reg(7), t = PR_G, t2 = PR_ACC;
    // the easy part: r = f^((p^6 - 1)(p^2 + 1))
    f12_inv(y0, sp, f);            // y0 = f^-1
    f12_conj(y1, f);
    f12_mul(y2, y1, y0);           // f^(p^6 - 1)
    f12_frobenius(y3, y2, 2);
    f12_mul(r, y3, y2);
    // the hard part
    f12_cyclotomic_sqr(y0, r); f12_conj(y0, y0);
    f12_cyclotomic_exp(y5, sp, r);
    f12_cyclotomic_sqr(y1, y5);
    f12_mul(y3, y0, y5);
    f12_cyclotomic_exp(y0, sp, y3);
    f12_cyclotomic_exp(y2, sp, y0);
    f12_cyclotomic_exp(y4, sp, y2);
    f12_mul(t, y4, y1); f12_copy(y4, t);
    f12_cyclotomic_exp(y1, sp, y4);
    f12_conj(y3, y3);
    f12_mul(t, y1, y3); f12_mul(y1, t, r);
    f12_conj(y3, r);
    f12_mul(t, y0, r); f12_frobenius(y0, t, 3);
    f12_mul(t, y4, y3); f12_frobenius(y4, t, 1);
    f12_mul(t, y5, y2); f12_frobenius(y5, t, 2);
    f12_mul(t, y5, y0); f12_mul(t2, t, y4); f12_mul(f, t2, y1);
    for (int k = 0; k < 6; k++) mul(f + k, f + k, PR_C_OUT);   // to the radix of the image (or, canonical, out of Montgomery form)
  }
};

// the constant table of a family, internal form (class M): 0, 1, gamma[j][k], then the two factors of the ABI boundary as elements of Fp
// -- 2^400 mod p on the way in; on the way out 2^384 mod p for Montgomery images, the integer 1 for canonical ones
template <class E>
inline void pr_consts(Fe2 (&out)[PR_CONSTS], bool canonical) {
  using F = typename E::Fld;
  const Modulus<F> md;
  E::zero(out[0]);
  E::set_one(out[1]);
  for (int i = 0; i < 15; i++) E::from_plain(out[2 + i], PrFamily<E>::K::FROB[i], md);
  E::zero(out[17]);
  fe_set(out[17].c0, F::CIN);
  E::zero(out[18]);
  if (canonical) out[18].c0.v[0] = 1;
  else fe_set(out[18].c0, F::COUT);
}

// ---- the plan of a call: how n pairs in groups of `group` become lanes -------------------------------------------------------------
// A group up to PR_SERIAL_GROUP pairs is one item: one lane walks its pairs.  A larger one is `parts` items of `run` pairs each, and
// the items' values are multiplied as a tree of fan-in PR_FAN_IN across lanes and blocks; the order is fixed by the indices alone.
// A chunk is as many whole groups as PR_MAX_ITEMS items hold (at least one).
struct PrPlan {
  uint64_t n, group, groups, run, parts, chunk_groups;
};
inline PrPlan pr_plan(uint64_t n, uint64_t group) {
  PrPlan p{};
  p.n = n;
  p.group = group;
  p.groups = group ? n / group : 0;
  if (group <= PR_SERIAL_GROUP) {
    p.run = group;
    p.parts = 1;
  } else {
    p.run = (group + PR_MAX_ITEMS - 1) / PR_MAX_ITEMS;
    p.parts = (group + p.run - 1) / p.run;
  }
  p.chunk_groups = p.parts ? PR_MAX_ITEMS / p.parts : 0;
  if (p.chunk_groups < 1) p.chunk_groups = 1;
  if (p.chunk_groups > p.groups) p.chunk_groups = p.groups;
  return p;
}

enum : uint32_t { kPrCanonical = 1u, kPrDevice = 2u, kPrCheck = 0x100u /* internal: one byte per group instead of an image */ };

// what the three stages of one chunk share
struct PrRun {
  const PrOp* miller; uint32_t miller_len;
  const PrOp* accum; uint32_t accum_len;
  const PrOp* fexp; uint32_t fexp_len;
  const Fe2* consts;                   // of the output form of the call (pr_consts)
  uint32_t* ws; uint64_t pitch;        // items of the chunk (Miller loops and the product tree): PR_MILLER_SLOTS slots a lane
  uint32_t* ws_f; uint64_t pitch_f;    // groups of the chunk (final exponentiation): PR_SLOTS slots a lane
  const uint8_t* g1; uint64_t g1_stride;
  const uint8_t* g2; uint64_t g2_stride;
  uint8_t* out;                        // the chunk's first image or check byte
  uint64_t first_pair;                 // of the chunk
  uint64_t group, run, parts, groups;  // groups: of this chunk
  uint64_t stride;                     // of the product level at hand
  uint32_t flags;
};

MSM_HD uint32_t pr_word(const uint8_t* p, uint32_t i) { return ((const uint32_t*)p)[i]; }

// stage 1, item `it` of the chunk: the product of the Miller values of its run of pairs, left in its ACC
template <class E>
MSM_HD void pr_miller_lane(const PrRun& p, uint64_t it) {
  using F = typename E::Fld;
  const typename E::Md md;
  const PrWs ws{p.ws, (uint32_t)p.pitch, (uint32_t)it};
  Fe one, zero;
  fe_set(one, F::ONE);
  fe_zero(zero);
#pragma unroll 1
  for (uint32_t k = 0; k < 12; k++) pr_store_fe(ws, PR_ACC + k / 2, k & 1, k == 0 ? one : zero);
  const uint64_t gi = it / p.parts, part = it % p.parts;
  const uint64_t lo = part * p.run, hi = lo + p.run < p.group ? lo + p.run : p.group;
#pragma unroll 1
  for (uint64_t q = lo; q < hi; q++) {
    const uint64_t pair = p.first_pair + gi * p.group + q;
    const uint8_t* a = p.g1 + pair * p.g1_stride;
    const uint8_t* b = p.g2 + pair * p.g2_stride;
    const bool flag = a[96] != 0 || b[192] != 0;   // the flag byte is authoritative
    // six coordinates as raw limbs: xP, yP, xQ.c0, xQ.c1, yQ.c0, yQ.c1 (the program's first products convert them)
#pragma unroll 1
    for (uint32_t c = 0; c < 6; c++) {
      const uint8_t* src = c < 2 ? a + 48 * c : b + 48 * (c - 2);
      uint32_t w[12];
#pragma unroll
      for (uint32_t i = 0; i < 12; i++) w[i] = pr_word(src, i);
      Fe x;
      fe_from_words(x, w);
      x.v[NL - 1] &= (1u << 17) - 1;   // bits 381 .. 383 of a coordinate are ignored: a canonical one has none, and junk stays below 32p
      if (c < 2) {
        pr_store_fe(ws, PR_PX + c, 0, x);
        pr_store_fe(ws, PR_PX + c, 1, zero);
      } else {
        pr_store_fe(ws, PR_QX + (c - 2) / 2, c & 1, x);
      }
    }
    pr_exec<E>(ws, p.miller, p.miller_len, p.consts, flag, md);
  }
}

// stage 2, one level: lane `t` multiplies up to PR_FAN_IN values `stride` items apart into the first
template <class E>
MSM_HD void pr_product_lane(const PrRun& p, uint64_t t) {
  const typename E::Md md;
  const uint64_t span = p.stride * PR_FAN_IN, per_group = (p.parts + span - 1) / span;
  const uint64_t gi = t / per_group, first = (t % per_group) * span;
  const PrWs ws{p.ws, (uint32_t)p.pitch, (uint32_t)(gi * p.parts + first)};
#pragma unroll 1
  for (uint32_t k = 1; k < PR_FAN_IN; k++) {
    const uint64_t other = first + k * p.stride;
    if (other >= p.parts) break;
    const PrWs from{p.ws, (uint32_t)p.pitch, (uint32_t)(gi * p.parts + other)};
#pragma unroll 1
    for (uint32_t c = 0; c < 12; c++) {
      Fe x;
      pr_load_fe(x, from, PR_ACC + c / 2, c & 1);
      pr_store_fe(ws, PR_F + c / 2, c & 1, x);
    }
    pr_exec<E>(ws, p.accum, p.accum_len, p.consts, false, md);
  }
}

// stage 3, group `gi` of the chunk: the final exponentiation and the image (or the check byte)
template <class E>
MSM_HD void pr_final_lane(const PrRun& p, uint64_t gi) {
  using F = typename E::Fld;
  const typename E::Md md;
  const PrWs ws{p.ws_f, (uint32_t)p.pitch_f, (uint32_t)gi};
  const PrWs from{p.ws, (uint32_t)p.pitch, (uint32_t)(gi * p.parts)};
#pragma unroll 1
  for (uint32_t c = 0; c < 12; c++) {
    Fe x;
    pr_load_fe(x, from, PR_ACC + c / 2, c & 1);
    pr_store_fe(ws, PR_F + c / 2, c & 1, x);
  }
  // (a Miller value of 0 -- impossible for points of order r -- stays 0 through the inverse and the chain: the all-zero image)
  pr_exec<E>(ws, p.fexp, p.fexp_len, p.consts, false, md);
  // twelve elements in arkworks' order: c0 = (a0, a2, a4), c1 = (a1, a3, a5); the program left them in the radix of the image
  const bool check = (p.flags & kPrCheck) != 0;
  bool is_one = true;
#pragma unroll 1
  for (uint32_t t = 0; t < 12; t++) {
    const uint32_t e = t >> 1, slot = 2 * (e % 3) + e / 3;
    Fe x;
    pr_load_fe(x, ws, PR_F + slot, t & 1);
    fe_reduce<F>(x);
    uint32_t w[12];
    fe_to_words(w, x);
    if (check) {
#pragma unroll
      for (uint32_t i = 0; i < 12; i++) is_one = is_one && w[i] == (t == 0 && i == 0 ? 1u : 0u);
    } else {
      uint32_t* dst = (uint32_t*)(p.out + gi * PR_GT_BYTES) + 12 * t;
#pragma unroll
      for (uint32_t i = 0; i < 12; i++) dst[i] = w[i];
    }
  }
  if (check) p.out[gi] = is_one ? 1 : 0;
}

// The launches of one call, shared by the engine and the host build.  RUN has miller(PrRun, items), product(PrRun, lanes) and
// final(PrRun, groups).  `base` holds the programs, the constants, the workspaces and the inputs; out_unit: bytes per group.
template <class RUN>
void pr_chain(RUN& run, const PrRun& base, const PrPlan& pl, uint8_t* out, size_t out_unit) {
  for (uint64_t g0 = 0; g0 < pl.groups; g0 += pl.chunk_groups) {
    PrRun p = base;
    p.groups = pl.groups - g0 < pl.chunk_groups ? pl.groups - g0 : pl.chunk_groups;
    p.first_pair = g0 * pl.group;
    p.out = out + g0 * out_unit;
    run.miller(p, p.groups * pl.parts);
    for (uint64_t s = 1; s < pl.parts; s *= PR_FAN_IN) {
      p.stride = s;
      const uint64_t span = s * PR_FAN_IN;
      run.product(p, p.groups * ((pl.parts + span - 1) / span));
    }
    run.final(p, p.groups);
  }
}

// words of the two workspaces for a plan
inline uint64_t pr_ws_items(const PrPlan& pl) { return pl.chunk_groups * pl.parts; }
inline uint64_t pr_ws_words(const PrPlan& pl) { return pr_ws_items(pl) * PR_MILLER_SLOTS * PR_FE2_WORDS; }
inline uint64_t pr_wsf_words(const PrPlan& pl) { return pl.chunk_groups * (uint64_t)PR_SLOTS * PR_FE2_WORDS; }

#if defined(__HIPCC__)
template <class E>
__global__ void __launch_bounds__(PR_LANES) __attribute__((amdgpu_waves_per_eu(2, 2))) k_pairing_miller(PrRun p, uint64_t items) {
  const uint64_t i = (uint64_t)blockIdx.x * PR_LANES + threadIdx.x;
  if (i < items) pr_miller_lane<E>(p, i);
}
template <class E>
__global__ void __launch_bounds__(PR_LANES) __attribute__((amdgpu_waves_per_eu(2, 2))) k_pairing_product(PrRun p, uint64_t lanes) {
  const uint64_t i = (uint64_t)blockIdx.x * PR_LANES + threadIdx.x;
  if (i < lanes) pr_product_lane<E>(p, i);
}
template <class E>
__global__ void __launch_bounds__(PR_LANES) __attribute__((amdgpu_waves_per_eu(2, 2))) k_pairing_final(PrRun p, uint64_t groups) {
  const uint64_t i = (uint64_t)blockIdx.x * PR_LANES + threadIdx.x;
  if (i < groups) pr_final_lane<E>(p, i);
}
#endif

}  // namespace msm
