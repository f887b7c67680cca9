// h2c.hpp -- batch hash-to-curve for BLS12-381 G1 and G2 (RFC 9380, suites BLS12381G1_XMD:SHA-256_SSWU_RO_ and
// BLS12381G2_XMD:SHA-256_SSWU_RO_, and their _NU_ forms): what arkworks calls DefaultFieldHasher<Sha256, 128>::hash_to_field,
// WBMap::map_to_curve and MapToCurveBasedHasher::hash (ARK ff/src/fields/field_hashers, ec/src/hashing).  Only the names and the
// contract are arkworks'; the algorithm is the device's:
//
//   expand   one lane per message: expand_message_xmd (RFC 9380 5.3.1) and the reduction modulo p.  SHA-256 stays in registers --
//            eight state words and a rolling 16-word schedule whose 16 slots are named by constants (the loop over the four groups of
//            16 rounds is rolled, a group is not: a schedule indexed by the round would live in memory).  Message bytes come from
//            device memory through the offsets; the first block of b_0 is 64 zero bytes, its state a constant computed at create; a
//            lane runs as many blocks as its message needs, so a wave runs as many as its longest.  Meant for short messages
//            (32 .. 200 bytes): a lane per message is a poor shape for kilobyte messages.  Each 64-byte string is hi 2^256 + lo with
//            both halves below p; it becomes a Montgomery image by two conversions and one product with the image of 2^256.
//   map      one lane per u: the straight-line simplified SWU of RFC 9380 appendix F.2, division-free, with sqrt_ratio as ONE
//            exponentiation (the p = 3 mod 4 form for G1, the q = 9 mod 16 form for Fp2; tools/gen_h2c_consts.py states both as one
//            formula), sgn0 as the RFC defines it for m = 1 and m = 2, then the isogeny as Horner evaluations on the projective
//            x = xn/xd: with the map written x_num/h^2, y y_num/h^3 (h monic, the kernel polynomial) and Z = xd H the result is the
//            XYZZ point (XN xd, y YN xd^3, Z^2, Z^3) with no inversion.  The special cases are computed, not branched away: tv1 == 0
//            (which includes u = 0) selects x1 = B/(Z A); a vanishing H gives ZZ = 0, which is infinity.
//   clear    one lane per output: the pair sum by the general xyzz_add (which handles Q0 = +-Q1), then the cofactor.  G1: h_eff =
//            1 - z, 64 bits, double-and-add.  G2: Budroni-Pintore, [z^2 - z - 1]Q + [z - 1]psi(Q) + psi^2(2Q), which equals
//            h_eff Q for EVERY point of the curve (the host test compares with plain double-and-add by the 636-bit h_eff off the
//            subgroup): two 64-bit multiplications.  Points that are not in use wait in the lane's slots of the work buffer.
//   Fp2      over Fp2 the map and the clearing keep EVERY value in the lane's slots between products (below, "over Fp2"): that is
//            what fits two waves per SIMD; the arithmetic is the same, operation for operation.
//   output   k_fb_normalize of fixed_base.hpp as it stands.
//
// Every per-element step is an MSM_HD function, so the host build (host_test_api.cpp, ht_h2c_*) runs the same code under MSM_CHECK.
// Limb bounds: every value that enters a product is class M, or a sum / difference of at most three class-M values (value < 4.5p,
// limbs < 2^30), which is within the contract of E::mul; Horner steps are E::mul2, whose output (< 4p, carried) is its own input class.
#pragma once
#include "point_mul.hpp"
#include "sqrt.hpp"

namespace msm {

#include "h2c_consts.inc"

template <class E>
struct H2cConsts;
template <>
struct H2cConsts<FpEl<Bls12_381_Fq>> : H2c_381_G1 {};
template <>
struct H2cConsts<Fp2El<Bls12_381_Fq, 1>> : H2c_381_G2 {};

constexpr uint32_t H2C_LANES = 256;
constexpr uint32_t H2C_MAX_LANES = 1u << 17;   // lanes in flight of one chunk: the work buffers are sized by this, never by n
constexpr uint32_t H2C_MAX_DST = 255;
constexpr uint32_t H2C_H_EFF_G1[2] = {0x00010001u, 0xd2010000u};   // 1 - z

// ---- SHA-256 -------------------------------------------------------------------------------------------------------------------
struct H2cShaK {
  static constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
      0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
      0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
      0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
      0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
      0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  static constexpr uint32_t IV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
};

MSM_HD uint32_t h2c_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

MSM_HD void h2c_sha_iv(uint32_t (&h)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = H2cShaK::IV[i];
}

// one compression; w is consumed (it ends as the schedule words 64 .. 79, which nobody reads)
MSM_HD void h2c_sha_block(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll 1
  for (int j = 0; j < 4; j++) {
    const uint32_t* k = H2cShaK::K + 16 * j;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint32_t t1 = hh + (h2c_rotr(e, 6) ^ h2c_rotr(e, 11) ^ h2c_rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[i] + w[i];
      const uint32_t t2 = (h2c_rotr(a, 2) ^ h2c_rotr(a, 13) ^ h2c_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
      // slot i now takes word t + 16 = w[t] + s0(w[t + 1]) + w[t + 9] + s1(w[t + 14]); the three are in their slots, old or new
      const uint32_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
      w[i] += (h2c_rotr(x, 7) ^ h2c_rotr(x, 18) ^ (x >> 3)) + w[(i + 9) & 15] + (h2c_rotr(y, 17) ^ h2c_rotr(y, 19) ^ (y >> 10));
    }
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// Absorb bytes [0, len) of a stream and the padding, after `done` bytes (a multiple of 64) that the state h already holds.
// S::word(pos) gives the big-endian word of bytes pos .. pos + 3 with 0x80 at position len and zero beyond.
template <class S>
MSM_HD void h2c_sha_finish(uint32_t (&h)[8], uint32_t done, uint32_t len, const S& s) {
  const uint32_t nblk = (len + 9 + 63) >> 6;
#pragma unroll 1
  for (uint32_t b = 0; b < nblk; b++) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = s.word(64 * b + 4 * (uint32_t)k);
    if (b == nblk - 1) {
      const uint64_t bits = ((uint64_t)done + len) * 8;
      w[14] = (uint32_t)(bits >> 32);
      w[15] = (uint32_t)bits;
    }
    h2c_sha_block(h, w);
  }
}

// What a handle knows of its domain separation tag: DST_prime = DST || len(DST) in memory the kernel can read (device memory for
// the kernels, host memory for the host build), and the state after the 64 zero bytes that open b_0.
struct H2cDst {
  uint32_t z_pad[8];
  const uint8_t* prime;
  uint32_t prime_len;   // 2 .. 256
};

// msg || I2OSP(len_in_bytes, 2) || 0 || DST_prime
struct H2cStream0 {
  const uint8_t* msg;
  uint32_t mlen, lib;
  const uint8_t* prime;
  uint32_t prime_len;
  MSM_HD uint32_t len() const { return mlen + 3 + prime_len; }
  MSM_HD uint32_t byte(uint32_t pos) const {
    if (pos < mlen) return msg[pos];
    const uint32_t q = pos - mlen;
    if (q == 0) return lib >> 8;
    if (q == 1) return lib & 0xff;
    if (q == 2) return 0;
    if (q - 3 < prime_len) return prime[q - 3];
    return q - 3 == prime_len ? 0x80u : 0u;
  }
  MSM_HD uint32_t word(uint32_t pos) const {
    if (pos + 4 <= mlen) return ((uint32_t)msg[pos] << 24) | ((uint32_t)msg[pos + 1] << 16) | ((uint32_t)msg[pos + 2] << 8) | msg[pos + 3];
    return (byte(pos) << 24) | (byte(pos + 1) << 16) | (byte(pos + 2) << 8) | byte(pos + 3);
  }
};

// (b_0 xor b_(i-1)) || i || DST_prime
struct H2cStreamI {
  uint32_t head[8];
  uint32_t index;
  const uint8_t* prime;
  uint32_t prime_len;
  MSM_HD uint32_t len() const { return 33 + prime_len; }
  MSM_HD uint32_t byte(uint32_t pos) const {
    const uint32_t q = pos - 32;
    if (q == 0) return index;
    if (q - 1 < prime_len) return prime[q - 1];
    return q - 1 == prime_len ? 0x80u : 0u;
  }
  MSM_HD uint32_t word(uint32_t pos) const {
    if (pos < 32) {
      uint32_t r = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) r = (pos == 4u * k) ? head[k] : r;
      return r;
    }
    return (byte(pos) << 24) | (byte(pos + 1) << 16) | (byte(pos + 2) << 8) | byte(pos + 3);
  }
};

// SHA-256 of a byte string in host or device memory (create: the oversize DST; the host tests)
MSM_HD void h2c_sha256(uint32_t (&h)[8], const uint8_t* data, uint32_t len) {
  struct Plain {
    const uint8_t* p;
    uint32_t n;
    MSM_HD uint32_t byte(uint32_t pos) const { return pos < n ? p[pos] : (pos == n ? 0x80u : 0u); }
    MSM_HD uint32_t word(uint32_t pos) const { return (byte(pos) << 24) | (byte(pos + 1) << 16) | (byte(pos + 2) << 8) | byte(pos + 3); }
  } s{data, len};
  h2c_sha_iv(h);
  h2c_sha_finish(h, 0, len, s);
}

// a 32-byte digest as a big-endian integer -> class M
template <class F>
MSM_HD void h2c_digest_to_fe(Fe& r, const uint32_t (&h)[8], const Modulus<F>& md) {
  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = h[7 - k];
#pragma unroll
  for (int k = 8; k < 12; k++) w[k] = 0;
  FpEl<F>::from_plain(r, w, md);
}

// The reduction of hash_to_field: the 64-byte string hi || lo (two digests, big-endian: OS2IP gives hi 2^256 + lo, both halves below
// 2^256 < p) -> the ABI image of its residue, 12 words.  Two conversions and one product with the image of 2^256; the sum is below
// 3p with limbs below 2^29, which fe_to_abi takes.  The kernel and the host build call this one function.
template <class F>
MSM_HD void h2c_reduce(uint32_t* out, const uint32_t (&hi)[8], const uint32_t (&lo)[8], const Modulus<F>& md) {
  Fe a, b, two256, t, sum;
  h2c_digest_to_fe<F>(a, hi, md);
  h2c_digest_to_fe<F>(b, lo, md);
  fe_set(two256, H2c_381_Common::TWO_256);
  fe_mul<F>(t, a, two256, md);
  fe_add(sum, t, b);                  // < 3p, limbs < 2^29
  fe_to_abi<F>(out, sum, md);
}

// hash_to_field of one message: `elems` = count * m base-field images, 12 words each, at out.  elems is 1, 2 or 4.
template <class F>
MSM_HD void h2c_expand(uint32_t* out, const uint8_t* msg, uint32_t mlen, uint32_t elems, const H2cDst& dst, const Modulus<F>& md) {
  uint32_t b0[8], prev[8], hi[8];
#pragma unroll
  for (int k = 0; k < 8; k++) b0[k] = dst.z_pad[k];
  {
    const H2cStream0 s{msg, mlen, 64 * elems, dst.prime, dst.prime_len};
    h2c_sha_finish(b0, 64, s.len(), s);
  }
#pragma unroll
  for (int k = 0; k < 8; k++) prev[k] = hi[k] = 0;
#pragma unroll 1
  for (uint32_t i = 1; i <= 2 * elems; i++) {
    H2cStreamI s;
#pragma unroll
    for (int k = 0; k < 8; k++) s.head[k] = b0[k] ^ prev[k];
    s.index = i;
    s.prime = dst.prime;
    s.prime_len = dst.prime_len;
    h2c_sha_iv(prev);
    h2c_sha_finish(prev, 0, s.len(), s);
    if (i & 1) {
#pragma unroll
      for (int k = 0; k < 8; k++) hi[k] = prev[k];
    } else {
      h2c_reduce<F>(out + 12 * ((i >> 1) - 1), hi, prev, md);
    }
  }
}

// ---- the map -------------------------------------------------------------------------------------------------------------------
MSM_HD void h2c_load(Fe& r, const uint32_t (*c)[NL]) {
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = c[0][i];
}
MSM_HD void h2c_load(Fe2& r, const uint32_t (*c)[NL]) {
#pragma unroll
  for (int i = 0; i < NL; i++) {
    r.c0.v[i] = c[0][i];
    r.c1.v[i] = c[1][i];
  }
}

// sgn0 of RFC 9380 section 4.1 from the canonical integers
template <class E>
MSM_HD uint32_t h2c_sgn0(const typename E::T& a, const typename E::Md& md) {
  uint32_t w[E::WORDS];
  E::to_plain(w, a, md);
  if constexpr (E::WORDS == 12) {
    return w[0] & 1;
  } else {
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) nz |= w[i];
    return nz ? (w[0] & 1) : (w[12] & 1);
  }
}

// r = a^e for the constant e of `bits` bits (2-bit digits from the top, as fe_pow_const); a, r class M
template <class E, int NW>
MSM_HD void h2c_pow_const(typename E::T& r, const typename E::T& a, const uint32_t (&w)[NW], int bits, const typename E::Md& md) {
  typename E::T a2, a3, acc;
  E::sqr(a2, a, md);
  E::mul(a3, a2, a, md);
  const int top = (bits - 1) >> 1;
  {
    const uint32_t d = (check_scalar_word<NW>(w, top >> 4) >> ((top & 15) * 2)) & 3;
    acc = d == 1 ? a : (d == 2 ? a2 : a3);
  }
#pragma unroll 1
  for (int i = top - 1; i >= 0; i--) {
    E::sqr(acc, acc, md);
    E::sqr(acc, acc, md);
    const uint32_t d = (check_scalar_word<NW>(w, i >> 4) >> ((i & 15) * 2)) & 3;
    if (d) {   // wave-uniform
      const typename E::T m = d == 1 ? a : (d == 2 ? a2 : a3);
      E::mul(acc, acc, m, md);
    }
  }
  r = acc;
}

// (is_square, y) with y^2 = u/v when u/v is a square and y^2 = Z u/v otherwise; u, v class M, v != 0.  u == 0 gives (true, 0).
// The p = 3 (mod 4) form (S = 1); over Fp2 (S = 3) h2c_sqrt_ratio_slots below does the same through the lane's slots.
template <class E>
MSM_HD bool h2c_sqrt_ratio(typename E::T& y, const typename E::T& u, const typename E::T& v, const typename E::Md& md) {
  using K = H2cConsts<E>;
  using T = typename E::T;
  static_assert(K::S == 1, "the register form is written for p = 3 (mod 4)");
  T pre, w, g, zu, zc;
  {
    T v2;
    E::sqr(v2, v, md);
    E::mul(pre, u, v, md);            // u v
    E::mul(w, pre, v2, md);           // u v^3
  }
  h2c_pow_const<E, K::EXP_WORDS>(g, w, K::EXP, K::EXP_BITS, md);
  E::mul(g, g, pre, md);              // gamma: gamma^2 v / u is a root of unity of order 2^S
  h2c_load(zc, K::Z);
  E::mul(zu, zc, u, md);
  bool found = false, square = false;
  E::zero(y);
#pragma unroll 1
  for (int k = 0; k < 2 * K::NROOTS; k++) {
    T c, cand, t;
    h2c_load(c, K::ROOTS[k]);
    E::mul(cand, g, c, md);
    E::sqr(t, cand, md);
    E::mul(t, t, v, md);
    T want = zu;
    E::cmov(want, u, k < K::NROOTS);
    const bool hit = check_equal<E>(t, want) && !found;
    E::cmov(y, cand, hit);
    square = square || (hit && k < K::NROOTS);
    found = found || hit;
  }
  return square;
}

// sum c[i] xn^i xd^(deg - i), i <= deg: Horner, one fused dual product a step.  xn, xd class M; r < 4p, carried limbs.
template <class E, int ROWS>
MSM_HD void h2c_horner(typename E::T& r, const uint32_t (&c)[ROWS][H2cConsts<E>::M][NL], const typename E::T& xn, const typename E::T& xd,
                       const typename E::Md& md) {
  typename E::T acc, pw = xd, k;
  h2c_load(acc, c[ROWS - 1]);
#pragma unroll 1
  for (int i = ROWS - 2; i >= 0; i--) {
    h2c_load(k, c[i]);
    E::mul2(acc, acc, xn, k, pw, md);
    if (i) E::mul(pw, pw, xd, md);
  }
  r = acc;
}

// u (class M) -> the point (xn / xd, y) of E', all three class M but y, which is a carried value of at most 2p
template <class E>
MSM_HD void h2c_sswu(typename E::T& xn, typename E::T& xd, typename E::T& y, const typename E::T& u, const typename E::Md& md) {
  using K = H2cConsts<E>;
  using T = typename E::T;
  using F = typename E::Fld;
  T A, B, one, tv1, tv2, tv3, tv4, tv5, tv6, t, x2n, gxn, y1;
  h2c_load(A, K::A);
  h2c_load(B, K::B);
  E::set_one(one);
  E::sqr(t, u, md);
  h2c_load(tv4, K::Z);
  E::mul(tv1, tv4, t, md);            // Z u^2
  E::sqr(tv2, tv1, md);
  E::add(tv2, tv2, tv1);              // Z^2 u^4 + Z u^2: < 3p, limbs < 2^29
  const bool exceptional = check_is_zero(tv2, (E*)nullptr);
  E::add(t, tv2, one);                // < 4.5p, limbs < 3 * 2^28
  E::mul(tv3, B, t, md);              // B (tv2 + 1)
  E::neg(t, tv2, F::BIAS4_29);        // (p, 4p], limbs < 2^30
  E::mul(tv4, A, t, md);              // -A tv2
  h2c_load(t, K::ZA);
  E::cmov(tv4, t, exceptional);       // Z A when tv2 == 0
  E::sqr(tv2, tv3, md);
  E::sqr(tv6, tv4, md);
  E::mul(tv5, A, tv6, md);
  E::add(tv2, tv2, tv5);              // < 3p
  E::mul(tv2, tv2, tv3, md);
  E::mul(tv6, tv6, tv4, md);          // tv4^3: the denominator of g(x1)
  E::mul(tv5, B, tv6, md);
  E::add(t, tv2, tv5);                // < 3p
  E::mul(gxn, t, one, md);            // the numerator of g(x1), class M
  E::mul(x2n, tv1, tv3, md);
  const bool square = h2c_sqrt_ratio<E>(y1, gxn, tv6, md);
  xn = x2n;
  E::mul(t, tv1, u, md);
  E::mul(y, t, y1, md);
  E::cmov(xn, tv3, square);
  E::cmov(y, y1, square);
  {
    const bool flip = h2c_sgn0<E>(u, md) != h2c_sgn0<E>(y, md);
    T ny;
    E::neg(ny, y, F::BIAS2_28);       // (0, 2p], limbs < 2^29
    E::carry(ny);
    E::cmov(y, ny, flip);
  }
  xd = tv4;
}

// The isogeny E' -> E at (xn / xd, y), xd != 0: (XN xd, y YN xd^3, Z^2, Z^3) with Z = xd H.  xn, xd class M; y up to 2p, limbs < 2^29.
template <class E>
MSM_HD void h2c_iso(XyzzT<typename E::T>& out, const typename E::T& xn, const typename E::T& xd, const typename E::T& y, const typename E::Md& md) {
  using K = H2cConsts<E>;
  using T = typename E::T;
  T XN, H, YN, d2, d3, t;
  h2c_horner<E, 2 * K::DEG_H + 2>(XN, K::X_NUM, xn, xd, md);
  h2c_horner<E, K::DEG_H + 1>(H, K::H, xn, xd, md);
  h2c_horner<E, 3 * K::DEG_H + 1>(YN, K::Y_NUM, xn, xd, md);
  E::mul(out.x, XN, xd, md);
  E::sqr(d2, xd, md);
  E::mul(d3, d2, xd, md);
  E::mul(t, y, YN, md);
  E::mul(out.y, t, d3, md);
  E::mul(t, H, xd, md);               // Z = xd H: zero exactly at a kernel abscissa, where the image is infinity
  E::sqr(out.zz, t, md);
  E::mul(out.zzz, out.zz, t, md);
}

// u (class M) -> the point of E as XYZZ; no cofactor clearing
template <class E>
MSM_HD void h2c_map(XyzzT<typename E::T>& out, const typename E::T& u, const typename E::Md& md) {
  typename E::T xn, xd, y;
  h2c_sswu<E>(xn, xd, y, u, md);
  h2c_iso<E>(out, xn, xd, y, md);
}

// ---- cofactor clearing -----------------------------------------------------------------------------------------------------------
// acc = [k] (*base) for the constant k whose top set bit is `top`; the base is read again at every addition, so that it is not live
// across the doublings
template <class E, int NW>
MSM_HD void h2c_mul_slot(XyzzT<typename E::T>& acc, const XyzzT<typename E::T>* base, const uint32_t (&w)[NW], int top, const typename E::Md& md) {
  acc = *base;
#pragma unroll 1
  for (int bit = top - 1; bit >= 0; bit--) {
    xyzz_dbl<E>(acc, md);
    if ((check_scalar_word<NW>(w, bit >> 5) >> (bit & 31)) & 1) {
      const XyzzT<typename E::T> b = *base;
      xyzz_add<E>(acc, b, md);
    }
  }
}

// acc = h_eff * acc over Fp: h_eff = 1 - z, 64 bits.  slot: one record that this lane owns (the base of the walk waits there).
// Over Fp2 h2c_clear_slots below runs Budroni-Pintore's chain.
template <class E>
MSM_HD void h2c_clear(XyzzT<typename E::T>& acc, XyzzT<typename E::T>* slot, const typename E::Md& md) {
  static_assert(E::WORDS == 12, "the register form is written for G1");
  slot[0] = acc;
  h2c_mul_slot<E, 2>(acc, slot, H2C_H_EFF_G1, 63, md);
}

// ---- over Fp2: values wait in the lane's slots between products ----------------------------------------------------------------------
// An Fp2 element is 28 registers, a product needs about a hundred more, and two waves per SIMD leave 256: the map holds eight values
// across its exponentiation and the general addition two points of four.  So over Fp2 every named value lives in a slot of the
// lane's work memory (slot k of lane i at [k * pitch + i], as the pairing workspace is laid out), a step loads its operands, computes
// and stores, and at most four values are live in registers at any product.  The map's arithmetic and limb bounds are those of
// h2c_sswu / h2c_horner / h2c_iso above, the group law's those of xyzz_dbl / xyzz_add in curve.hpp, operation for operation; only
// where a value waits has changed.  (A change to xyzz_dbl or xyzz_add must be made in h2c_slot_dbl / h2c_slot_add as well; curve.hpp
// says so at both.  tests/test_h2c_host.py holds the slot forms to the model and to plain double-and-add.)
// The cofactor chain is a list of steps (double, add, copy, negate, psi) written at compile time and walked by ONE rolled loop, so
// the group law is in the code once.
MSM_HD void h2c_fence() { asm volatile("" ::: "memory"); }   // a slot is re-read from memory, never kept in registers across steps

struct H2cMem {
  Fe2* p;
  size_t pitch;
  MSM_HD Fe2 get(int k) const {
    h2c_fence();
    return p[(size_t)k * pitch];
  }
  MSM_HD void put(int k, const Fe2& v) const {
    p[(size_t)k * pitch] = v;
    h2c_fence();
  }
};

// slots of the map
enum { HS_U = 0, HS_TV1, HS_TV3, HS_XD, HS_X2N, HS_GXN, HS_TV6, HS_PRE, HS_W, HS_A2, HS_A3, HS_G, HS_ZU, HS_Y, HS_XN, HS_T0, HS_T1, H2C_MAP_SLOTS };
// slots of the clearing: five points of four coordinates, then the temporaries of the group law
enum { HP_ACC = 0, HP_Q = 4, HP_T1 = 8, HP_T2 = 12, HP_B = 16, HT_0 = 20, HT_1, HT_2, HT_3, HT_4, HT_5, HT_6, HT_7, H2C_CLEAR_SLOTS };

// HS_GXN = u, HS_TV6 = v (class M, v != 0) -> HS_Y, and whether u / v is a square: h2c_sqrt_ratio with S = 3
template <class E>
MSM_HD bool h2c_sqrt_ratio_slots(const H2cMem& s, const typename E::Md& md) {
  using K = H2cConsts<E>;
  using T = typename E::T;
  static_assert(K::S == 3, "the slot form is written for q = 9 (mod 16)");
  {
    T v = s.get(HS_TV6), v2, v3, v4, v7, pre, w;
    E::sqr(v2, v, md);
    E::mul(v3, v2, v, md);
    E::sqr(v4, v2, md);
    E::mul(v7, v4, v3, md);
    {
      const T u = s.get(HS_GXN);
      E::mul(pre, u, v7, md);           // u v^7
    }
    s.put(HS_PRE, pre);
    E::sqr(v4, v4, md);
    E::mul(w, pre, v4, md);             // u v^15
    s.put(HS_W, w);
    E::sqr(v2, w, md);
    s.put(HS_A2, v2);
    E::mul(v3, v2, w, md);
    s.put(HS_A3, v3);
  }
  {
    // w^EXP, 2-bit digits from the top; the multiplier of a digit comes from its slot
    const int top = (K::EXP_BITS - 1) >> 1;
    const uint32_t d0 = (check_scalar_word<K::EXP_WORDS>(K::EXP, top >> 4) >> ((top & 15) * 2)) & 3;
    T acc = s.get(HS_W + (int)d0 - 1);
#pragma unroll 1
    for (int i = top - 1; i >= 0; i--) {
      E::sqr(acc, acc, md);
      E::sqr(acc, acc, md);
      const uint32_t d = (check_scalar_word<K::EXP_WORDS>(K::EXP, i >> 4) >> ((i & 15) * 2)) & 3;
      if (d) {   // wave-uniform
        const T m = s.get(HS_W + (int)d - 1);
        E::mul(acc, acc, m, md);
      }
    }
    const T pre = s.get(HS_PRE);
    E::mul(acc, acc, pre, md);          // gamma
    s.put(HS_G, acc);
  }
  {
    T zc, zu;
    h2c_load(zc, K::Z);
    const T u = s.get(HS_GXN);
    E::mul(zu, zc, u, md);
    s.put(HS_ZU, zu);
    E::zero(zu);
    s.put(HS_Y, zu);
  }
  bool found = false, square = false;
#pragma unroll 1
  for (int k = 0; k < 2 * K::NROOTS; k++) {
    T c, cand, t;
    h2c_load(c, K::ROOTS[k]);
    {
      const T g = s.get(HS_G);
      E::mul(cand, g, c, md);
    }
    E::sqr(t, cand, md);
    {
      const T v = s.get(HS_TV6);
      E::mul(t, t, v, md);
    }
    const T want = s.get(k < K::NROOTS ? HS_GXN : HS_ZU);
    const bool hit = check_equal<E>(t, want) && !found;
    T y = s.get(HS_Y);
    E::cmov(y, cand, hit);
    s.put(HS_Y, y);
    square = square || (hit && k < K::NROOTS);
    found = found || hit;
  }
  return square;
}

// HS_U = u (class M) -> HS_XN, HS_XD, HS_Y: h2c_sswu
template <class E>
MSM_HD void h2c_sswu_slots(const H2cMem& s, const typename E::Md& md) {
  using K = H2cConsts<E>;
  using T = typename E::T;
  using F = typename E::Fld;
  {
    T c, t, tv1, tv2, tv3, tv4;
    {
      const T u = s.get(HS_U);
      E::sqr(t, u, md);
    }
    h2c_load(c, K::Z);
    E::mul(tv1, c, t, md);              // Z u^2
    s.put(HS_TV1, tv1);
    E::sqr(tv2, tv1, md);
    E::add(tv2, tv2, tv1);              // < 3p, limbs < 2^29
    const bool exceptional = check_is_zero(tv2, (E*)nullptr);
    E::set_one(c);
    E::add(t, tv2, c);                  // < 4.5p
    h2c_load(c, K::B);
    E::mul(tv3, c, t, md);
    s.put(HS_TV3, tv3);
    E::neg(t, tv2, F::BIAS4_29);
    h2c_load(c, K::A);
    E::mul(tv4, c, t, md);
    h2c_load(c, K::ZA);
    E::cmov(tv4, c, exceptional);
    s.put(HS_XD, tv4);
  }
  {
    T c, tv4 = s.get(HS_XD), tv6, tv5;
    E::sqr(tv6, tv4, md);
    h2c_load(c, K::A);
    E::mul(tv5, c, tv6, md);
    s.put(HS_T0, tv5);
    E::mul(tv6, tv6, tv4, md);          // tv4^3
    s.put(HS_TV6, tv6);
    h2c_load(c, K::B);
    E::mul(tv5, c, tv6, md);
    s.put(HS_T1, tv5);
  }
  {
    T tv3 = s.get(HS_TV3), tv2, t, c;
    E::sqr(tv2, tv3, md);
    {
      const T tv5 = s.get(HS_T0);
      E::add(tv2, tv2, tv5);            // < 3p
    }
    E::mul(tv2, tv2, tv3, md);
    {
      const T tv5 = s.get(HS_T1);
      E::add(t, tv2, tv5);              // < 3p
    }
    E::set_one(c);
    E::mul(tv2, t, c, md);              // the numerator of g(x1), class M
    s.put(HS_GXN, tv2);
    {
      const T tv1 = s.get(HS_TV1);
      E::mul(t, tv1, tv3, md);
    }
    s.put(HS_X2N, t);
  }
  const bool square = h2c_sqrt_ratio_slots<E>(s, md);
  {
    T y1 = s.get(HS_Y), t, y;
    {
      const T tv1 = s.get(HS_TV1), u = s.get(HS_U);
      E::mul(t, tv1, u, md);
    }
    E::mul(y, t, y1, md);
    E::cmov(y, y1, square);
    uint32_t su;
    {
      const T u = s.get(HS_U);
      su = h2c_sgn0<E>(u, md);
    }
    const bool flip = su != h2c_sgn0<E>(y, md);
    E::neg(t, y, F::BIAS2_28);          // (0, 2p], limbs < 2^29
    E::carry(t);
    E::cmov(y, t, flip);
    s.put(HS_Y, y);
  }
  {
    T xn = s.get(HS_X2N);
    const T tv3 = s.get(HS_TV3);
    E::cmov(xn, tv3, square);
    s.put(HS_XN, xn);
  }
}

// sum c[i] xn^i xd^(deg - i) from HS_XN, HS_XD: h2c_horner with the two products of a step apart; r < 3p, limbs < 2^29
template <class E, int ROWS>
MSM_HD void h2c_horner_slots(typename E::T& r, const uint32_t (&c)[ROWS][H2cConsts<E>::M][NL], const H2cMem& s, const typename E::Md& md) {
  typename E::T acc, pw = s.get(HS_XD);
  h2c_load(acc, c[ROWS - 1]);
#pragma unroll 1
  for (int i = ROWS - 2; i >= 0; i--) {
    typename E::T t1, t2;
    {
      const typename E::T xn = s.get(HS_XN);
      E::mul(t1, acc, xn, md);
    }
    h2c_load(t2, c[i]);
    E::mul(t2, t2, pw, md);
    E::add(acc, t1, t2);                // < 3p, limbs < 2^29
    if (i) {
      const typename E::T xd = s.get(HS_XD);
      E::mul(pw, pw, xd, md);
    }
  }
  r = acc;
}

// HS_XN, HS_XD, HS_Y -> the point of E in out (memory): h2c_iso
template <class E>
MSM_HD void h2c_iso_slots(XyzzT<typename E::T>* out, const H2cMem& s, const typename E::Md& md) {
  using K = H2cConsts<E>;
  using T = typename E::T;
  {
    T v, r;
    h2c_horner_slots<E, 2 * K::DEG_H + 2>(v, K::X_NUM, s, md);
    const T xd = s.get(HS_XD);
    E::mul(r, v, xd, md);
    out->x = r;
    h2c_fence();
  }
  {
    T v, t, r;
    h2c_horner_slots<E, K::DEG_H + 1>(v, K::H, s, md);
    {
      const T xd = s.get(HS_XD);
      E::mul(t, v, xd, md);             // Z = xd H
    }
    E::sqr(r, t, md);
    out->zz = r;
    h2c_fence();
    E::mul(r, r, t, md);
    out->zzz = r;
    h2c_fence();
  }
  {
    T v, t, r;
    {
      const T xd = s.get(HS_XD);
      E::sqr(t, xd, md);
      E::mul(t, t, xd, md);
    }
    s.put(HS_T0, t);
    h2c_horner_slots<E, 3 * K::DEG_H + 1>(v, K::Y_NUM, s, md);
    {
      const T y = s.get(HS_Y);
      E::mul(t, y, v, md);
    }
    {
      const T d3 = s.get(HS_T0);
      E::mul(r, t, d3, md);
    }
    out->y = r;
    h2c_fence();
  }
}

// ---- the group law on points in slots (x, y, zz, zzz at b .. b + 3) ------------------------------------------------------------------
template <class E>
MSM_HD bool h2c_slot_is_inf(const H2cMem& s, int b) {
  const typename E::T zz = s.get(b + 2);
  return E::is_zero_M(zz);
}

MSM_HD void h2c_slot_copy(const H2cMem& s, int d, int a) {
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    const Fe2 v = s.get(a + k);
    s.put(d + k, v);
  }
}

// xyzz_dbl on the point at a
template <class E>
MSM_HD void h2c_slot_dbl(const H2cMem& s, int a, const typename E::Md& md) {
  using T = typename E::T;
  using F = typename E::Fld;
  {
    T u, v, w;
    {
      const T y = s.get(a + 1);
      E::dbl(u, y);
    }
    E::prep(u);
    E::sqr_c(v, u, md);
    s.put(HT_0, v);
    E::template mul_c<false>(w, u, v, md);
    s.put(HT_1, w);
  }
  {
    T x = s.get(a), sx, m, mm, t;
    {
      const T v = s.get(HT_0);
      E::template mul_c<false>(sx, x, v, md);
    }
    E::sqr_c(t, x, md);
    E::dbl(m, t);
    E::add(m, m, t);                    // 3 XX
    E::carry(m);
    s.put(HT_2, m);
    E::sqr_c(mm, m, md);
    E::dbl(t, sx);
    E::sub(x, mm, t, F::BIAS4_29);
    E::carry(x);
    s.put(a, x);
    E::sub(t, sx, x, F::BIAS8_29);
    E::carry(t);
    s.put(HT_3, t);
  }
  {
    T t1, t2, r;
    {
      const T m = s.get(HT_2), d = s.get(HT_3);
      E::template mul_c<true>(t1, m, d, md);
    }
    {
      const T y1 = s.get(a + 1), w = s.get(HT_1);
      E::template mul_c<false>(t2, y1, w, md);
    }
    E::sub(r, t1, t2, F::BIAS2_28);     // M (S - X3) - Y1 W, as mul_sub_c
    E::carry(r);
    s.put(a + 1, r);
  }
  {
    T r;
    {
      const T v = s.get(HT_0), zz = s.get(a + 2);
      E::template mul_c<false>(r, v, zz, md);
    }
    s.put(a + 2, r);
    {
      const T w = s.get(HT_1), zzz = s.get(a + 3);
      E::template mul_c<false>(r, w, zzz, md);
    }
    s.put(a + 3, r);
  }
}

// xyzz_add: the point at a += the point at b, every case
template <class E>
MSM_HD void h2c_slot_add(const H2cMem& s, int a, int b, const typename E::Md& md) {
  using T = typename E::T;
  using F = typename E::Fld;
  if (h2c_slot_is_inf<E>(s, b)) return;
  if (h2c_slot_is_inf<E>(s, a)) {
    h2c_slot_copy(s, a, b);
    return;
  }
  bool same_x;
  {
    T u1, u2, P, PP;
    {
      const T x1 = s.get(a), zz2 = s.get(b + 2);
      E::template mul_c<false>(u1, x1, zz2, md);
    }
    s.put(HT_0, u1);
    {
      const T x2 = s.get(b), zz1 = s.get(a + 2);
      E::template mul_c<false>(u2, x2, zz1, md);
    }
    E::sub(P, u2, u1, F::BIAS2_28);
    E::prep(P);
    s.put(HT_1, P);
    E::sqr_c(PP, P, md);
    s.put(HT_2, PP);
    same_x = E::is_zero_M(PP);
  }
  {
    T s1, s2, R;
    {
      const T y1 = s.get(a + 1), zzz2 = s.get(b + 3);
      E::template mul_c<false>(s1, y1, zzz2, md);
    }
    s.put(HT_3, s1);
    {
      const T y2 = s.get(b + 1), zzz1 = s.get(a + 3);
      E::template mul_c<false>(s2, y2, zzz1, md);
    }
    E::sub(R, s2, s1, F::BIAS2_28);
    if (same_x) {
      T r2;
      E::sqr(r2, R, md);
      if (E::is_zero_M(r2)) {
        h2c_slot_dbl<E>(s, a, md);
      } else {
        E::zero(r2);
#pragma unroll 1
        for (int k = 0; k < 4; k++) s.put(a + k, r2);
      }
      return;
    }
    E::carry(R);
    s.put(HT_4, R);
  }
  {
    // add_tail
    T ppp, q, r2, t, x3;
    {
      const T P = s.get(HT_1), PP = s.get(HT_2);
      E::template mul_c<false>(ppp, P, PP, md);
      s.put(HT_5, ppp);
      const T u1 = s.get(HT_0);
      E::template mul_c<false>(q, u1, PP, md);
    }
    {
      const T R = s.get(HT_4);
      E::sqr_c(r2, R, md);
    }
    E::dbl(t, q);
    E::add(t, t, ppp);
    E::sub(x3, r2, t, F::BIAS8_30);
    E::carry(x3);
    s.put(a, x3);
    E::sub(t, q, x3, F::BIAS16_29);
    E::carry(t);
    s.put(HT_6, t);
  }
  {
    T t1, t2, r;
    {
      const T R = s.get(HT_4), d = s.get(HT_6);
      E::template mul_c<true>(t1, R, d, md);
    }
    {
      const T s1 = s.get(HT_3), ppp = s.get(HT_5);
      E::template mul_c<false>(t2, s1, ppp, md);
    }
    E::sub(r, t1, t2, F::BIAS2_28);
    E::carry(r);
    s.put(a + 1, r);
  }
  {
    T t, r;
    {
      const T zz1 = s.get(a + 2), zz2 = s.get(b + 2);
      E::template mul_c<false>(t, zz1, zz2, md);
    }
    {
      const T PP = s.get(HT_2);
      E::template mul_c<false>(r, t, PP, md);
    }
    s.put(a + 2, r);
    {
      const T zzz1 = s.get(a + 3), zzz2 = s.get(b + 3);
      E::template mul_c<false>(t, zzz1, zzz2, md);
    }
    {
      const T ppp = s.get(HT_5);
      E::template mul_c<false>(r, t, ppp, md);
    }
    s.put(a + 3, r);
  }
}

// -P (y through a product with one, so that it is class M again) and psi(P) on the point at a, a coordinate at a time: conj
// commutes with the quotients, so psi(X, Y, ZZ, ZZZ) = (conj X PSI_X, conj Y PSI_Y, conj ZZ, conj ZZZ)
template <class E>
MSM_HD void h2c_slot_neg(const H2cMem& s, int a, const typename E::Md& md) {
  typename E::T y = s.get(a + 1), ny, one;
  E::set_one(one);
  E::neg(ny, y, E::Fld::BIAS16_29);
  E::mul(y, ny, one, md);
  s.put(a + 1, y);
}

template <class E>
MSM_HD void h2c_slot_psi(const H2cMem& s, int a, const typename E::Md& md) {
  using Sub = typename CheckConsts<E>::Sub;
  using F = typename E::Fld;
#pragma unroll 1
  for (int k = 0; k < 2; k++) {
    Fe2 c = s.get(a + k), kc, r;
    fe_neg(kc.c1, c.c1, F::BIAS16_29);
    c.c1 = kc.c1;
    if (k == 0) {
      fe_set(kc.c0, Sub::PSI_X0);
      fe_set(kc.c1, Sub::PSI_X1);
    } else {
      fe_set(kc.c0, Sub::PSI_Y0);
      fe_set(kc.c1, Sub::PSI_Y1);
    }
    E::mul(r, c, kc, md);
    s.put(a + k, r);
  }
#pragma unroll 1
  for (int k = 2; k < 4; k++) {
    Fe2 c = s.get(a + k);
    Fe n, one;
    fe_set(one, F::ONE);
    fe_neg(n, c.c1, F::BIAS2_28);
    fe_mul<F>(c.c1, n, one, md);
    s.put(a + k, c);
  }
}

// The steps of the pair sum and of Budroni-Pintore's chain for z < 0, |z| = 0xd201000000010000, written at compile time.
enum { HO_DBL = 0, HO_ADD, HO_COPY, HO_NEG, HO_PSI };
struct H2cG2Prog {
  uint8_t op[192], a[192], b[192];
  int n;
  constexpr void emit(int o, int x, int y) {
    op[n] = (uint8_t)o;
    a[n] = (uint8_t)x;
    b[n] = (uint8_t)y;
    n++;
  }
  constexpr void walk(int base) {   // ACC = [|z|] base, ACC == base on entry; then ACC = -ACC: [z] base
    const uint64_t z = 0xd201000000010000ull;
    for (int bit = 62; bit >= 0; bit--) {
      emit(HO_DBL, HP_ACC, 0);
      if ((z >> bit) & 1) emit(HO_ADD, HP_ACC, base);
    }
    emit(HO_NEG, HP_ACC, 0);
  }
  constexpr H2cG2Prog() : op{}, a{}, b{}, n(0) {
    emit(HO_ADD, HP_ACC, HP_B);      // step 0: the pair sum; a single point starts at step 1
    emit(HO_COPY, HP_Q, HP_ACC);
    walk(HP_Q);                      // z Q
    emit(HO_COPY, HP_T1, HP_ACC);
    emit(HO_COPY, HP_B, HP_Q);
    emit(HO_PSI, HP_B, 0);
    emit(HO_ADD, HP_ACC, HP_B);      // z Q + psi(Q)
    emit(HO_COPY, HP_T2, HP_ACC);
    walk(HP_T2);                     // z^2 Q + z psi(Q)
    emit(HO_COPY, HP_B, HP_T1);
    emit(HO_NEG, HP_B, 0);
    emit(HO_ADD, HP_ACC, HP_B);      // - z Q
    emit(HO_COPY, HP_B, HP_Q);
    emit(HO_NEG, HP_B, 0);
    emit(HO_ADD, HP_ACC, HP_B);      // - Q
    emit(HO_COPY, HP_B, HP_Q);
    emit(HO_PSI, HP_B, 0);
    emit(HO_NEG, HP_B, 0);
    emit(HO_ADD, HP_ACC, HP_B);      // - psi(Q)
    emit(HO_COPY, HP_B, HP_Q);
    emit(HO_DBL, HP_B, 0);
    emit(HO_PSI, HP_B, 0);
    emit(HO_PSI, HP_B, 0);
    emit(HO_ADD, HP_ACC, HP_B);      // + psi^2(2Q)
  }
};
struct H2cG2Steps {
  static constexpr H2cG2Prog P{};
};

// HP_ACC (and, with pairs, HP_B) -> HP_ACC = h_eff (ACC [+ B])
template <class E>
MSM_HD void h2c_clear_slots(const H2cMem& s, bool pairs, const typename E::Md& md) {
  static_assert(CheckConsts<E>::Sub::U_NEG && CheckConsts<E>::Sub::U[1] == 0xd2010000u && CheckConsts<E>::Sub::U[0] == 0x00010000u, "the steps are written for this z");
#pragma unroll 1
  for (int i = pairs ? 0 : 1; i < H2cG2Steps::P.n; i++) {
    const int op = H2cG2Steps::P.op[i], a = H2cG2Steps::P.a[i], b = H2cG2Steps::P.b[i];
    if (op == HO_DBL) h2c_slot_dbl<E>(s, a, md);
    else if (op == HO_ADD) h2c_slot_add<E>(s, a, b, md);
    else if (op == HO_COPY) h2c_slot_copy(s, a, b);
    else if (op == HO_NEG) h2c_slot_neg<E>(s, a, md);
    else h2c_slot_psi<E>(s, a, md);
  }
}

// ---- one entry for both fields: over Fp in registers, over Fp2 through the lane's slots -----------------------------------------------
// out = map(u).  ws: the lane's first slot (Fp2 only), slots `pitch` apart
template <class E>
MSM_HD void h2c_map_at(XyzzT<typename E::T>* out, const typename E::T& u, void* ws, size_t pitch, const typename E::Md& md) {
  if constexpr (E::WORDS == 12) {
    XyzzT<typename E::T> o;
    h2c_map<E>(o, u, md);
    *out = o;
  } else {
    const H2cMem s{(Fe2*)ws, pitch};
    s.put(HS_U, u);
    h2c_sswu_slots<E>(s, md);
    h2c_iso_slots<E>(out, s, md);
  }
}
// out = h_eff (a [+ b]); b may be null
template <class E>
MSM_HD void h2c_clear_at(XyzzT<typename E::T>* out, const XyzzT<typename E::T>* a, const XyzzT<typename E::T>* b, void* ws, size_t pitch,
                         const typename E::Md& md) {
  if constexpr (E::WORDS == 12) {
    XyzzT<typename E::T> acc = *a;
    if (b) {
      const XyzzT<typename E::T> q = *b;
      xyzz_add<E>(acc, q, md);
    }
    h2c_clear<E>(acc, (XyzzT<typename E::T>*)ws, md);
    *out = acc;
  } else {
    const H2cMem s{(Fe2*)ws, pitch};
    for (int k = 0; k < 4; k++) s.put(HP_ACC + k, ((const Fe2*)a)[k]);
    if (b)
      for (int k = 0; k < 4; k++) s.put(HP_B + k, ((const Fe2*)b)[k]);
    h2c_clear_slots<E>(s, b != nullptr, md);
    for (int k = 0; k < 4; k++) ((Fe2*)out)[k] = s.get(HP_ACC + k);
  }
}
// bytes of work memory a lane of the map / of the clearing kernel owns
template <class E>
constexpr size_t h2c_map_ws_bytes() { return E::WORDS == 12 ? 0 : (size_t)H2C_MAP_SLOTS * sizeof(Fe2); }
template <class E>
constexpr size_t h2c_clear_ws_bytes() { return E::WORDS == 12 ? sizeof(XyzzT<typename E::T>) : (size_t)H2C_CLEAR_SLOTS * sizeof(Fe2); }

// ---- offsets ---------------------------------------------------------------------------------------------------------------------
// The n + 1 offsets of a host-pointer call: non-decreasing and inside the buffer.  Returns nullptr, or what is wrong.
inline const char* h2c_check_offsets(const uint64_t* off, size_t n, size_t data_bytes) {
  if (!off) return "null offsets";
  for (size_t i = 0; i < n; i++)
    if (off[i] > off[i + 1]) return "the offsets decrease";
  if (off[n] > data_bytes) return "the last offset lies outside the message buffer";
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] - off[i] >= (1ull << 28)) return "a message of 2^28 bytes or more";
  return nullptr;
}

// create-time host code: DST (or the hash of an oversize one) || its length, and the state after 64 zero bytes.  prime: 256 bytes.
inline void h2c_make_dst(uint8_t* prime, uint32_t& prime_len, uint32_t (&z_pad)[8], const uint8_t* dst, size_t dst_len) {
  if (dst_len > H2C_MAX_DST) {
    static const char tag[] = "H2C-OVERSIZE-DST-";
    uint8_t* buf = new uint8_t[17 + dst_len];
    for (int i = 0; i < 17; i++) buf[i] = (uint8_t)tag[i];
    for (size_t i = 0; i < dst_len; i++) buf[17 + i] = dst[i];
    uint32_t h[8];
    h2c_sha256(h, buf, (uint32_t)(17 + dst_len));
    delete[] buf;
    for (int i = 0; i < 32; i++) prime[i] = (uint8_t)(h[i >> 2] >> (24 - 8 * (i & 3)));
    dst_len = 32;
  } else {
    for (size_t i = 0; i < dst_len; i++) prime[i] = dst[i];
  }
  prime[dst_len] = (uint8_t)dst_len;
  prime_len = (uint32_t)dst_len + 1;
  uint32_t w[16] = {0};
  h2c_sha_iv(z_pad);
  h2c_sha_block(z_pad, w);
}

#if defined(__HIPCC__)
struct H2cRun {
  H2cDst dst;
  const uint8_t* data;
  const uint64_t* offsets;
  uint64_t data_bytes;
};

// one lane per message: elems images of 12 words at out[i * elems * 12].  A bad offset cannot read outside the buffer: every
// message is clamped to it.
template <class F>
__global__ void __launch_bounds__(H2C_LANES) k_h2c_expand(const H2cRun p, uint32_t n, uint32_t elems, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * H2C_LANES + threadIdx.x;
  if (i >= n) return;
  const Modulus<F> md;
  uint64_t lo = p.offsets[i], hi = p.offsets[i + 1];
  lo = lo < p.data_bytes ? lo : p.data_bytes;
  hi = hi < lo ? lo : (hi < p.data_bytes ? hi : p.data_bytes);
  const uint64_t len = hi - lo < (1ull << 28) ? hi - lo : (1ull << 28) - 1;
  h2c_expand<F>(out + (size_t)i * elems * 12, p.data + lo, (uint32_t)len, elems, p.dst, md);
}

// one lane per u (E::WORDS words each, packed) -> XYZZ.  ws (Fp2 only): H2C_MAP_SLOTS * n elements, slot-major
template <class E>
__global__ void __launch_bounds__(H2C_LANES) k_h2c_map(const uint32_t* __restrict__ u, uint32_t n, uint8_t* ws, XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * H2C_LANES + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  constexpr int W = E::WORDS;
  uint32_t w[W];
#pragma unroll
  for (int k = 0; k < W; k++) w[k] = u[(size_t)i * W + k];
  typename E::T x;
  E::from_abi(x, w, md);
  h2c_map_at<E>(&out[i].p, x, ws + (size_t)i * sizeof(typename E::T), n, md);
}

// one lane per output: in[i] (pairs == 0) or in[2i] + in[2i + 1], times h_eff.  ws: h2c_clear_ws_bytes * n, slot-major
template <class E>
__global__ void __launch_bounds__(H2C_LANES) k_h2c_clear(const XyzzDevT<typename E::T>* __restrict__ in, uint32_t n, uint32_t pairs, uint8_t* ws,
                                                         XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * H2C_LANES + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  const XyzzDevT<typename E::T>* a = in + (pairs ? 2 * (size_t)i : i);
  constexpr size_t unit = E::WORDS == 12 ? sizeof(XyzzT<typename E::T>) : sizeof(typename E::T);   // what a slot holds
  h2c_clear_at<E>(&out[i].p, &a->p, pairs ? &a[1].p : nullptr, ws + (size_t)i * unit, n, md);
}
#endif

}  // namespace msm
