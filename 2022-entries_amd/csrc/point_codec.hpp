// point_codec.hpp -- arkworks' COMPRESSED point records on the device: x plus two flag bits (48 B per G1 point, 96 B per G2
// point), what plain `serialize` / `deserialize` mean in the reference (ARK ec/src/models/short_weierstrass.rs:1120-1126, 1188-1201).
//
//   record   x as a little-endian normal-form integer (G2: c0 | c1), SWFlags in the top two bits of the last byte: bit 6 infinity,
//            bit 7 "y is the larger of y and -y" (ARK short_weierstrass.rs:1123; P1B nickray driver/algebra/serialize/src/flags.rs:107-134)
//   larger   sqrt.hpp, lex_largest_words
//   decode   y = sqrt(x^3 + b); of the two roots the larger iff bit 7 is set (get_point_from_x, short_weierstrass.rs:199-214)
//
// Decoding writes arkworks in-memory Affine images (Montgomery R = 2^384, flag byte, pad bytes zero, infinity as (0, 0, flag 1)) or
// uncompressed records (infinity as (0, 1) with bit 6, the record mi355_msm_point_to_serialized writes), and one status byte:
//
//   0  decoded, or flagged infinity -- the flag is authoritative, as everywhere in this ABI: a flagged record is valid whatever its x
//      bits hold
//   1  malformed: x (a component) is not below p after the flag bits are masked, or BOTH flag bits are set -- an encoding arkworks'
//      SWFlags::from_u8 refuses, and bit 7 carries meaning here, so this decoder refuses it too (the check of uncompressed records,
//      check_points.hpp, stays lenient as documented there)
//   2  no point has this x: x^3 + b has no square root
//
// The lowest applicable status wins.  A record that fails is written as an all-zero image with flag 0 -- a record check_bases reports
// as off the curve, never a silent infinity.  x = 0 without the flag is a real point on every curve here, (0, +-sqrt b).
// There is no subgroup test in the decode lane: the caller runs k_check_points over the decoded records when asked to.
//
// Encoding (k_compress_points) reads images or uncompressed records; status 1 for a non-canonical coordinate (the record is then all
// zeros), no curve test -- arkworks' `serialize` has none.  Of an uncompressed record's flag bits only bit 6 is read (check_points.hpp).
//
// Limb bounds: x and y enter as class M (from_plain / from_abi); x^3 + b is < 4p with limbs < 2^29 and goes through one product
// by one to become class M before the root (sqrt.hpp wants class M); -y is the BIAS2_28 negation of a class-M value, (0.5p, 2p] with
// limbs < 2^29, inside the contract of to_plain / to_abi (limbs < 2^30, value < 32p), which canonicalise it (y = 0: 2p -> 0).
#pragma once
#include "sqrt.hpp"

namespace msm {

enum CodecStatus : uint8_t { CODEC_OK = 0, CODEC_MALFORMED = 1, CODEC_NO_POINT = 2 };

// One compressed record (E::WORDS words) -> 2 * E::WORDS words of coordinates in the chosen form; `inf` = the record is a flagged
// infinity (the flag byte of an image; an uncompressed record carries bit 6 itself).
template <class E, bool OUT_SERIALIZED>
MSM_HD uint8_t decompress_point(uint32_t* out, uint8_t& inf, const uint32_t* rec, const typename E::Md& md) {
  using F = typename E::Fld;
  using T = typename E::T;
  constexpr int W = E::WORDS;
  uint32_t w[W];
#pragma unroll
  for (int k = 0; k < W; k++) w[k] = rec[k];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) out[k] = 0;
  const uint32_t top = w[W - 1];
  const bool want_larger = (top >> 31) != 0;
  w[W - 1] &= 0x3fffffffu;
  inf = 0;
  if ((top >> 30) == 3) return CODEC_MALFORMED;
  if ((top >> 30) & 1) {
    inf = 1;
    if (OUT_SERIALIZED) {
      out[W] = 1;
      out[2 * W - 1] = 0x40000000u;
    }
    return CODEC_OK;
  }
  bool canonical = true;
#pragma unroll
  for (int c = 0; c < W / 12; c++) canonical = canonical && check_words_below_p<F>(w + 12 * c);
  if (!canonical) return CODEC_MALFORMED;
  T x, y, ny;
  E::from_plain(x, w, md);
  {
    T x2, x3, b, rhs, one;
    E::sqr(x2, x, md);
    E::mul(x3, x2, x, md);
    check_load_b<typename CheckConsts<E>::Sub>(b);
    E::add(rhs, x3, b);          // < 4p, limbs < 2^29
    E::set_one(one);
    E::mul(rhs, rhs, one, md);   // the same residue, class M
    if (!el_sqrt(y, rhs, md, (E*)nullptr)) return CODEC_NO_POINT;
  }
  E::neg(ny, y, F::BIAS2_28);    // (0.5p, 2p], limbs < 2^29
  const bool flip = el_lex_largest<E>(y, md) != want_larger;
  E::cmov(y, ny, flip);
  if (OUT_SERIALIZED) {
#pragma unroll
    for (int k = 0; k < W; k++) out[k] = w[k];
    E::to_plain(out + W, y, md);
  } else {
    E::to_abi(out, x, md);
    E::to_abi(out + W, y, md);
  }
  return CODEC_OK;
}

// One point (2 * E::WORDS words of coordinates, and the flag byte of an image) -> E::WORDS words of the compressed record.
template <class E, bool IN_SERIALIZED>
MSM_HD uint8_t compress_point(uint32_t* out, uint8_t& inf, const uint32_t* rec, uint8_t flag, const typename E::Md& md) {
  using F = typename E::Fld;
  using T = typename E::T;
  constexpr int W = E::WORDS;
  uint32_t w[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) w[k] = rec[k];
#pragma unroll
  for (int k = 0; k < W; k++) out[k] = 0;
  if (IN_SERIALIZED) {
    flag = (w[2 * W - 1] >> 30) & 1;
    w[2 * W - 1] &= 0x3fffffffu;
  }
  inf = flag ? 1 : 0;
  if (flag) {
    out[W - 1] = 0x40000000u;
    return CODEC_OK;
  }
  bool canonical = true;
#pragma unroll
  for (int c = 0; c < 2 * W / 12; c++) canonical = canonical && check_words_below_p<F>(w + 12 * c);
  if (!canonical) return CODEC_MALFORMED;
  bool larger;
  if (IN_SERIALIZED) {
#pragma unroll
    for (int k = 0; k < W; k++) out[k] = w[k];
    larger = lex_largest_words(w + W, (E*)nullptr);
  } else {
    T x, y;
    E::from_abi(x, w, md);
    E::from_abi(y, w + W, md);
    E::to_plain(out, x, md);
    larger = el_lex_largest<E>(y, md);
  }
  if (larger) out[W - 1] |= 0x80000000u;
  return CODEC_OK;
}

#if defined(__HIPCC__)
// One lane per record, 256 per block.  `in`: n compressed records; `out`: images `stride` bytes apart (a 4-byte multiple, every word
// of the stride is written: coordinates, flag, zero pad) or uncompressed records.  Status bit 7 marks a flagged infinity for the
// engine's count, as k_check_points does.  Plain vector stores.
template <class E, bool OUT_SERIALIZED>
__global__ void __launch_bounds__(256) k_decompress_points(const uint8_t* __restrict__ in, uint32_t n, uint8_t* __restrict__ out, size_t stride,
                                                          uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  constexpr int W = E::WORDS;
  uint32_t o[2 * W];
  uint8_t inf;
  const uint8_t st = decompress_point<E, OUT_SERIALIZED>(o, inf, reinterpret_cast<const uint32_t*>(in + (size_t)i * 4 * W), md);
  const size_t rec = OUT_SERIALIZED ? (size_t)8 * W : stride;
  uint32_t* q = reinterpret_cast<uint32_t*>(out + (size_t)i * rec);
#pragma unroll
  for (int k = 0; k < 2 * W; k++) q[k] = o[k];
  if (!OUT_SERIALIZED) {
    q[2 * W] = inf;
    for (size_t k = 2 * W + 1; k < stride / 4; k++) q[k] = 0;
  }
  status[i] = (uint8_t)(st | (inf ? 0x80 : 0));
}

// One lane per point: images `stride` bytes apart or uncompressed records -> compressed records.
template <class E, bool IN_SERIALIZED>
__global__ void __launch_bounds__(256) k_compress_points(const uint8_t* __restrict__ in, size_t stride, uint32_t n, uint8_t* __restrict__ out,
                                                        uint8_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  typename E::Md md;
  constexpr int W = E::WORDS;
  const size_t rec = IN_SERIALIZED ? (size_t)8 * W : stride;
  const uint8_t* p = in + (size_t)i * rec;
  const uint8_t flag = IN_SERIALIZED ? (uint8_t)0 : p[8 * W];
  uint32_t o[W];
  uint8_t inf;
  const uint8_t st = compress_point<E, IN_SERIALIZED>(o, inf, reinterpret_cast<const uint32_t*>(p), flag, md);
  uint32_t* q = reinterpret_cast<uint32_t*>(out + (size_t)i * 4 * W);
#pragma unroll
  for (int k = 0; k < W; k++) q[k] = o[k];
  status[i] = (uint8_t)(st | (inf ? 0x80 : 0));
}
#endif

}  // namespace msm
