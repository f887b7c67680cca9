// group_fft.hpp -- radix-2 transforms of vectors of curve points over a domain of the scalar field (arkworks'
// Radix2EvaluationDomain::fft / ifft / coset_fft / coset_ifft on G1Projective / G2Projective coefficients): out[i] = sum_j w^(i j) P_j,
// the products scalar multiples.
//
// Reference behaviour: ARK poly/src/domain/mod.rs:99-170 (the four calls, distribute_powers), poly/src/domain/mod.rs DomainCoeff;
// the butterfly multiplier is the field element's canonical integer (ec/src/models/short_weierstrass/group.rs MulAssign<Fr>).
//
// Decomposition.  k = log2 n stages of n / 2 butterflies, decimation in time in Stockham's self-sorting layout: after stage s the
// vector holds the 2^(k-s-1) sub-transforms of size 2^(s+1), bin i of the sub-transform over the inputs = c (mod 2^(k-s-1)) at
// [c + i 2^(k-s-1)].  Butterfly b < n / 2 of stage s, with h = 2^(k-s-1), i = b / h, c = b mod h:
//
//     A = x[c + 2 h i],  B = x[c + 2 h i + h],  T = w_n^(h i) * B,      y[b] = A + T,  y[b + n / 2] = A - T.
//
// Stage 0 reads the input in natural order (A = x[b], B = x[b + n / 2]) and all its twiddles are 1: it multiplies nothing.  The last
// stage writes the output in natural order.  The permutation an in-place transform makes up front as a bit reversal is spread over
// the load index maps gf_index_a / gf_index_b, and every stage WRITES two contiguous runs -- which is what lets the output
// normalisation of fixed_base.hpp, which writes consecutive images, put the results back into affine form as it stands.
//
// One lane per butterfly.  The twiddle LO[e mod 2^14] * HI[e >> 14] comes out of the domain's tables (the inverse root's for the
// inverse kinds) and is brought to the canonical integer in registers (one product by COUT_NORM, one conditional subtraction); its
// signed digits drive pm_windowed_mul over B's table, built as k_pm_table builds it and normalised by Launch<E>::pre_normalize; the
// two xyzz_madd of the affine A onto T and -T follow in the same kernel.  T never goes to memory.
// The coset kinds and 1/n are one more multiplication per point, by g^j, n^-1 or g^-j n^-1 as ONE factor, its own launch
// (k_gf_scale) before the first stage (coset forward) or after the last (the inverse kinds).
//
// No curve test and no subgroup test.  A record on no curve gives an unspecified result, but every memory access is a function of
// the lane index, n and the twiddle digits alone.  Every per-element step is an MSM_HD function (host_test_api.cpp, ht_gf_*).
#pragma once
#include <cstdio>
#include <type_traits>

#include "ntt.hpp"
#include "point_mul.hpp"

namespace msm {

template <class E>
using GfFr = std::conditional_t<CheckConsts<E>::R_BITS == 253, Bls12_377_Fr29, Bls12_381_Fr29>;

// ---- index maps --------------------------------------------------------------------------------------------------------------
// butterfly b < 2^(k-1) of stage s < k
MSM_HD uint32_t gf_index_a(uint32_t k, uint32_t s, uint32_t b) {
  const uint32_t hl = k - s - 1;
  return ((b >> hl) << (hl + 1)) | (b & ((1u << hl) - 1));
}
MSM_HD uint32_t gf_index_b(uint32_t k, uint32_t s, uint32_t b) { return gf_index_a(k, s, b) + (1u << (k - s - 1)); }
// the exponent of w_n in the butterfly's twiddle: h i, below n / 2; 0 for every butterfly of stage 0
MSM_HD uint32_t gf_twiddle_exp(uint32_t k, uint32_t s, uint32_t b) {
  const uint32_t hl = k - s - 1;
  return (b >> hl) << hl;
}

// ---- multipliers -------------------------------------------------------------------------------------------------------------
// root^e from the two-level tables as the canonical integer below r, 8 words
template <class FR>
MSM_HD void gf_twiddle_words(uint32_t (&s)[8], const NttTable& t, uint32_t k, uint32_t e) {
  const uint32_t h = ntt_lo_log(k);
  Fr x = t.lo[e & ((1u << h) - 1)];
  const Fr f = t.hi[e >> h];
  fr_mul<FR>(x, x, f);   // class M
  fr_to_abi<FR>(s, x, true);
}

// the factor of point j outside the stages: g^j (coset forward), scale = 1/n (inverse), g^-j / n (coset inverse; the tables are those
// of g^-1), one canonical integer
struct GfScale {
  NttTable g;
  Fr scale;   // 1/n, a reduced Montgomery element like the tables' entries
  uint32_t has_g, has_scale;
};
template <class FR>
MSM_HD void gf_scale_words(uint32_t (&s)[8], const GfScale& sc, uint32_t k, uint32_t j) {
  Fr x;
  if (sc.has_g) {
    const uint32_t h = ntt_lo_log(k);
    x = sc.g.lo[j & ((1u << h) - 1)];
    const Fr f = sc.g.hi[j >> h];
    fr_mul<FR>(x, x, f);
    if (sc.has_scale) fr_mul<FR>(x, x, sc.scale);
  } else {
    x = sc.scale;
  }
  fr_to_abi<FR>(s, x, true);
}

// ---- points ------------------------------------------------------------------------------------------------------------------
// a vector of Affine images `stride` bytes apart of which the first in_len exist; the rest stand for the point at infinity and their
// bytes are never read
struct GfVec {
  const uint8_t* p;
  size_t stride;
  uint32_t in_len;
};

// image idx -> words and flag (1: infinity, by the flag byte or by idx >= in_len)
template <class E>
MSM_HD uint8_t gf_read(uint32_t (&rec)[2 * E::WORDS], const GfVec& v, uint32_t idx) {
  constexpr int W = E::WORDS;
  if (idx >= v.in_len) {
#pragma unroll
    for (int q = 0; q < 2 * W; q++) rec[q] = 0;
    return 1;
  }
  const uint8_t* p = v.p + (size_t)idx * v.stride;
#pragma unroll
  for (int q = 0; q < 2 * W; q++) rec[q] = reinterpret_cast<const uint32_t*>(p)[q];
  return p[8 * W] ? 1 : 0;
}

// returns true for the point at infinity (P is then zeros)
template <class E>
MSM_HD bool gf_load(AffineT<typename E::T>& P, const GfVec& v, uint32_t idx, const typename E::Md& md) {
  uint32_t rec[2 * E::WORDS];
  if (gf_read<E>(rec, v, idx)) {
    E::zero(P.x);
    E::zero(P.y);
    return true;
  }
  pm_load_point<E>(P, rec, md);
  return false;
}

// *sum = T + A, *diff = -T + A: two mixed additions, the first result stored before the second begins (an Fp2 point is 112 registers).
// -T takes T's y through one product by 1 (class M, which the BIAS2_28 negation asks for: a stored y is only below 16p) and negates
// it as xyzz_from_affine negates an affine y.  T is used up.
template <class E>
MSM_HD void gf_butterfly(XyzzT<typename E::T>* sum, XyzzT<typename E::T>* diff, XyzzT<typename E::T>& T, const AffineT<typename E::T>& A, bool a_inf,
                         const typename E::Md& md) {
  using El = typename E::T;
  {
    XyzzT<El> acc = T;
    if (!a_inf) xyzz_madd<E>(acc, A, false, false, md);
    *sum = acc;
  }
  El one, ym;
  E::set_one(one);
  E::mul(ym, T.y, one, md);
  E::neg(T.y, ym, E::Fld::BIAS2_28);   // (0, 2p], limbs < 2^29
  E::carry(T.y);                       // (T at infinity: zz = 0 stays, and the addition below starts from A)
  if (!a_inf) xyzz_madd<E>(T, A, false, false, md);
  *diff = T;
}

// a stage-0 butterfly: T = B itself
template <class E>
MSM_HD void gf_butterfly_first(XyzzT<typename E::T>* sum, XyzzT<typename E::T>* diff, const GfVec& v, uint32_t k, uint32_t b, const typename E::Md& md) {
  using El = typename E::T;
  AffineT<El> A, B;
  XyzzT<El> T;
  if (gf_load<E>(B, v, gf_index_b(k, 0, b), md))
    xyzz_set_inf<E>(T);
  else
    xyzz_from_affine<E>(T, B, false);
  const bool a_inf = gf_load<E>(A, v, gf_index_a(k, 0, b), md);
  gf_butterfly<E>(sum, diff, T, A, a_inf, md);
}

// a butterfly of stage s >= 1 through B's table (records table[e * pitch]); `top` as pm_windowed_mul takes it
template <class E>
MSM_HD void gf_butterfly_mul(XyzzT<typename E::T>* sum, XyzzT<typename E::T>* diff, const GfVec& v, const AffineDevT<typename E::T>* __restrict__ table,
                             size_t pitch, const uint32_t (&tw)[8], uint32_t w, uint32_t top, uint32_t k, uint32_t s, uint32_t b, const typename E::Md& md) {
  using El = typename E::T;
  XyzzT<El> T;
  pm_windowed_mul<E>(T, table, pitch, tw, w, top, md);
  AffineT<El> A;
  const bool a_inf = gf_load<E>(A, v, gf_index_a(k, s, b), md);
  gf_butterfly<E>(sum, diff, T, A, a_inf, md);
}

// table of point idx, as pm_table lays it out
template <class E>
MSM_HD void gf_table(XyzzT<typename E::T>* out, size_t pitch, const GfVec& v, uint32_t idx, uint32_t entries, const typename E::Md& md) {
  uint32_t rec[2 * E::WORDS];
  const uint8_t flag = gf_read<E>(rec, v, idx);
  pm_table<E>(out, pitch, rec, flag, entries, md);
}

// ---- what a call can be refused for, decided from plain values (the engine passes its handles' fields; the host build the test's) --
// returns nullptr or the message
struct GfCall {
  int ctx_curve, ctx_sharded, ctx_device, dom_curve, dom_device;
  uint32_t k;
  const void* out;
  size_t out_stride;
  const void* in;
  size_t in_len, stride;
  unsigned kind, flags;
  int has_offset, offset_is_zero;
  size_t work_limit;   // bytes the two work vectors may take
};
constexpr unsigned kGfProjective = 2u;   // the flag bit mul_points uses

inline size_t gf_coord_bytes(int curve) { return curve >= 2 ? 96 : 48; }                     // curve ids 0, 1: G1; 2, 3: G2
inline int gf_family(int curve) { return curve & 1; }                                        // 0: BLS12-377, 1: BLS12-381
inline size_t gf_image_bytes(int curve, unsigned flags) { return (flags & kGfProjective) ? 3 * gf_coord_bytes(curve) : 2 * gf_coord_bytes(curve) + 8; }
inline size_t gf_vec_bytes(int curve, uint32_t k) { return ((size_t)2 << k) * (2 * gf_coord_bytes(curve) + 8); }

// the part that needs no handle
inline const char* gf_check_kind(unsigned kind, unsigned flags, int has_offset, char* buf, size_t buflen) {
  if (kind > 3) {
    snprintf(buf, buflen, "unknown transform kind %u (0 forward, 1 inverse, 2 coset forward, 3 coset inverse)", kind);
    return buf;
  }
  if (flags & ~kGfProjective) {
    snprintf(buf, buflen, "unknown fft_points flag bits 0x%x (bit 1: Projective images)", flags);
    return buf;
  }
  if (has_offset && !(kind & 2)) return "an offset was given to a transform that is not over a coset";
  return nullptr;
}

inline const char* gf_check_call(const GfCall& c, char* buf, size_t buflen) {
  if (const char* m = gf_check_kind(c.kind, c.flags, c.has_offset, buf, buflen)) return m;
  if (c.has_offset && c.offset_is_zero) return "the coset offset is zero";
  if (c.ctx_sharded) return "fft_points is not available on a sharded context: use a single-device context";
  if (gf_family(c.ctx_curve) != gf_family(c.dom_curve)) return "the domain and the context are of different curve families";
  if (c.ctx_device != c.dom_device) {
    snprintf(buf, buflen, "the domain is on device %d and the context on device %d", c.dom_device, c.ctx_device);
    return buf;
  }
  const size_t n = (size_t)1 << c.k, cb = gf_coord_bytes(c.ctx_curve), img = gf_image_bytes(c.ctx_curve, c.flags);
  if (c.in_len > n) {
    snprintf(buf, buflen, "in_len %zu exceeds the domain size %zu", c.in_len, n);
    return buf;
  }
  if (c.stride % 4 || c.stride < 2 * cb + 1) {
    snprintf(buf, buflen, "stride %zu is not a 4-byte multiple >= %zu", c.stride, 2 * cb + 1);
    return buf;
  }
  if (c.out_stride % 4 || c.out_stride < img) {
    snprintf(buf, buflen, "out_stride %zu is not a 4-byte multiple >= the %zu-byte image", c.out_stride, img);
    return buf;
  }
  if (!c.out || (!c.in && c.in_len)) return "null input or output pointer";
  if (c.in && c.in_len) {
    const uintptr_t a = (uintptr_t)c.in, b = (uintptr_t)c.out;
    const uintptr_t rlen = (uintptr_t)((c.in_len - 1) * c.stride + 2 * cb + 1), wlen = (uintptr_t)((n - 1) * c.out_stride + img);
    const bool same = a == b && c.stride == c.out_stride;
    if (!same && a < b + wlen && b < a + rlen) return "input and output overlap in part (out == in with equal strides is allowed)";
  }
  if (gf_vec_bytes(c.ctx_curve, c.k) > c.work_limit) {
    snprintf(buf, buflen, "a transform of 2^%u points needs %zu bytes of work vectors, above the limit of %zu", c.k, gf_vec_bytes(c.ctx_curve, c.k), c.work_limit);
    return buf;
  }
  return nullptr;
}

#if defined(__HIPCC__)
// one lane per table point: lane i builds the table of B of butterfly b0 + i of stage s (stage_mode) or of point b0 + i
template <class E>
__global__ void __launch_bounds__(256) k_gf_table(GfVec v, uint32_t k, uint32_t s, uint32_t stage_mode, uint32_t b0, uint32_t cn, uint32_t entries,
                                                  XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cn) return;
  typename E::Md md;
  const uint32_t idx = stage_mode ? gf_index_b(k, s, b0 + i) : b0 + i;
  gf_table<E>(reinterpret_cast<XyzzT<typename E::T>*>(out + i), cn, v, idx, entries, md);
}

// the walk's start for a wave: the highest window any of its live lanes needs.  The same bit length and wave maximum as the block
// inside k_pm_mul (point_mul.hpp), which is left as it stands here; one shared helper for both walks is a follow-up.
__device__ __forceinline__ uint32_t gf_wave_top(const uint32_t (&s)[8], bool live, uint32_t w) {
  uint32_t bits = 0;
#pragma unroll
  for (int q = 0; q < 8; q++)
    if (s[q]) bits = 32u * q + 32u - (uint32_t)__clz((int)s[q]);
  if (!live) bits = 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)bits, off, 64);
    bits = o > bits ? o : bits;
  }
  return pm_top_window((uint32_t)__builtin_amdgcn_readfirstlane((int)bits), w);
}

// one lane per butterfly: lane i is butterfly b0 + i of stage s; out[i] = A + T, out[cn + i] = A - T.  MUL = false: stage 0.
// Lanes past cn keep the wave whole for the maximum and do nothing else.
template <class E, bool MUL>
__global__ void __launch_bounds__(256) k_gf_stage(GfVec v, const AffineDevT<typename E::T>* __restrict__ table, NttTable tw, uint32_t k, uint32_t s,
                                                  uint32_t b0, uint32_t cn, uint32_t w, XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < cn;
  typename E::Md md;
  XyzzT<typename E::T>* sum = reinterpret_cast<XyzzT<typename E::T>*>(out + i);
  XyzzT<typename E::T>* diff = reinterpret_cast<XyzzT<typename E::T>*>(out + (size_t)cn + i);
  if constexpr (MUL) {
    const uint32_t b = b0 + (live ? i : 0);
    uint32_t sc[8];
    gf_twiddle_words<GfFr<E>>(sc, tw, k, gf_twiddle_exp(k, s, b));
    const uint32_t top = gf_wave_top(sc, live, w);
    if (!live) return;
    gf_butterfly_mul<E>(sum, diff, v, table + i, cn, sc, w, top, k, s, b, md);
  } else {
    if (!live) return;
    gf_butterfly_first<E>(sum, diff, v, k, b0 + i, md);
  }
}

// one lane per point: out[i] = factor(j0 + i) * P through the table
template <class E>
__global__ void __launch_bounds__(256) k_gf_scale(const AffineDevT<typename E::T>* __restrict__ table, GfScale fs, uint32_t k, uint32_t j0, uint32_t cn,
                                                  uint32_t w, XyzzDevT<typename E::T>* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < cn;
  uint32_t sc[8];
  gf_scale_words<GfFr<E>>(sc, fs, k, j0 + (live ? i : 0));
  const uint32_t top = gf_wave_top(sc, live, w);
  if (!live) return;
  typename E::Md md;
  XyzzDevT<typename E::T> o;
  pm_windowed_mul<E>(o.p, table + i, cn, sc, w, top, md);
  out[i] = o;
}
#endif

}  // namespace msm
