// launch_fixed.hpp -- host-callable launchers of the fixed-base kernels (fixed_base.hpp).  Declared here, defined and instantiated for
// the four curves in kernels_fixed.hip; the only other unit that includes it is the engine (msm_fixed.hpp).
#pragma once
#include "launch.hpp"

namespace msm {

template <class E>
struct LaunchFixed {
  using El = typename E::T;
  // 2^(w j) g, j < levels, from the caller's Affine image of g (device memory, flag byte at 8 * E::WORDS)
  static hipError_t level_bases(const uint8_t* d_img, uint32_t w, uint32_t levels, XyzzDevT<El>* out, hipStream_t st);
  // d * lbase[j] for every d < 2^w and j < levels, XYZZ, level-major
  static hipError_t table(const AffineDevT<El>* lbase, const uint8_t* lbase_inf, uint32_t w, uint32_t levels, XyzzDevT<El>* out, hipStream_t st);
  // out[i] = scalar_i * g through the table (levels << w records)
  static hipError_t mul(const AffineDevT<El>* table, const uint32_t* scalars, uint32_t n, uint32_t w, uint32_t levels, bool from_mont, XyzzDevT<El>* out,
                        hipStream_t st);
  // XYZZ results -> Affine / Projective images `out_stride` bytes apart; prefix: n elements of scratch
  static hipError_t normalize(const XyzzDevT<El>* in, uint32_t n, El* prefix, uint8_t* out, size_t out_stride, bool projective, hipStream_t st);
};

extern template struct LaunchFixed<Bls12_377_G1::E>;
extern template struct LaunchFixed<Bls12_381_G1::E>;
extern template struct LaunchFixed<Bls12_377_G2::E>;
extern template struct LaunchFixed<Bls12_381_G2::E>;

}  // namespace msm
