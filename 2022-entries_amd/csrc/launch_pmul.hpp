// launch_pmul.hpp -- host-callable launchers of the point-multiplication kernels (point_mul.hpp).  Declared here, defined and
// instantiated for the four curves in kernels_pmul.hip; the only other unit that includes it is the engine (msm_pmul.hpp).
#pragma once
#include "launch.hpp"
#include "point_mul.hpp"   // PmNaf

namespace msm {

template <class E>
struct LaunchPmul {
  using El = typename E::T;
  // (e + 1) P_i for e < entries at out[e * n + i], XYZZ, from Affine images `stride` bytes apart (device memory)
  static hipError_t table(const uint8_t* d_points, size_t stride, uint32_t n, uint32_t entries, XyzzDevT<El>* out, hipStream_t st);
  // out[i] = scalar_i * P_i through the normalised table (2^(w-1) * n records, entry-major)
  static hipError_t mul(const AffineDevT<El>* table, const uint32_t* scalars, uint32_t n, uint32_t w, bool from_mont, XyzzDevT<El>* out, hipStream_t st);
  // out[i] = k * P_i, k in non-adjacent form
  static hipError_t mul_uniform(const uint8_t* d_points, size_t stride, uint32_t n, const PmNaf& naf, XyzzDevT<El>* out, hipStream_t st);
};

extern template struct LaunchPmul<Bls12_377_G1::E>;
extern template struct LaunchPmul<Bls12_381_G1::E>;
extern template struct LaunchPmul<Bls12_377_G2::E>;
extern template struct LaunchPmul<Bls12_381_G2::E>;

}  // namespace msm
