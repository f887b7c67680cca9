// launch_gfft.hpp -- host-callable launchers of the point-transform kernels (group_fft.hpp).  Declared here, defined and instantiated
// for the four curves in kernels_gfft.hip; the only other unit that includes it is the engine (msm_gfft.hpp).
#pragma once
#include "launch.hpp"
#include "group_fft.hpp"

namespace msm {

template <class E>
struct LaunchGfft {
  using El = typename E::T;
  // (e + 1) Q_i for e < entries at out[e * cn + i], XYZZ; Q_i: B of butterfly b0 + i of stage s (stage_mode), else point b0 + i
  static hipError_t table(const GfVec& v, uint32_t k, uint32_t s, bool stage_mode, uint32_t b0, uint32_t cn, uint32_t entries, XyzzDevT<El>* out, hipStream_t st);
  // butterflies [b0, b0 + cn) of stage s: out[i] = A + T, out[cn + i] = A - T; stage 0 takes no table
  static hipError_t stage(const GfVec& v, const AffineDevT<El>* table, const NttTable& tw, uint32_t k, uint32_t s, uint32_t b0, uint32_t cn, uint32_t w,
                          XyzzDevT<El>* out, hipStream_t st);
  // out[i] = factor(j0 + i) * P_(j0 + i) through the normalised table
  static hipError_t scale(const AffineDevT<El>* table, const GfScale& fs, uint32_t k, uint32_t j0, uint32_t cn, uint32_t w, XyzzDevT<El>* out, hipStream_t st);
};

extern template struct LaunchGfft<Bls12_377_G1::E>;
extern template struct LaunchGfft<Bls12_381_G1::E>;
extern template struct LaunchGfft<Bls12_377_G2::E>;
extern template struct LaunchGfft<Bls12_381_G2::E>;

}  // namespace msm
