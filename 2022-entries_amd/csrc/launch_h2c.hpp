// launch_h2c.hpp -- host-callable launchers of the three kernels of h2c.hpp.  Declared here, defined and instantiated for the two
// groups of BLS12-381 in kernels_h2c.hip; the only other unit that includes it is the engine (msm_h2c.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include "h2c.hpp"

namespace msm {

template <class E>
struct LaunchH2c {
  using El = typename E::T;
  // one lane per message / u / output, H2C_LANES lanes per block
  static hipError_t expand(const H2cRun& p, uint32_t n, uint32_t elems, uint32_t* out, hipStream_t st);
  static hipError_t map(const uint32_t* u, uint32_t n, uint8_t* ws, XyzzDevT<El>* out, hipStream_t st);
  static hipError_t clear(const XyzzDevT<El>* in, uint32_t n, bool pairs, uint8_t* ws, XyzzDevT<El>* out, hipStream_t st);
};

extern template struct LaunchH2c<Bls12_381_G1::E>;
extern template struct LaunchH2c<Bls12_381_G2::E>;

}  // namespace msm
