// launch_mle.hpp -- host-callable launchers of the kernels of mle.hpp.  Declared here, defined and instantiated for the two scalar
// fields in kernels_mle.hip; the only other unit that includes it is the engine (msm_mle.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "mle.hpp"

namespace msm {

template <class FR>
struct LaunchMle {
  // one block per tile of 2^tile_log elements
  static hipError_t fix(const MleFix& p, hipStream_t st);
  // one lane per output
  static hipError_t eq(const MleEq& p, hipStream_t st);
  // one block per 2^tile_log pairs; D: the largest factor count, 1 .. MLE_MAX_FACTORS
  static hipError_t round(const MleRound& p, uint32_t D, hipStream_t st);
  // one block per 2^tile_log rows
  static hipError_t sum(const MleSum& p, hipStream_t st);
};

extern template struct LaunchMle<Bls12_377_Fr29>;
extern template struct LaunchMle<Bls12_381_Fr29>;

}  // namespace msm
