// launch_pairing.hpp -- host-callable launchers of the three kernels of pairing.hpp.  Declared here, defined and instantiated for the two
// families in kernels_pairing.hip; the only other unit that includes it is the engine (msm_pairing.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "pairing.hpp"

namespace msm {

template <class E>
struct LaunchPairing {
  // one lane per item / product / group, PR_LANES lanes per block
  static hipError_t miller(const PrRun& p, uint64_t items, hipStream_t st);
  static hipError_t product(const PrRun& p, uint64_t lanes, hipStream_t st);
  static hipError_t final(const PrRun& p, uint64_t groups, hipStream_t st);
};

extern template struct LaunchPairing<Fp2El<Bls12_377_Fq, 5>>;
extern template struct LaunchPairing<Fp2El<Bls12_381_Fq, 1>>;

}  // namespace msm
