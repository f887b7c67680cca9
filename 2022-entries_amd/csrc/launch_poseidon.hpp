// launch_poseidon.hpp -- host-callable launcher of the kernel of poseidon.hpp.  Declared here, defined and instantiated for the two
// scalar fields in kernels_poseidon.hip; the only other unit that includes it is the engine (msm_poseidon.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "poseidon.hpp"

namespace msm {

template <class FR>
struct LaunchPoseidon {
  // one lane per sponge, POS_LANES lanes per block, pos_lds_bytes(t) bytes of LDS
  static hipError_t hash(const PosRun& p, hipStream_t st);
};

extern template struct LaunchPoseidon<Bls12_377_Fr29>;
extern template struct LaunchPoseidon<Bls12_381_Fr29>;

}  // namespace msm
