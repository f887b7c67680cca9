// launch_ntt.hpp -- host-callable launchers of the transform kernels (ntt.hpp).  Declared here, defined and instantiated for the two
// scalar fields in kernels_ntt.hip; the only other unit that includes it is the engine (msm_ntt.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "ntt.hpp"

namespace msm {

template <class FR>
struct LaunchNtt {
  // one pass over `batch` vectors of 2^k elements (ps.src / ps.dst: the first vector)
  static hipError_t pass(const NttPass& ps, uint32_t batch, hipStream_t st);
  // out[i] = a[i] * b[i] in the ABI form of `normal`
  static hipError_t mul_vec(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, bool normal, hipStream_t st);
  // out[i] = base^i for i < n, canonical
  static hipError_t table(const Fr& base, uint32_t n, Fr* out, hipStream_t st);
};

extern template struct LaunchNtt<Bls12_377_Fr29>;
extern template struct LaunchNtt<Bls12_381_Fr29>;

}  // namespace msm
