// launch_quot.hpp -- host-callable launchers of the kernels of quotient.hpp.  Declared here, defined and instantiated for the two
// scalar fields in kernels_quot.hip; the only other unit that includes it is the engine (msm_quot.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "quotient.hpp"

namespace msm {

template <class FR>
struct LaunchQuot {
  // one lane per row of the domain
  static hipError_t xm1(const QuotXm1& p, hipStream_t st);
  static hipError_t rows(const QuotRows& p, hipStream_t st);
  // one lane per element, p.n >= 1
  static hipError_t lincomb(const LinComb& p, hipStream_t st);
};

extern template struct LaunchQuot<Bls12_377_Fr29>;
extern template struct LaunchQuot<Bls12_381_Fr29>;

}  // namespace msm
