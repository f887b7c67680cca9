// launch_expr.hpp -- the host-callable launcher of the kernel of expr.hpp.  Declared here, defined and instantiated for the two scalar
// fields in kernels_expr.hip; the only other unit that includes it is the engine (msm_expr.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "expr.hpp"

namespace msm {

template <class FR>
struct LaunchExpr {
  // one lane per row, blocks of one wave, `slots` slots of dynamic LDS per lane
  static hipError_t rows(const ExprRun& p, uint32_t slots, hipStream_t st);
};

extern template struct LaunchExpr<Bls12_377_Fr29>;
extern template struct LaunchExpr<Bls12_381_Fr29>;

}  // namespace msm
