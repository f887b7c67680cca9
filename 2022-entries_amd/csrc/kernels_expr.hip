// kernels_expr.hip -- the kernel of expr.hpp (a compiled expression, one lane per row) for the two scalar fields, in a unit of its own.
#include "launch_expr.hpp"

namespace msm {

template <class FR>
hipError_t LaunchExpr<FR>::rows(const ExprRun& p, uint32_t slots, hipStream_t st) {
  if (p.len == 0) return hipSuccess;
  if (slots > EXPR_MAX_SLOTS) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(((uint64_t)p.len + EXPR_LANES - 1) / EXPR_LANES);
  hipLaunchKernelGGL((k_expr_rows<FR>), dim3(grid), dim3(EXPR_LANES), expr_lds_bytes(slots), st, p);
  return hipGetLastError();
}

template struct LaunchExpr<Bls12_377_Fr29>;
template struct LaunchExpr<Bls12_381_Fr29>;

}  // namespace msm
