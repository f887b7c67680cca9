// kernels_mle.hip -- the kernels of mle.hpp (one pass of fix_variables, the eq table, a sumcheck round for every degree, the further
// sums of its partial rows) for the two scalar fields, in a unit of its own.
#include "launch_mle.hpp"

namespace msm {

template <class FR>
hipError_t LaunchMle<FR>::fix(const MleFix& p, hipStream_t st) {
  hipLaunchKernelGGL((k_mle_fix<FR>), dim3((unsigned)(p.n >> p.tile_log)), dim3(MLE_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchMle<FR>::eq(const MleEq& p, hipStream_t st) {
  hipLaunchKernelGGL((k_mle_eq<FR>), dim3((unsigned)((p.n + MLE_THREADS - 1) / MLE_THREADS)), dim3(MLE_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchMle<FR>::round(const MleRound& p, uint32_t D, hipStream_t st) {
  const dim3 grid((unsigned)mle_blocks(p.npts, p.tile_log)), block(MLE_THREADS);
  switch (D) {
    case 1: hipLaunchKernelGGL((k_mle_round<FR, 1>), grid, block, 0, st, p); break;
    case 2: hipLaunchKernelGGL((k_mle_round<FR, 2>), grid, block, 0, st, p); break;
    case 3: hipLaunchKernelGGL((k_mle_round<FR, 3>), grid, block, 0, st, p); break;
    case 4: hipLaunchKernelGGL((k_mle_round<FR, 4>), grid, block, 0, st, p); break;
    case 5: hipLaunchKernelGGL((k_mle_round<FR, 5>), grid, block, 0, st, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchMle<FR>::sum(const MleSum& p, hipStream_t st) {
  hipLaunchKernelGGL((k_mle_sum<FR>), dim3((unsigned)mle_blocks(p.n, p.tile_log)), dim3(MLE_THREADS), 0, st, p);
  return hipGetLastError();
}

template struct LaunchMle<Bls12_377_Fr29>;
template struct LaunchMle<Bls12_381_Fr29>;

}  // namespace msm
