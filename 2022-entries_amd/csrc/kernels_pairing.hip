// kernels_pairing.hip -- the kernels of pairing.hpp (Miller loops, the product tree, the final exponentiation) for the two families, in
// a unit of their own.
#include "launch_pairing.hpp"

namespace msm {

namespace {
inline unsigned pr_grid(uint64_t lanes) { return (unsigned)((lanes + PR_LANES - 1) / PR_LANES); }
}  // namespace

template <class E>
hipError_t LaunchPairing<E>::miller(const PrRun& p, uint64_t items, hipStream_t st) {
  if (items == 0) return hipSuccess;
  hipLaunchKernelGGL((k_pairing_miller<E>), dim3(pr_grid(items)), dim3(PR_LANES), 0, st, p, items);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchPairing<E>::product(const PrRun& p, uint64_t lanes, hipStream_t st) {
  if (lanes == 0) return hipSuccess;
  hipLaunchKernelGGL((k_pairing_product<E>), dim3(pr_grid(lanes)), dim3(PR_LANES), 0, st, p, lanes);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchPairing<E>::final(const PrRun& p, uint64_t groups, hipStream_t st) {
  if (groups == 0) return hipSuccess;
  hipLaunchKernelGGL((k_pairing_final<E>), dim3(pr_grid(groups)), dim3(PR_LANES), 0, st, p, groups);
  return hipGetLastError();
}

template struct LaunchPairing<Fp2El<Bls12_377_Fq, 5>>;
template struct LaunchPairing<Fp2El<Bls12_381_Fq, 1>>;

}  // namespace msm
