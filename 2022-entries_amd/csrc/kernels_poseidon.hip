// kernels_poseidon.hip -- the kernel of poseidon.hpp (n sponges of one shape, one lane each) for the two scalar fields, in a unit of
// its own.
#include "launch_poseidon.hpp"

namespace msm {

template <class FR>
hipError_t LaunchPoseidon<FR>::hash(const PosRun& p, hipStream_t st) {
  if (p.n == 0 || p.n_out == 0) return hipSuccess;
  const unsigned grid = (unsigned)((p.n + POS_LANES - 1) / POS_LANES);
  hipLaunchKernelGGL((k_poseidon_hash<FR>), dim3(grid), dim3(POS_LANES), pos_lds_bytes(p.tab.t), st, p);
  return hipGetLastError();
}

template struct LaunchPoseidon<Bls12_377_Fr29>;
template struct LaunchPoseidon<Bls12_381_Fr29>;

}  // namespace msm
