// kernels_377te.hip -- the walking kernels instantiated for the twisted-Edwards image of BLS12-377 G1 (te.hpp, laws.hpp),
// and the base converter.  Its own translation unit so that it compiles in parallel with the per-curve units.
#include "launch_impl.hpp"

namespace msm {

hipError_t LaunchTe::convert(const AffineDev* in, const uint8_t* inf, uint32_t n, uint32_t J, Fe* prefix, TeAffineDev* out, uint32_t* flags,
                             hipStream_t st) {
  hipLaunchKernelGGL((k_te_convert<Bls12_377_Fq, TeFq>), dim3(launch_blocks(((uint64_t)n + J - 1) / J)), dim3(256), 0, st, in, inf, n, J, prefix, out, flags);
  return hipGetLastError();
}

template struct WalkLaunch<TeLaw<TeFq>>;   // the limb shape of the Edwards path: te.hpp (no bucket_merge: launch_impl.hpp)

}  // namespace msm
