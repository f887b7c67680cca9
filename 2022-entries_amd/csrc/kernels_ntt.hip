// kernels_ntt.hip -- the transform kernels (ntt.hpp) for the two scalar fields, in a unit of its own so that the per-curve kernel
// units do not get slower to compile.
#include "launch_ntt.hpp"

namespace msm {

template <class FR>
hipError_t LaunchNtt<FR>::pass(const NttPass& ps, uint32_t batch, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  const uint32_t tiles = 1u << (ps.k - ps.p - ps.log_c);
  hipLaunchKernelGGL((k_ntt_pass<FR>), dim3(tiles, batch), dim3(NTT_THREADS), 0, st, ps);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchNtt<FR>::mul_vec(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, bool normal, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_fr_mul_vec<FR>), dim3((unsigned)((n + NTT_THREADS - 1) / NTT_THREADS)), dim3(NTT_THREADS), 0, st, a, b, out, n, normal ? 1u : 0u);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchNtt<FR>::table(const Fr& base, uint32_t n, Fr* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_ntt_table<FR>), dim3((n + NTT_THREADS - 1) / NTT_THREADS), dim3(NTT_THREADS), 0, st, base, n, out);
  return hipGetLastError();
}

template struct LaunchNtt<Bls12_377_Fr29>;
template struct LaunchNtt<Bls12_381_Fr29>;

// the yardstick of tests/test_isa_ntt.py (never launched)
template __global__ void k_fr_yardstick<Bls12_377_Fr29>(const Fr*, const Fr*, Fr*, uint32_t);
template __global__ void k_fr_yardstick<Bls12_381_Fr29>(const Fr*, const Fr*, Fr*, uint32_t);

}  // namespace msm
