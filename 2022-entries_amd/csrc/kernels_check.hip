// kernels_check.hip -- k_check_points (check_points.hpp) for all four curves and both methods, in a unit of its own so that the
// per-curve kernel units do not get slower to compile.
#include "check_points.hpp"
#include "launch.hpp"

namespace msm {

template <class E>
hipError_t Launch<E>::check_points(const uint8_t* in, size_t stride, uint32_t n, bool serialized, bool exact, uint8_t* status, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + 255) / 256), block(256);
  if (serialized) {
    if (exact)
      hipLaunchKernelGGL((k_check_points<E, true, CHECK_EXACT>), grid, block, 0, st, in, stride, n, status);
    else
      hipLaunchKernelGGL((k_check_points<E, true, CHECK_ENDO>), grid, block, 0, st, in, stride, n, status);
  } else {
    if (exact)
      hipLaunchKernelGGL((k_check_points<E, false, CHECK_EXACT>), grid, block, 0, st, in, stride, n, status);
    else
      hipLaunchKernelGGL((k_check_points<E, false, CHECK_ENDO>), grid, block, 0, st, in, stride, n, status);
  }
  return hipGetLastError();
}

template hipError_t Launch<Bls12_377_G1::E>::check_points(const uint8_t*, size_t, uint32_t, bool, bool, uint8_t*, hipStream_t);
template hipError_t Launch<Bls12_381_G1::E>::check_points(const uint8_t*, size_t, uint32_t, bool, bool, uint8_t*, hipStream_t);
template hipError_t Launch<Bls12_377_G2::E>::check_points(const uint8_t*, size_t, uint32_t, bool, bool, uint8_t*, hipStream_t);
template hipError_t Launch<Bls12_381_G2::E>::check_points(const uint8_t*, size_t, uint32_t, bool, bool, uint8_t*, hipStream_t);

}  // namespace msm
