// kernels_pmul.hip -- the point-multiplication kernels (point_mul.hpp) for all four curves, in a unit of its own so that the per-curve
// kernel units do not get slower to compile.
#include "point_mul.hpp"
#include "launch_pmul.hpp"

namespace msm {

template <class E>
hipError_t LaunchPmul<E>::table(const uint8_t* d_points, size_t stride, uint32_t n, uint32_t entries, XyzzDevT<El>* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_pm_table<E>), dim3((n + 255) / 256), dim3(256), 0, st, d_points, stride, n, entries, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchPmul<E>::mul(const AffineDevT<El>* table, const uint32_t* scalars, uint32_t n, uint32_t w, bool from_mont, XyzzDevT<El>* out,
                              hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_pm_mul<E>), dim3((n + 255) / 256), dim3(256), 0, st, table, scalars, n, w, from_mont ? 1u : 0u, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchPmul<E>::mul_uniform(const uint8_t* d_points, size_t stride, uint32_t n, const PmNaf& naf, XyzzDevT<El>* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_pm_mul_uniform<E>), dim3((n + 255) / 256), dim3(256), 0, st, d_points, stride, n, naf, out);
  return hipGetLastError();
}

template struct LaunchPmul<Bls12_377_G1::E>;
template struct LaunchPmul<Bls12_381_G1::E>;
template struct LaunchPmul<Bls12_377_G2::E>;
template struct LaunchPmul<Bls12_381_G2::E>;

}  // namespace msm
