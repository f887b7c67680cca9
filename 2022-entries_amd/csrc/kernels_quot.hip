// kernels_quot.hip -- the kernels of quotient.hpp (x - 1 per row, the rows of the Plonk quotient, the linear combination) for the two
// scalar fields, in a unit of its own.
#include "launch_quot.hpp"

namespace msm {

namespace {
unsigned quot_grid(uint64_t n) { return (unsigned)((n + POLY_THREADS - 1) / POLY_THREADS); }
}  // namespace

template <class FR>
hipError_t LaunchQuot<FR>::xm1(const QuotXm1& p, hipStream_t st) {
  hipLaunchKernelGGL((k_quot_xm1<FR>), dim3(quot_grid((uint64_t)1 << p.k)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchQuot<FR>::rows(const QuotRows& p, hipStream_t st) {
  hipLaunchKernelGGL((k_quot_rows<FR>), dim3(quot_grid((uint64_t)1 << p.k)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchQuot<FR>::lincomb(const LinComb& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lincomb<FR>), dim3(quot_grid(p.n)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template struct LaunchQuot<Bls12_377_Fr29>;
template struct LaunchQuot<Bls12_381_Fr29>;

}  // namespace msm
