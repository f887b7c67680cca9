// kernels_poly.hip -- the kernels of poly.hpp (batch inversion, evaluation, division by X - z, Lagrange coefficients, element-wise
// calls) for the two scalar fields, in a unit of its own.
#include "launch_poly.hpp"

namespace msm {

namespace {
unsigned poly_grid(const PolyTile& t) { return (unsigned)poly_tiles(t.n, t.tile_log); }
}  // namespace

template <class FR>
hipError_t LaunchPoly<FR>::eval(const PolyEval& p, hipStream_t st) {
  if (p.t.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_poly_eval<FR>), dim3(poly_grid(p.t)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchPoly<FR>::div(const PolyDiv& p, hipStream_t st) {
  if (p.t.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_poly_div<FR>), dim3(poly_grid(p.t)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchPoly<FR>::inv_prod(const PolyInv& p, hipStream_t st) {
  if (p.t.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_poly_inv_prod<FR>), dim3(poly_grid(p.t)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchPoly<FR>::inv_apply(const PolyInv& p, hipStream_t st) {
  if (p.t.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_poly_inv_apply<FR>), dim3(poly_grid(p.t)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchPoly<FR>::inv_tiles(Fr* tiles, uint64_t count, const Fr& coeff, hipStream_t st) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL((k_poly_inv_tiles<FR>), dim3((unsigned)((count + POLY_THREADS - 1) / POLY_THREADS)), dim3(POLY_THREADS), 0, st, tiles, count, coeff);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchPoly<FR>::lagrange(const PolyLagrange& p, hipStream_t st) {
  const uint32_t n = 1u << p.k;
  hipLaunchKernelGGL((k_poly_lagrange<FR>), dim3((n + POLY_THREADS - 1) / POLY_THREADS), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchPoly<FR>::vec_op(const PolyVecOp& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_poly_vec_op<FR>), dim3((unsigned)((p.n + POLY_THREADS - 1) / POLY_THREADS)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template struct LaunchPoly<Bls12_377_Fr29>;
template struct LaunchPoly<Bls12_381_Fr29>;

}  // namespace msm
