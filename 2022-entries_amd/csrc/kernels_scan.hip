// kernels_scan.hip -- the kernels of scan.hpp (prefix product, prefix sum, the rows of the permutation product) for the two scalar
// fields, in a unit of its own.
#include "launch_scan.hpp"

namespace msm {

namespace {
unsigned scan_grid(const ScanTile& s) { return (unsigned)poly_tiles(s.t.n, s.t.tile_log); }
}  // namespace

template <class FR>
hipError_t LaunchScan<FR>::up(unsigned op, const ScanUp& p, hipStream_t st) {
  if (p.s.t.n == 0) return hipSuccess;
  if (op == kScanProduct)
    hipLaunchKernelGGL((k_scan_up<FR, kScanProduct>), dim3(scan_grid(p.s)), dim3(POLY_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL((k_scan_up<FR, kScanSum>), dim3(scan_grid(p.s)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchScan<FR>::down(unsigned op, const ScanDown& p, hipStream_t st) {
  if (p.s.t.n == 0) return hipSuccess;
  if (op == kScanProduct)
    hipLaunchKernelGGL((k_scan_down<FR, kScanProduct>), dim3(scan_grid(p.s)), dim3(POLY_THREADS), 0, st, p);
  else
    hipLaunchKernelGGL((k_scan_down<FR, kScanSum>), dim3(scan_grid(p.s)), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchScan<FR>::perm(const ScanPerm& p, hipStream_t st) {
  const uint32_t n = 1u << p.k;
  hipLaunchKernelGGL((k_scan_perm<FR>), dim3((n + POLY_THREADS - 1) / POLY_THREADS), dim3(POLY_THREADS), 0, st, p);
  return hipGetLastError();
}

template struct LaunchScan<Bls12_377_Fr29>;
template struct LaunchScan<Bls12_381_Fr29>;

}  // namespace msm
