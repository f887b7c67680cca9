// kernels_sparse.hip -- the kernels of sparse.hpp (the coefficients at create; z to class M, the lane totals, the rows and the rows
// that cross a lane boundary at apply) for the two scalar fields, in a unit of its own.
#include "launch_sparse.hpp"

namespace msm {

namespace {
unsigned sparse_grid(uint64_t n) { return (unsigned)((n + SPARSE_LANES - 1) / SPARSE_LANES); }
}  // namespace

template <class FR>
hipError_t LaunchSparse<FR>::vals(const SparseVals& p, hipStream_t st) {
  if (p.slots == 0) return hipSuccess;
  hipLaunchKernelGGL((k_sparse_vals<FR>), dim3(sparse_grid(p.slots)), dim3(SPARSE_LANES), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchSparse<FR>::z(const SparseZ& p, hipStream_t st) {
  if (p.cols == 0) return hipSuccess;
  hipLaunchKernelGGL((k_sparse_z<FR>), dim3(sparse_grid(p.cols)), dim3(SPARSE_LANES), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchSparse<FR>::totals(const SparseRun& p, hipStream_t st) {
  if (p.m.nlanes == 0) return hipSuccess;
  hipLaunchKernelGGL((k_sparse_totals<FR>), dim3(sparse_grid(p.m.nlanes)), dim3(SPARSE_LANES), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchSparse<FR>::rows(const SparseRun& p, hipStream_t st) {
  if (p.m.nlanes == 0) return hipSuccess;
  hipLaunchKernelGGL((k_sparse_rows<FR>), dim3(sparse_grid(p.m.nlanes)), dim3(SPARSE_LANES), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchSparse<FR>::cross(const SparseRun& p, hipStream_t st) {
  if (p.m.rows == 0) return hipSuccess;
  hipLaunchKernelGGL((k_sparse_cross<FR>), dim3(sparse_grid(p.m.rows)), dim3(SPARSE_LANES), 0, st, p);
  return hipGetLastError();
}

template struct LaunchSparse<Bls12_377_Fr29>;
template struct LaunchSparse<Bls12_381_Fr29>;

}  // namespace msm
