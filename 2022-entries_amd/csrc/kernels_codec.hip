// kernels_codec.hip -- k_decompress_points / k_compress_points (point_codec.hpp) for all four curves and both record forms, in a unit
// of its own so that the per-curve kernel units do not get slower to compile.
#include "point_codec.hpp"
#include "launch_codec.hpp"

namespace msm {

template <class E>
hipError_t LaunchCodec<E>::decompress(const uint8_t* in, uint32_t n, uint8_t* out, size_t stride, bool serialized, uint8_t* status, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + 255) / 256), block(256);
  if (serialized)
    hipLaunchKernelGGL((k_decompress_points<E, true>), grid, block, 0, st, in, n, out, stride, status);
  else
    hipLaunchKernelGGL((k_decompress_points<E, false>), grid, block, 0, st, in, n, out, stride, status);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchCodec<E>::compress(const uint8_t* in, size_t stride, uint32_t n, bool serialized, uint8_t* out, uint8_t* status, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + 255) / 256), block(256);
  if (serialized)
    hipLaunchKernelGGL((k_compress_points<E, true>), grid, block, 0, st, in, stride, n, out, status);
  else
    hipLaunchKernelGGL((k_compress_points<E, false>), grid, block, 0, st, in, stride, n, out, status);
  return hipGetLastError();
}

template struct LaunchCodec<Bls12_377_G1::E>;
template struct LaunchCodec<Bls12_381_G1::E>;
template struct LaunchCodec<Bls12_377_G2::E>;
template struct LaunchCodec<Bls12_381_G2::E>;

}  // namespace msm
