// kernels_fixed.hip -- the fixed-base kernels (fixed_base.hpp) for all four curves, in a unit of its own so that the per-curve kernel
// units do not get slower to compile.
#include "fixed_base.hpp"
#include "launch_fixed.hpp"

namespace msm {

template <class E>
hipError_t LaunchFixed<E>::level_bases(const uint8_t* d_img, uint32_t w, uint32_t levels, XyzzDevT<El>* out, hipStream_t st) {
  hipLaunchKernelGGL((k_fb_level_bases<E>), dim3(1), dim3(64), 0, st, d_img, w, levels, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchFixed<E>::table(const AffineDevT<El>* lbase, const uint8_t* lbase_inf, uint32_t w, uint32_t levels, XyzzDevT<El>* out, hipStream_t st) {
  const uint32_t runs = ((1u << w) + FB_TABLE_RUN - 1) / FB_TABLE_RUN;
  hipLaunchKernelGGL((k_fb_table<E>), dim3((levels * runs + 255) / 256), dim3(256), 0, st, lbase, lbase_inf, w, levels, runs, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchFixed<E>::mul(const AffineDevT<El>* table, const uint32_t* scalars, uint32_t n, uint32_t w, uint32_t levels, bool from_mont,
                               XyzzDevT<El>* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_fb_mul<E>), dim3((n + 255) / 256), dim3(256), 0, st, table, scalars, n, w, levels, from_mont ? 1u : 0u, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchFixed<E>::normalize(const XyzzDevT<El>* in, uint32_t n, El* prefix, uint8_t* out, size_t out_stride, bool projective, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const dim3 grid(((n + FB_NORM_RUN - 1) / FB_NORM_RUN + 255) / 256), block(256);
  if (projective)
    hipLaunchKernelGGL((k_fb_normalize<E, true>), grid, block, 0, st, in, n, prefix, out, out_stride);
  else
    hipLaunchKernelGGL((k_fb_normalize<E, false>), grid, block, 0, st, in, n, prefix, out, out_stride);
  return hipGetLastError();
}

template struct LaunchFixed<Bls12_377_G1::E>;
template struct LaunchFixed<Bls12_381_G1::E>;
template struct LaunchFixed<Bls12_377_G2::E>;
template struct LaunchFixed<Bls12_381_G2::E>;

}  // namespace msm
