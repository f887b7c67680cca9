// kernels_gfft.hip -- the point-transform kernels (group_fft.hpp) for all four curves, in a unit of its own so that the per-curve
// kernel units do not get slower to compile.
#include "group_fft.hpp"
#include "launch_gfft.hpp"

namespace msm {

template <class E>
hipError_t LaunchGfft<E>::table(const GfVec& v, uint32_t k, uint32_t s, bool stage_mode, uint32_t b0, uint32_t cn, uint32_t entries, XyzzDevT<El>* out,
                                hipStream_t st) {
  if (cn == 0) return hipSuccess;
  hipLaunchKernelGGL((k_gf_table<E>), dim3((cn + 255) / 256), dim3(256), 0, st, v, k, s, stage_mode ? 1u : 0u, b0, cn, entries, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchGfft<E>::stage(const GfVec& v, const AffineDevT<El>* table, const NttTable& tw, uint32_t k, uint32_t s, uint32_t b0, uint32_t cn, uint32_t w,
                                XyzzDevT<El>* out, hipStream_t st) {
  if (cn == 0) return hipSuccess;
  if (s == 0)
    hipLaunchKernelGGL((k_gf_stage<E, false>), dim3((cn + 255) / 256), dim3(256), 0, st, v, table, tw, k, s, b0, cn, w, out);
  else
    hipLaunchKernelGGL((k_gf_stage<E, true>), dim3((cn + 255) / 256), dim3(256), 0, st, v, table, tw, k, s, b0, cn, w, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchGfft<E>::scale(const AffineDevT<El>* table, const GfScale& fs, uint32_t k, uint32_t j0, uint32_t cn, uint32_t w, XyzzDevT<El>* out,
                                hipStream_t st) {
  if (cn == 0) return hipSuccess;
  hipLaunchKernelGGL((k_gf_scale<E>), dim3((cn + 255) / 256), dim3(256), 0, st, table, fs, k, j0, cn, w, out);
  return hipGetLastError();
}

template struct LaunchGfft<Bls12_377_G1::E>;
template struct LaunchGfft<Bls12_381_G1::E>;
template struct LaunchGfft<Bls12_377_G2::E>;
template struct LaunchGfft<Bls12_381_G2::E>;

}  // namespace msm
