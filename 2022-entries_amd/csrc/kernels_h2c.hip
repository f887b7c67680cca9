// kernels_h2c.hip -- the kernels of h2c.hpp (expand_message_xmd with the reduction, the map, the pair sum with the cofactor
// clearing) for the two groups of BLS12-381, in a unit of their own.
#include "launch_h2c.hpp"

namespace msm {

namespace {
inline unsigned h2c_grid(uint32_t lanes) { return (lanes + H2C_LANES - 1) / H2C_LANES; }
}  // namespace

template <class E>
hipError_t LaunchH2c<E>::expand(const H2cRun& p, uint32_t n, uint32_t elems, uint32_t* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_h2c_expand<typename E::Fld>), dim3(h2c_grid(n)), dim3(H2C_LANES), 0, st, p, n, elems, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchH2c<E>::map(const uint32_t* u, uint32_t n, uint8_t* ws, XyzzDevT<El>* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_h2c_map<E>), dim3(h2c_grid(n)), dim3(H2C_LANES), 0, st, u, n, ws, out);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchH2c<E>::clear(const XyzzDevT<El>* in, uint32_t n, bool pairs, uint8_t* ws, XyzzDevT<El>* out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_h2c_clear<E>), dim3(h2c_grid(n)), dim3(H2C_LANES), 0, st, in, n, pairs ? 1u : 0u, ws, out);
  return hipGetLastError();
}

template struct LaunchH2c<Bls12_381_G1::E>;
template struct LaunchH2c<Bls12_381_G2::E>;

}  // namespace msm
