// kernels_lookup.hip -- the kernels of lookup.hpp (the canonical keys, the build and the probe of the hash table, the counters as
// elements, the u32 scan, the expansion of plookup's sorted vector, the rows of the logUp sum) for the two scalar fields, in a unit of
// its own.
#include "launch_lookup.hpp"

namespace msm {

namespace {
unsigned lookup_grid(uint64_t n) { return (unsigned)((n + LOOKUP_THREADS - 1) / LOOKUP_THREADS); }
unsigned lookup_scan_grid(uint64_t n) { return (unsigned)((n + ((uint64_t)1 << LOOKUP_SCAN_TILE_LOG) - 1) >> LOOKUP_SCAN_TILE_LOG); }
}  // namespace

template <class FR>
hipError_t LaunchLookup<FR>::canon(const LookupCanon& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lookup_canon<FR>), dim3(lookup_grid(p.n)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::build(const LookupBuild& p, hipStream_t st) {
  if (p.t.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lookup_build<FR>), dim3(lookup_grid(p.t.n)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::mult(const LookupMult& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lookup_mult<FR>), dim3(lookup_grid(p.n)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::probe(const LookupProbe& p, hipStream_t st) {
  if (p.n_f == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lookup_probe<FR>), dim3(lookup_grid((p.n_f + p.batches - 1) / p.batches)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::scan_up(const LookupScan& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lookup_scan_up<FR>), dim3(lookup_scan_grid(p.n)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::scan_down(const LookupScan& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lookup_scan_down<FR>), dim3(lookup_scan_grid(p.n)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::expand(const LookupExpand& p, hipStream_t st) {
  if (p.total == 0) return hipSuccess;
  hipLaunchKernelGGL((k_lookup_expand<FR>), dim3(lookup_grid(p.total)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::logup_den(const LogupRows& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_logup_den<FR>), dim3(lookup_grid(p.n)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template <class FR>
hipError_t LaunchLookup<FR>::logup_term(const LogupRows& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL((k_logup_term<FR>), dim3(lookup_grid(p.n)), dim3(LOOKUP_THREADS), 0, st, p);
  return hipGetLastError();
}

template struct LaunchLookup<Bls12_377_Fr29>;
template struct LaunchLookup<Bls12_381_Fr29>;

}  // namespace msm
