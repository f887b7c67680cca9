// launch_scan.hpp -- host-callable launchers of the kernels of scan.hpp.  Declared here, defined and instantiated for the two scalar
// fields in kernels_scan.hip; the only other unit that includes it is the engine (msm_scan.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "scan.hpp"

namespace msm {

template <class FR>
struct LaunchScan {
  // one block per tile of p.s.t.n elements; op: kScanProduct or kScanSum
  static hipError_t up(unsigned op, const ScanUp& p, hipStream_t st);
  static hipError_t down(unsigned op, const ScanDown& p, hipStream_t st);
  // one lane per row of the domain
  static hipError_t perm(const ScanPerm& p, hipStream_t st);
};

extern template struct LaunchScan<Bls12_377_Fr29>;
extern template struct LaunchScan<Bls12_381_Fr29>;

}  // namespace msm
