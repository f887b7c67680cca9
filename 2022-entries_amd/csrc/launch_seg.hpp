// launch_seg.hpp -- host-callable launchers of the segmented-MSM kernels (seg_msm.hpp).  Declared here, defined and instantiated for
// the four curves in kernels_seg.hip; the only other unit that includes it is the engine (msm_seg.hpp).
#pragma once
#include "launch.hpp"
#include "seg_msm.hpp"   // SmLaunch

namespace msm {

template <class E>
struct LaunchSeg {
  using El = typename E::T;
  // the window sums of one class: wsum[window * a.nseg + k] for segment k of the class
  static hipError_t accumulate(const SmLaunch& a, XyzzDevT<El>* wsum, hipStream_t st);
  // stage[ids[k]] = sum over the windows of segment k of the class (ids NULL: stage[k])
  static hipError_t tail(const XyzzDevT<El>* wsum, const uint32_t* ids, uint32_t nseg, uint32_t nwin, uint32_t c, XyzzDevT<El>* stage, hipStream_t st);
};

extern template struct LaunchSeg<Bls12_377_G1::E>;
extern template struct LaunchSeg<Bls12_381_G1::E>;
extern template struct LaunchSeg<Bls12_377_G2::E>;
extern template struct LaunchSeg<Bls12_381_G2::E>;

}  // namespace msm
