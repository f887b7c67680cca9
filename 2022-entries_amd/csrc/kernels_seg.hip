// kernels_seg.hip -- the segmented-MSM kernels (seg_msm.hpp) for all four curves, in a unit of its own so that the per-curve kernel
// units do not get slower to compile.
#include "seg_msm.hpp"
#include "launch_seg.hpp"

namespace msm {

template <class E>
hipError_t LaunchSeg<E>::accumulate(const SmLaunch& a, XyzzDevT<El>* wsum, hipStream_t st) {
  if (a.nseg == 0) return hipSuccess;
  if (a.c < 1 || a.c > SM_MAX_WINDOW || a.tile < SM_MIN_TILE || a.tile > SM_MAX_TILE || (a.tile & (a.tile - 1))) return hipErrorInvalidValue;
  const uint64_t items = (uint64_t)a.nseg * a.nwin, blocks = (items + sm_slices(a.c) - 1) / sm_slices(a.c);
  const size_t lds = (size_t)4 * sm_lds_words(a.c, a.tile, sizeof(XyzzT<El>) / 4);
  if (blocks >= (1ull << 31) || lds > (152u << 10)) return hipErrorInvalidValue;
  if (lds > (64u << 10)) {   // (Fp2 at c = 9 alone: 256 lanes' points of 448 B, 112 KiB of the CU's 160)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sm_accumulate<E>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_sm_accumulate<E>), dim3((uint32_t)blocks), dim3(sm_block_threads(a.c)), lds, st, a, wsum);
  return hipGetLastError();
}

template <class E>
hipError_t LaunchSeg<E>::tail(const XyzzDevT<El>* wsum, const uint32_t* ids, uint32_t nseg, uint32_t nwin, uint32_t c, XyzzDevT<El>* stage, hipStream_t st) {
  if (nseg == 0) return hipSuccess;
  hipLaunchKernelGGL((k_sm_tail<E>), dim3((nseg + 63) / 64), dim3(64), 0, st, wsum, ids, nseg, nwin, c, stage);
  return hipGetLastError();
}

template struct LaunchSeg<Bls12_377_G1::E>;
template struct LaunchSeg<Bls12_381_G1::E>;
template struct LaunchSeg<Bls12_377_G2::E>;
template struct LaunchSeg<Bls12_381_G2::E>;

}  // namespace msm
