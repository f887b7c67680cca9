// launch_impl.hpp -- definitions of Launch<E> and WalkLaunch<G>; include only from the kernels_*.hip units that instantiate them.
#pragma once
#include <type_traits>
#include "launch.hpp"
#include "msm_kernels.hpp"

namespace msm {

inline uint32_t launch_blocks(uint64_t n) { return (uint32_t)((n + 255) / 256); }

template <class E>
hipError_t Launch<E>::convert_bases(const uint8_t* in, size_t stride, uint32_t n, bool serialized, AffineDevT<El>* out, uint8_t* inf,
                                    hipStream_t st) {
  if (serialized)
    hipLaunchKernelGGL((k_convert_bases<E, true>), dim3(launch_blocks(n)), dim3(256), 0, st, in, stride, n, out, inf);
  else
    hipLaunchKernelGGL((k_convert_bases<E, false>), dim3(launch_blocks(n)), dim3(256), 0, st, in, stride, n, out, inf);
  return hipGetLastError();
}

template <class E>
hipError_t Launch<E>::pre_double(const AffineDevT<El>* in, const uint8_t* inf_in, uint32_t n, uint32_t c, XyzzDevT<El>* out, hipStream_t st) {
  hipLaunchKernelGGL((k_pre_double<E>), dim3(launch_blocks(n)), dim3(256), 0, st, in, inf_in, n, c, out);
  return hipGetLastError();
}

template <class E>
hipError_t Launch<E>::pre_normalize(const XyzzDevT<El>* in, uint32_t n, uint32_t J, El* prefix, AffineDevT<El>* out, uint8_t* inf_out,
                                    hipStream_t st) {
  hipLaunchKernelGGL((k_pre_normalize<E>), dim3(launch_blocks(((uint64_t)n + J - 1) / J)), dim3(256), 0, st, in, n, J, prefix, out, inf_out);
  return hipGetLastError();
}

// ---- the walking kernels, once for every law ----------------------------------------------------------------------------------------
// The law of the four-lanes-per-addition form of G's two latency-bound kernels (msm_kernels.hpp); void: G has none.
template <class G>
struct QuadOf {
  using Q = void;
};
template <class E>
struct QuadOf<SwLaw<E>> {
  using Q = SwQuad<E>;
};
template <class F>
struct QuadOf<TeLaw<F>> {
  using Q = TeQuad<F>;
};
template <class G>
inline constexpr bool kHasQuad = !std::is_void_v<typename QuadOf<G>::Q>;

template <class G>
inline constexpr bool kIsSwLaw = false;
template <class E>
inline constexpr bool kIsSwLaw<SwLaw<E>> = true;

// a grid of `walkers` walkers: walker t is the G::LANES neighbouring hardware lanes from G::LANES * t
template <class G>
uint32_t walk_blocks(uint64_t walkers) {
  static_assert(std::is_same_v<typename LawMem<G>::MemT, typename G::MemT> && std::is_same_v<typename LawMem<G>::BaseDev, typename G::BaseDev>,
                "LawMem (launch.hpp) restates the law's memory types");
  return launch_blocks(G::LANES * walkers);
}

template <class G>
hipError_t WalkLaunch<G>::accumulate(const uint2* entries, const uint32_t* n_real, uint32_t K, const BaseDev* bases, SegOutT<El> out, uint32_t nlanes,
                                     uint32_t* flags, uint32_t e32_rk_off, hipStream_t st) {
  // MSM_GATHER = 0 builds the one-lane-per-record walk of the XYZZ laws instead (A/B: profiles/r02_ab_gather.txt)
#ifndef MSM_GATHER
#define MSM_GATHER 2
#endif
  if (e32_rk_off) {
    const uint32_t* const words = reinterpret_cast<const uint32_t*>(entries);
    const Entries32Ptr e32{words, words + e32_rk_off};
    if constexpr (MSM_GATHER == 2 || !kIsSwLaw<G>)
      hipLaunchKernelGGL((k_accumulate_glds<G, Entries32>), dim3(walk_blocks<G>(nlanes)), dim3(256), 0, st, e32, n_real, K, bases, out, nlanes, flags);
    else
      hipLaunchKernelGGL((k_accumulate<G, Entries32>), dim3(walk_blocks<G>(nlanes)), dim3(256), 0, st, e32, n_real, K, bases, out, nlanes, flags);
    return hipGetLastError();
  }
  if constexpr (MSM_GATHER == 2 || !kIsSwLaw<G>)
    hipLaunchKernelGGL((k_accumulate_glds<G>), dim3(walk_blocks<G>(nlanes)), dim3(256), 0, st, entries, n_real, K, bases, out, nlanes, flags);
  else
    hipLaunchKernelGGL((k_accumulate<G>), dim3(walk_blocks<G>(nlanes)), dim3(256), 0, st, entries, n_real, K, bases, out, nlanes, flags);
  return hipGetLastError();
}

template <class G>
hipError_t WalkLaunch<G>::sum_bases(const BaseDev* bases, const uint8_t* inf, uint32_t first, uint32_t n, uint32_t per_lane, SegOutT<El> out,
                                    uint32_t nlanes, uint32_t* flags, hipStream_t st) {
  if constexpr (G::LANES != 1) {
    return hipErrorNotSupported;   // (the sum of bases is never paired: no such kernel is built)
  } else {
    hipLaunchKernelGGL((k_sum_bases<G>), dim3(walk_blocks<G>(nlanes)), dim3(256), 0, st, bases, inf, first, n, per_lane, out, nlanes, flags);
    return hipGetLastError();
  }
}

template <class G>
hipError_t WalkLaunch<G>::segreduce(const XyzzDevT<El>* in_slots, const uint32_t* in_keys, uint32_t n_in, uint32_t K, SegOutT<El> out, uint32_t nlanes,
                                    uint32_t quad_limit, uint32_t* flags, hipStream_t st) {
  if constexpr (kHasQuad<G>) {
    if (nlanes <= quad_limit) {   // latency form: four lanes per addition (msm_kernels.hpp)
      hipLaunchKernelGGL((k_segreduce_quad<typename QuadOf<G>::Q>), dim3(launch_blocks(4ull * nlanes)), dim3(256), 0, st, in_slots, in_keys, n_in, K, out,
                         nlanes, flags);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((k_segreduce<G>), dim3(walk_blocks<G>(nlanes)), dim3(256), 0, st, in_slots, in_keys, n_in, K, out, nlanes, flags);
  return hipGetLastError();
}

template <class G>
hipError_t WalkLaunch<G>::bucket_reduce(bool first, const XyzzDevT<El>* in_a, const XyzzDevT<El>* in_x, uint32_t n_per_win, uint32_t L, uint32_t chunks,
                                        uint32_t windows, uint32_t out_stride, XyzzDevT<El>* out_a, XyzzDevT<El>* out_x, uint32_t* flags, hipStream_t st,
                                        uint32_t run_win) {
  dim3 grid(walk_blocks<G>((uint64_t)windows * chunks));
  if (first)
    hipLaunchKernelGGL((k_bucket_reduce<G, true>), grid, dim3(256), 0, st, in_a, in_x, n_per_win, L, chunks, windows, out_stride, out_a, out_x, flags, run_win);
  else
    hipLaunchKernelGGL((k_bucket_reduce<G, false>), grid, dim3(256), 0, st, in_a, in_x, n_per_win, L, chunks, windows, out_stride, out_a, out_x, flags, run_win);
  return hipGetLastError();
}

template <class G>
hipError_t WalkLaunch<G>::reduce_scan_step(const XyzzDevT<El>* in, const XyzzDevT<El>* in2, XyzzDevT<El>* out, uint32_t nb, uint32_t windows, uint32_t d,
                                           uint32_t mode, uint32_t quad_limit, uint32_t* flags, hipStream_t st) {
  const uint64_t threads = (uint64_t)windows * (mode == 1 ? d : nb);
  if constexpr (kHasQuad<G>) {
    if (threads <= quad_limit) {
      hipLaunchKernelGGL((k_reduce_scan_step_quad<typename QuadOf<G>::Q>), dim3(launch_blocks(4 * threads)), dim3(256), 0, st, in, in2, out, nb, windows, d,
                         mode, flags);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((k_reduce_scan_step<G>), dim3(walk_blocks<G>(threads)), dim3(256), 0, st, in, in2, out, nb, windows, d, mode, flags);
  return hipGetLastError();
}

template <class G>
hipError_t WalkLaunch<G>::bucket_merge(XyzzDevT<El>* total, const XyzzDevT<El>* part, uint32_t n, uint32_t* flags, hipStream_t st) {
  if constexpr (G::CARRY_IN) {
    return hipErrorNotSupported;   // (such a law accumulates a later chunk straight onto the stored buckets: no such kernel is built)
  } else {
    hipLaunchKernelGGL((k_bucket_merge<G>), dim3(walk_blocks<G>(n)), dim3(256), 0, st, total, part, n, flags);
    return hipGetLastError();
  }
}

// Every launcher of curve E under its one-lane law, member by member; kernels_<curve>.hip.  A unit's kernels lie in its code object in the order in
// which their launchers are instantiated, and this is the order the units have always had: a change of host code leaves their code objects the same
// byte for byte (a kernel that moves changes its pc-relative literals).
#define MSM_INSTANTIATE_SW_LAUNCHERS(E)                                                                                                          \
  using A_ = AffineDevT<E::T>;                                                                                                                   \
  using X_ = XyzzDevT<E::T>;                                                                                                                     \
  using S_ = SegOutT<E::T>;                                                                                                                      \
  using W_ = WalkLaunch<SwLaw<E>>;                                                                                                               \
  template hipError_t Launch<E>::convert_bases(const uint8_t*, size_t, uint32_t, bool, A_*, uint8_t*, hipStream_t);                              \
  template hipError_t W_::accumulate(const uint2*, const uint32_t*, uint32_t, const A_*, S_, uint32_t, uint32_t*, uint32_t, hipStream_t);        \
  template hipError_t W_::segreduce(const X_*, const uint32_t*, uint32_t, uint32_t, S_, uint32_t, uint32_t, uint32_t*, hipStream_t);             \
  template hipError_t Launch<E>::pre_double(const A_*, const uint8_t*, uint32_t, uint32_t, X_*, hipStream_t);                                    \
  template hipError_t Launch<E>::pre_normalize(const X_*, uint32_t, uint32_t, E::T*, A_*, uint8_t*, hipStream_t);                                \
  template hipError_t W_::bucket_reduce(bool, const X_*, const X_*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, X_*, X_*, uint32_t*, hipStream_t, uint32_t); \
  template hipError_t W_::reduce_scan_step(const X_*, const X_*, X_*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, hipStream_t); \
  template hipError_t W_::bucket_merge(X_*, const X_*, uint32_t, uint32_t*, hipStream_t);                                                        \
  template hipError_t W_::sum_bases(const A_*, const uint8_t*, uint32_t, uint32_t, uint32_t, S_, uint32_t, uint32_t*, hipStream_t);

}  // namespace msm
