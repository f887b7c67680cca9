// launch.hpp -- host-callable launchers of the per-curve kernels.  Declared here, defined in launch_impl.hpp and explicitly
// instantiated once per curve and law in kernels_<curve>.hip, kernels_<curve>p.hip and kernels_377te.hip, so the instantiations (each
// minutes of hipcc time: every field multiply is fully unrolled) compile in parallel and the engine TU stays small.  The engine never
// sees launch_impl.hpp: its calls of WalkLaunch<G> resolve at link time to the members those units instantiate.
#pragma once
#include <hip/hip_runtime.h>

#include "host_curve.hpp"
#include "msm_types.hpp"
#include "partition_plan.hpp"
#include "te.hpp"

namespace msm {

// The group laws of the walking kernels (laws.hpp), declared only: the engine names them and never sees a kernel.
template <class E>
struct SwLaw;
template <class F>
struct TeLaw;
template <class F, int NB>
struct SwPairLaw;

// What a law keeps in memory (G::MemT and G::BaseDev of laws.hpp), for units that see only the declarations above.
template <class G>
struct LawMem;
template <class E>
struct LawMem<SwLaw<E>> {
  using MemT = typename E::T;
  using BaseDev = AffineDevT<MemT>;
};
template <class F>
struct LawMem<TeLaw<F>> {
  using MemT = Fe;
  using BaseDev = TeAffineDev;
};
template <class F, int NB>
struct LawMem<SwPairLaw<F, NB>> {   // the records of SwLaw<Fp2El<F, NB>>: the two forms mix freely
  using MemT = Fe2;
  using BaseDev = AffineDevT<Fe2>;
};

// The second form of a law's kernels: G2 with every Fp2 value spread over two neighbouring lanes (SwPairLaw is device code only:
// laws.hpp, fp2pair.hpp).  Over Fp, and for TeLaw, there is one form.
template <class G>
struct PairedForm {
  using L = G;
};
template <class F, int NB>
struct PairedForm<SwLaw<Fp2El<F, NB>>> {
  using L = SwPairLaw<F, NB>;
};

// The six walking kernels under law G, G::LANES hardware lanes per walker.  G = SwLaw<E> (kernels_<curve>.hip), SwPairLaw<F, NB> (G2
// with every Fp2 value spread over two neighbouring lanes: kernels_<curve>p.hip) or TeLaw<TeFq> (the twisted-Edwards fast path of
// BLS12-377 G1: kernels_377te.hip).  `flags` (TeLaw only, nullptr otherwise): [1] = 1 when an addition hit a vanishing denominator.
// `quad_limit` (per context, option "quad_limit"): launches of at most that many additions use the four-lanes-per-addition kernels
// (latency), larger ones G::LANES lanes each (throughput); SwPairLaw has no quad form and ignores it -- the engine picks the law of
// a G2 launch (walk_form).  Not every law has every kernel: SwPairLaw has no sum_bases, and TeLaw no bucket_merge (the later chunks
// of a carried batch accumulate straight onto the stored buckets -- SegOutT::carry_in).  (The order of the members is the order of
// the kernels in the code object of a unit that instantiates the struct as a whole.)
template <class G>
struct WalkLaunch {
  using El = typename LawMem<G>::MemT;
  using BaseDev = typename LawMem<G>::BaseDev;
  // `e32_rk_off` != 0: the entries are Entries32 words (msm_types.hpp) and run_keys starts that many words into the buffer
  static hipError_t accumulate(const uint2* entries, const uint32_t* n_real, uint32_t K, const BaseDev* bases, SegOutT<El> out, uint32_t nlanes,
                               uint32_t* flags, uint32_t e32_rk_off, hipStream_t st);
  // anchored window: one fragment per lane of the plain sum of bases [first, first + n) (k_sum_bases)
  static hipError_t sum_bases(const BaseDev* bases, const uint8_t* inf, uint32_t first, uint32_t n, uint32_t per_lane, SegOutT<El> out, uint32_t nlanes,
                              uint32_t* flags, hipStream_t st);
  static hipError_t segreduce(const XyzzDevT<El>* in_slots, const uint32_t* in_keys, uint32_t n_in, uint32_t K, SegOutT<El> out, uint32_t nlanes,
                              uint32_t quad_limit, uint32_t* flags, hipStream_t st);
  static hipError_t bucket_reduce(bool first, const XyzzDevT<El>* in_a, const XyzzDevT<El>* in_x, uint32_t n_per_win, uint32_t L, uint32_t chunks,
                                  uint32_t windows, uint32_t out_stride, XyzzDevT<El>* out_a, XyzzDevT<El>* out_x, uint32_t* flags, hipStream_t st,
                                  uint32_t run_win = 0xffffffffu);   // (first level: this window's plain chunk sums become the A of row `windows`)
  // small windows: one step of the scan-based reduction (k_reduce_scan_step)
  static hipError_t reduce_scan_step(const XyzzDevT<El>* in, const XyzzDevT<El>* in2, XyzzDevT<El>* out, uint32_t nb, uint32_t windows, uint32_t d,
                                     uint32_t mode, uint32_t quad_limit, uint32_t* flags, hipStream_t st);
  // carried buckets: total[b] += part[b] (k_bucket_merge)
  static hipError_t bucket_merge(XyzzDevT<El>* total, const XyzzDevT<El>* part, uint32_t n, uint32_t* flags, hipStream_t st);
};

// The kernels that walk nothing: base conversion, the table builders, the point check.
template <class E>
struct Launch {
  using El = typename E::T;
  static hipError_t convert_bases(const uint8_t* in, size_t stride, uint32_t n, bool serialized, AffineDevT<El>* out, uint8_t* inf,
                                  hipStream_t st);
  static hipError_t pre_double(const AffineDevT<El>* in, const uint8_t* inf_in, uint32_t n, uint32_t c, XyzzDevT<El>* out, hipStream_t st);
  static hipError_t pre_normalize(const XyzzDevT<El>* in, uint32_t n, uint32_t J, El* prefix, AffineDevT<El>* out, uint8_t* inf_out,
                                  hipStream_t st);
  // one status byte per record (check_points.hpp): 0 valid, 1 not canonical, 2 off the curve, 3 outside the order-r subgroup.
  // Defined and instantiated in kernels_check.hip, not with the rest of the struct.
  static hipError_t check_points(const uint8_t* in, size_t stride, uint32_t n, bool serialized, bool exact, uint8_t* status, hipStream_t st);
};

// The base converter of the twisted-Edwards fast path (kernels_377te.hip).  `flags`: [0] += bases without an image.
struct LaunchTe {
  static constexpr uint32_t kDefaultQuadLimit = 1u << 18;   // tools/quad_limit_sweep.py: flat from 2^16 up, 2^18 best at 2^20 pairs
  static hipError_t convert(const AffineDev* in, const uint8_t* inf, uint32_t n, uint32_t J, Fe* prefix, TeAffineDev* out, uint32_t* flags,
                            hipStream_t st);
};

// Bucket grouping (partition.hip): digits + MSD partition of the (key, value) entries.  scalar_field: 0 = BLS12-377 Fr, 1 = BLS12-381 Fr
// (only the Montgomery conversions depend on it); scalar_mode: a ScalarMode of digits.hpp.  Returns the index of the entry buffer that holds the sorted entries.
struct PartLaunch {
  static int run(int scalar_field, int scalar_mode, const uint32_t* d_scalars, const uint8_t* d_inf, const PartPlan& p, const PartBuffers& b,
                 hipStream_t st, hipEvent_t mid, hipError_t& err);
  // -DMSM_DEBUG builds only (otherwise a no-op that reports nothing): the slot-key check after the accumulation, then the stream is
  // synchronised and the violation counters of this chunk are read -- what[] names the first violated invariant, empty = all held.
  static hipError_t debug_finish(const PartPlan& p, const PartBuffers& b, const uint32_t* slot_keys, uint32_t nslots, hipStream_t st, char* what,
                                 size_t what_len, uint64_t* checks_done);
};

extern template struct Launch<Bls12_377_G1::E>;
extern template struct Launch<Bls12_381_G1::E>;
extern template struct Launch<Bls12_377_G2::E>;
extern template struct Launch<Bls12_381_G2::E>;

}  // namespace msm
