// msm_types.hpp -- device data layouts shared by the kernels and the host orchestration.
#pragma once
#include "curve.hpp"

namespace msm {

constexpr uint32_t KEY_NONE = 0xffffffffu;
constexpr uint32_t IDX_MASK = 0x7fffffffu;

// ---- Entries32: the sorted entry stream as ONE 32-bit word per entry ------------------------------------------------------------
// The accumulation never uses a key as a number per entry: it asks "same bucket as the entry before?" and needs the bucket's number
// only when it stores a finished run.  The entries are fully sorted, and with uniform scalars the next non-empty bucket is almost
// always the next bucket, so the key travels as its STEP from the entry before, in five spare bits of the value word:
//     bits 25..0  base index          bits 30..26  step          bit 31  sign (as in the 64-bit format)
//     step 0: the key of the entry before;  1..30: that key + step;  31: the key stands in run_keys[position]
// run_keys is a sparse uint32 array indexed like the entries, in the unused upper half of the same buffer (e32_run_keys_offset words
// from its start).  It is written where a reader cannot know the key otherwise: at escapes (a gap of more than 30 buckets, the first
// run of a grouping segment -- the block that writes it cannot know the previous segment's last key -- and every run start of a
// segment that was cut into sub-jobs), and at every position that is a multiple of the lane length K, where a walking lane starts.
// Written by the last grouping pass (partition.hpp, pass_scatter_tiles), read by k_accumulate / k_accumulate_glds (msm_kernels.hpp).
constexpr uint32_t E32_IDX_BITS = 26;
constexpr uint32_t E32_IDX_MASK = (1u << E32_IDX_BITS) - 1;
constexpr uint32_t E32_STEP_MASK = 31u;
constexpr uint32_t E32_MAX_STEP = 30u;
constexpr uint32_t E32_ESCAPE = 31u;
MSM_HD uint32_t e32_pack(uint32_t value, uint32_t step) { return (value & (0x80000000u | E32_IDX_MASK)) | (step << E32_IDX_BITS); }
MSM_HD uint32_t e32_step(uint32_t word) { return (word >> E32_IDX_BITS) & E32_STEP_MASK; }
MSM_HD uint32_t e32_index(uint32_t word) { return word & E32_IDX_MASK; }
// the step of a run start `gap` buckets above the run before it; the first run of a segment has no run before it that its writer knows
MSM_HD uint32_t e32_step_of_gap(uint32_t gap, bool first_of_segment) { return (first_of_segment || gap > E32_MAX_STEP) ? E32_ESCAPE : gap; }
// the key of the entry at `pos`, given the key of the entry before it
MSM_HD uint32_t e32_next_key(uint32_t prev_key, uint32_t word, const uint32_t* run_keys, uint32_t pos) {
  const uint32_t step = e32_step(word);
  return step == E32_ESCAPE ? run_keys[pos] : prev_key + step;
}
// where run_keys starts, in words from the start of a buffer made for `capacity` 64-bit entries (+ 128 bytes): behind the words and
// the 64 bytes of slack that the entry queue of k_accumulate_glds may read past the last entry
MSM_HD uint32_t e32_run_keys_offset(uint64_t capacity) { return (uint32_t)((capacity + 16 + 15) & ~(uint64_t)15); }
// the first lane start (multiple of K) at or after `pos`
MSM_HD uint32_t e32_first_lane_start(uint32_t pos, uint32_t K) { return (pos + K - 1) / K * K; }
// the format applies to a chunk of n pairs whose base indices [idx0, idx0 + n) fit 26 bits, without precomputed tables
MSM_HD bool e32_applies(uint64_t idx0, uint64_t n, uint32_t table_levels) { return table_levels <= 1 && n <= (1ull << E32_IDX_BITS) && idx0 + n <= (1ull << E32_IDX_BITS); }

// Device layouts: AoS, 16-byte aligned so one lane's gather/store is a run of dwordx4 accesses.
//   G1: affine 112 B (2 x 14 limbs), XYZZ 224 B;   G2: affine 224 B, XYZZ 448 B.
template <class T>
struct alignas(128) AffineDevT {
  AffineT<T> p;
};
template <class T>
struct alignas(16) XyzzDevT {
  XyzzT<T> p;
};
using AffineDev = AffineDevT<Fe>;
using XyzzDev = XyzzDevT<Fe>;
static_assert(sizeof(AffineDev) == 128 && sizeof(AffineDevT<Fe2>) == 256, "device affine layout");
static_assert(sizeof(XyzzDev) == 224 && sizeof(XyzzDevT<Fe2>) == 448, "device xyzz layout");

template <class T>
struct SegOutT {
  XyzzDevT<T>* buckets;
  XyzzDevT<T>* slots;   // 2 per lane: [2t] head, [2t+1] tail
  uint32_t* slot_keys;  // KEY_NONE = empty slot
  // 1: the buckets already hold the sums of the batch's earlier chunks (carried buckets): the run that STARTS a bucket in this chunk
  // begins from the stored value instead of the identity, so the chunk's sums land on top of it with no merge pass
  uint32_t carry_in = 0;
};
using SegOut = SegOutT<Fe>;

}  // namespace msm
