// digits.hpp -- scalar-side helpers of the windowing (curve-independent apart from the scalar field constants); the digit
// extraction itself is fused into the first level of the bucket grouping (partition.hpp::next_digit).
// Reference behaviour: SPK msm/pippenger.cuh:116-123 (get_wval), CMB ProcessSignedDigits.cu:118-151 (signed digits).
#pragma once
#include "fp28.hpp"

namespace msm {

// Fr Montgomery form (a * 2^256 mod r, what arkworks' `Fr` holds) -> the plain integer a: one Montgomery reduction
// over 8 x 32-bit limbs.  This is `into_bigint` of VariableBaseMSM::msm (ARK ec/src/msm/variable_base/mod.rs:48-53,
// ff montgomery_backend.rs:445-465) and sppark's `mont` flag (SPK msm/pippenger.cuh:157-164).
// Defined for ANY 256-bit input: the reduction leaves (s + m r) / 2^256 <= r, and the one subtraction maps r to 0.
template <class FR>
MSM_HD void fr_from_montgomery(uint32_t (&s)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t m = s[0] * FR::RINV;
    uint64_t c = ((uint64_t)m * FR::R[0] + s[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      c += (uint64_t)m * FR::R[j] + s[j];
      s[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    s[7] = (uint32_t)c;
  }
  // result <= r; bring it below r
  uint32_t t[8];
  int64_t b = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    b += (int64_t)s[j] - FR::R[j];
    t[j] = (uint32_t)b;
    b >>= 32;
  }
  if (b == 0) {
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = t[j];
  }
}

// The mirror image: the plain integer a (what `scalars.bin` holds, arkworks' `into_bigint`) -> a * 2^256 mod r (the `Fr` limbs the
// ZPrize harness hands to the MSM), as ONE Montgomery product a * R2 * 2^-256 with R2 = 2^512 mod r, 8 x 32-bit CIOS.  Defined for
// ANY 256-bit a: with R2 < r every step keeps t < r + R2 < 2r < 2^256 (r < 2^255 for both scalar fields), so one subtraction ends it.
template <class FR>
MSM_HD void fr_to_montgomery(uint32_t (&s)[8]) {
  uint32_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t a = s[i];
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      c += (uint64_t)a * FR::R2[j] + t[j];
      t[j] = (uint32_t)c;
      c >>= 32;
    }
    const uint32_t top = (uint32_t)c;   // t + a R2 < 2^288: one word above t
    const uint32_t m = t[0] * FR::RINV;
    c = ((uint64_t)m * FR::R[0] + t[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      c += (uint64_t)m * FR::R[j] + t[j];
      t[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    t[7] = (uint32_t)c + top;   // (t + a R2 + m r) / 2^32 < r + R2: nothing above 2^256
  }
  // t < 2r: subtract r where t >= r (the borrow is found first, so no second copy of t is needed -- the caller holds a tile of
  // scalars in registers)
  int64_t b = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    b += (int64_t)t[j] - FR::R[j];
    b >>= 32;
  }
  const uint32_t keep = b ? 0u : 0xffffffffu;   // 0: t < r
  b = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    b += (int64_t)t[j] - (FR::R[j] & keep);
    s[j] = (uint32_t)b;
    b >>= 32;
  }
}

}  // namespace msm
