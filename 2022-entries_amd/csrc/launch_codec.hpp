// launch_codec.hpp -- host-callable launchers of the point-codec kernels (point_codec.hpp).  Declared here, defined and instantiated
// for the four curves in kernels_codec.hip; the only other unit that includes it is the engine (msm_codec.hpp).
#pragma once
#include "launch.hpp"

namespace msm {

template <class E>
struct LaunchCodec {
  // n compressed records -> Affine images `stride` bytes apart, or uncompressed records (`serialized`); one status byte each
  // (0 decoded, 1 malformed, 2 no point has this x; bit 7: flagged infinity)
  static hipError_t decompress(const uint8_t* in, uint32_t n, uint8_t* out, size_t stride, bool serialized, uint8_t* status, hipStream_t st);
  // n Affine images `stride` bytes apart, or uncompressed records (`serialized`) -> compressed records; status 0 / 1 (bit 7 as above)
  static hipError_t compress(const uint8_t* in, size_t stride, uint32_t n, bool serialized, uint8_t* out, uint8_t* status, hipStream_t st);
};

extern template struct LaunchCodec<Bls12_377_G1::E>;
extern template struct LaunchCodec<Bls12_381_G1::E>;
extern template struct LaunchCodec<Bls12_377_G2::E>;
extern template struct LaunchCodec<Bls12_381_G2::E>;

}  // namespace msm
