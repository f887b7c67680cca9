// mi355_msm_segments.hpp -- header-only C++ wrapper of mi355_msm_segments (mi355_msm.h): many small MSMs in one call, on top of the
// context type of mi355_msm.hpp.  A header of its own, so that mi355_msm.hpp stays the mirror of the reference's operator API.
//
//   std::vector<G1Affine> sums = mi355::msm_segments(ctx, points, scalars, offsets);          // out[s] over [offsets[s], offsets[s+1])
//   std::vector<G1Affine> sums = mi355::msm_segments_shared(ctx, points, scalars, nsegments);  // every segment over all points
//
// Arguments are judged here first (std::invalid_argument), then by the library (MsmError).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "mi355_msm.hpp"

namespace mi355 {

constexpr unsigned SEGMENTS_MONTGOMERY = 1u, SEGMENTS_DEVICE = 2u, SEGMENTS_SHARED = 4u, SEGMENTS_PROJECTIVE = 8u;

// out[s] = sum over offsets[s] <= i < offsets[s + 1] of scalars[i] * points[i]; an empty segment gives the point at infinity.
// scalars: 32-byte little-endian integers, all 256 bits significant (`montgomery`: arkworks Fr images).  Any curve points: no curve
// test, no subgroup test.  Affine images out, ready for set_bases, fft_points and compress_points.
inline std::vector<G1Affine> msm_segments(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points, const std::vector<BigInteger256>& scalars,
                                          const std::vector<uint64_t>& offsets, bool montgomery = false) {
  if (offsets.empty()) throw std::invalid_argument("msm_segments: offsets hold one value more than there are segments");
  if (offsets.front() != 0) throw std::invalid_argument("msm_segments: offsets[0] must be 0");
  for (size_t s = 1; s < offsets.size(); s++)
    if (offsets[s] < offsets[s - 1]) throw std::invalid_argument("msm_segments: offsets[" + std::to_string(s) + "] is smaller than its predecessor");
  if (offsets.back() != points.size()) throw std::invalid_argument("msm_segments: the last offset must equal the number of points");
  if (scalars.size() != points.size()) throw std::invalid_argument("msm_segments: one scalar per point");
  const size_t nseg = offsets.size() - 1;
  std::vector<G1Affine> out(nseg);
  check(mi355_msm_segments(ctx.context, points.data(), points.size(), sizeof(G1Affine), scalars.data(), scalars.size(), offsets.data(), nseg,
                           montgomery ? SEGMENTS_MONTGOMERY : 0u, out.data(), sizeof(G1Affine), nullptr));
  return out;
}

// The shared form: scalars holds nsegments rows of points.size() values; out[s] = sum_i scalars[s * points.size() + i] * points[i].
inline std::vector<G1Affine> msm_segments_shared(MultiScalarMultContext& ctx, const std::vector<G1Affine>& points, const std::vector<BigInteger256>& scalars,
                                                 size_t nsegments, bool montgomery = false) {
  if (scalars.size() != nsegments * points.size()) throw std::invalid_argument("msm_segments_shared: nsegments rows of one scalar per point");
  std::vector<G1Affine> out(nsegments);
  check(mi355_msm_segments(ctx.context, points.data(), points.size(), sizeof(G1Affine), scalars.data(), scalars.size(), nullptr, nsegments,
                           SEGMENTS_SHARED | (montgomery ? SEGMENTS_MONTGOMERY : 0u), out.data(), sizeof(G1Affine), nullptr));
  return out;
}

// Device pointers: images `stride` / `out_stride` bytes apart in device memory, ready on `stream` (a hipStream_t; nullptr = the default
// stream); `offsets` stays host memory.  `flags`: SEGMENTS_MONTGOMERY, SEGMENTS_SHARED (offsets empty), SEGMENTS_PROJECTIVE.
inline void msm_segments_on_stream(MultiScalarMultContext& ctx, const void* d_points, size_t npoints, size_t stride, const void* d_scalars, size_t nscalars,
                                const std::vector<uint64_t>& offsets, size_t nsegments, unsigned flags, void* d_out, size_t out_stride, void* stream) {
  if (flags & SEGMENTS_SHARED) {
    if (!offsets.empty()) throw std::invalid_argument("msm_segments_on_stream: the shared form takes no offsets");
  } else if (offsets.size() != nsegments + 1) {
    throw std::invalid_argument("msm_segments_on_stream: offsets hold nsegments + 1 values");
  }
  check(mi355_msm_segments(ctx.context, d_points, npoints, stride, d_scalars, nscalars, offsets.empty() ? nullptr : offsets.data(), nsegments,
                           flags | SEGMENTS_DEVICE, d_out, out_stride, stream));
}

}  // namespace mi355
