// asan_segments.cpp -- a stand-alone program (its own main, no Python) that drives the host build of csrc/seg_msm.hpp -- the launch plan
// and the serial walk through the kernels' per-element steps -- with heap buffers of exactly the sizes the call promises (the last
// image ends at its flag byte, 32 bytes a scalar, nsegments + 1 offsets), to be compiled with -fsanitize=address,undefined and run as
// it is:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I 2022-entries_amd/csrc -o asan_segments tests/asan_segments.cpp
// The offsets are adversarial: all segments empty, everything in the last segment, empty segments between long ones, lengths at the
// tile edges.  The records are random bytes -- on no curve, so the sums are unspecified, but every access must stay inside the
// buffers -- or flagged infinities and zero scalars, whose sums must come out as the point at infinity.  Exit code 0 and "ok".
#include "../2022-entries_amd/csrc/host_test_api.cpp"

#include <cstdlib>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint8_t next_byte() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (uint8_t)(g_state >> 24);
}
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "asan_segments: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool is_infinity_image(const uint8_t* img, size_t cb) {
  for (size_t k = 0; k < 2 * cb; k++)
    if (img[k]) return false;
  return img[2 * cb] == 1;
}

static int run_case(int curve, const std::vector<uint64_t>& offsets, int c, int tile, int mode) {
  const size_t cb = curve < 2 ? 48 : 96, stride = 2 * cb + 8, nseg = offsets.size() - 1, n = offsets.back();
  // exactly what the call may read: the last image ends behind its flag byte
  std::vector<uint8_t> points(n ? (n - 1) * stride + 2 * cb + 1 : 0), scalars(32 * n), out(nseg * stride, 0xa5);
  for (auto& b : points) b = mode == 1 ? 0 : (uint8_t)(next_byte() & 0x0f);   // (small bytes: coordinates below p)
  for (size_t i = 0; i < n; i++) points[i * stride + 2 * cb] = mode == 1 ? 1 : (uint8_t)(i % 5 == 0);
  for (auto& b : scalars) b = mode == 2 ? 0 : next_byte();
  std::vector<uint64_t> offs(offsets);   // a heap copy of nseg + 1 values
  REQUIRE(ht_sm_segments(curve, points.data(), stride, scalars.data(), offs.data(), nseg, 0, c, tile, 0, out.data(), stride) == 0);
  if (mode)
    for (size_t s = 0; s < nseg; s++) REQUIRE(is_infinity_image(out.data() + s * stride, cb));
  for (size_t s = 0; s < nseg; s++)
    if (offsets[s] == offsets[s + 1]) REQUIRE(is_infinity_image(out.data() + s * stride, cb));
  // the plan over the same offsets, into arrays of exactly the size it may fill
  std::vector<uint64_t> classes(11 * 9 * (nseg + 1)), bounds(3 * (nseg + 1)), summary(3);
  std::vector<uint32_t> ids(nseg + 1);
  for (size_t limit : {(size_t)2 << 30, (size_t)300000}) {
    const long nc = ht_sm_plan(offs.data(), nseg, 0, c, tile, nseg % 3, limit, curve < 2 ? 224 : 448, curve < 2 ? 56 : 112, classes.data(), 9 * (nseg + 1),
                               ids.data(), nseg + 1, bounds.data(), nseg + 1, summary.data());
    REQUIRE(nc >= 0);
    size_t covered = 0;
    for (long k = 0; k < nc; k++) {
      const uint64_t* r = classes.data() + 11 * k;
      REQUIRE(r[7] + r[6] <= nseg + 1 && r[8] + r[4] * r[6] <= r[10] && r[9] <= limit);
      for (uint64_t i = 0; i < r[6]; i++) REQUIRE(ids[r[7] + i] < r[2] - r[1]);
      covered += r[6];
    }
    size_t nonempty = 0;
    for (size_t s = 0; s < nseg; s++) nonempty += offsets[s + 1] > offsets[s];
    REQUIRE(covered == nonempty);
  }
  return 0;
}

int main() {
  const std::vector<std::vector<uint64_t>> shapes = {
      {0},                                    // no segment at all
      {0, 0, 0, 0},                           // all empty
      {0, 0, 0, 0, 70},                       // everything in the last segment
      {0, 70, 70, 70, 70},                    // everything in the first
      {0, 1, 1, 2, 65, 65, 129, 129},         // empty segments between the tile edges 1, 63 + 1, 64
      {0, 63, 127, 192, 193},
      {0, 129},
  };
  for (const auto& offsets : shapes)
    for (int curve : {0, 3})
      for (int c : {0, 1, 7, 9})
        for (int mode = 0; mode < 3; mode++) {
          if (mode && c) continue;                 // (the infinity cases once per shape, at the automatic window)
          if (curve == 3 && c == 9) continue;      // (minutes under the sanitizer and nothing the Fp case does not touch)
          if (run_case(curve, offsets, c, c == 7 ? 128 : 64, mode)) return 1;
        }
  // what the entry refuses
  uint8_t one[200] = {0};
  uint64_t offs[2] = {0, 0};
  REQUIRE(ht_sm_segments(0, one, 104, one, offs, 1, 0, 10, 64, 0, one, 104) == -1);   // window size
  REQUIRE(ht_sm_segments(0, one, 104, one, offs, 1, 0, 4, 96, 0, one, 104) == -1);    // tile not a power of two
  REQUIRE(ht_sm_segments(0, one, 104, one, offs, 1, 0, 4, 64, 4, one, 104) == -1);    // the shared form with offsets
  REQUIRE(ht_sm_segments(7, one, 104, one, offs, 1, 0, 4, 64, 0, one, 104) == -1);    // curve id
  printf("ok\n");
  return 0;
}
