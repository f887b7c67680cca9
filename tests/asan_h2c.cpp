// asan_h2c.cpp -- a stand-alone program (its own main, no Python) that drives the host code of csrc/h2c.hpp -- the offset checks, the
// create-time DST code and, through the ht_h2c_* entry points, the functions the kernels wrap -- with heap buffers of exactly the
// sizes the calls promise, to be compiled with -fsanitize=address,undefined and run as it is:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o asan_h2c tests/asan_h2c.cpp && ./asan_h2c
// Exit code 0 and "ok" on success.
#include "../2022-entries_amd/csrc/host_test_api.cpp"

#include <cstdlib>
#include <string>
#include <vector>

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "asan_h2c: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  // offsets: exactly n + 1 entries on the heap
  {
    std::vector<uint64_t> off = {0, 3, 3, 10};
    REQUIRE(h2c_check_offsets(off.data(), 3, 10) == nullptr);
    REQUIRE(h2c_check_offsets(off.data(), 3, 9) != nullptr);
    off[1] = 4;
    off[2] = 2;
    REQUIRE(h2c_check_offsets(off.data(), 3, 10) != nullptr);
    std::vector<uint64_t> none = {0};
    REQUIRE(h2c_check_offsets(none.data(), 0, 0) == nullptr);
    REQUIRE(h2c_check_offsets(nullptr, 0, 0) != nullptr);
    std::vector<uint64_t> huge = {0, (uint64_t)1 << 28};
    REQUIRE(h2c_check_offsets(huge.data(), 1, (size_t)1 << 30) != nullptr);
  }
  // DST_prime for tags of 1, 255, 256 and 1000 bytes: at most 256 bytes written
  for (size_t len : {(size_t)1, (size_t)255, (size_t)256, (size_t)1000}) {
    std::vector<uint8_t> dst(len, 0x5a), prime(len > 255 ? 33 : len + 1);
    std::vector<uint32_t> z(8);
    uint8_t wide[256];
    uint32_t plen = 0, zp[8];
    h2c_make_dst(wide, plen, zp, dst.data(), len);
    REQUIRE(plen == prime.size());
    REQUIRE(ht_h2c_dst(dst.data(), len, wide, z.data()) == (int)plen);
    REQUIRE(memcmp(z.data(), zp, 32) == 0 && wide[plen - 1] == plen - 1);
  }
  // SHA-256 of "abc" from a three-byte heap buffer
  {
    std::vector<uint8_t> abc = {'a', 'b', 'c'}, out(32);
    REQUIRE(ht_h2c_sha256(abc.data(), 3, out.data()) == 0);
    REQUIRE(out[0] == 0xba && out[1] == 0x78 && out[31] == 0xad);
  }
  // field, map and hash of both groups on messages that fill their buffer to the last byte
  for (int group = 0; group < 2; group++) {
    const size_t m = group ? 2 : 1, stride = group ? 200 : 104;
    std::vector<uint8_t> dst(43, 'D'), data;
    std::vector<uint64_t> off = {0};
    for (size_t len : {(size_t)0, (size_t)5, (size_t)55, (size_t)64, (size_t)130}) {
      data.insert(data.end(), len, (uint8_t)(len + 1));
      off.push_back(data.size());
    }
    const size_t n = off.size() - 1;
    std::vector<uint8_t> u(n * 2 * m * 48), pts(n * stride), one(n * m * 48);
    REQUIRE(ht_h2c_field(group, dst.data(), dst.size(), data.data(), data.size(), off.data(), n, 2, u.data()) == 0);
    REQUIRE(ht_h2c_field(group, dst.data(), dst.size(), data.data(), data.size(), off.data(), n, 1, one.data()) == 0);
    REQUIRE(ht_h2c_map(group, u.data(), 2 * n, 4, pts.data(), stride) == 0);
    std::vector<uint8_t> raw(2 * n * stride), cleared(n * stride);
    REQUIRE(ht_h2c_map(group, u.data(), 2 * n, 0, raw.data(), stride) == 0);
    REQUIRE(ht_h2c_map(group, one.data(), n, 1, cleared.data(), stride) == 0);
    REQUIRE(ht_h2c_map(group, u.data(), 3, 4, pts.data(), stride) == -1);
    off[2] = data.size() + 1;
    REQUIRE(ht_h2c_field(group, dst.data(), dst.size(), data.data(), data.size(), off.data(), n, 2, u.data()) == -1);
    // clearing: the fast chain and plain double-and-add agree on a point off the subgroup
    std::vector<uint8_t> a(stride), b(stride), k = {0x01, 0x00, 0x01, 0x00, 0x00, 0x00, 0x01, 0xd2};
    if (group == 0) {
      REQUIRE(ht_h2c_clear(group, 0, raw.data(), stride, 1, nullptr, 0, a.data(), stride) == 0);
      REQUIRE(ht_h2c_clear(group, 1, raw.data(), stride, 1, k.data(), k.size(), b.data(), stride) == 0);
      REQUIRE(memcmp(a.data(), b.data(), stride) == 0);
    } else {
      REQUIRE(ht_h2c_clear(group, 0, raw.data(), stride, 2, nullptr, 0, pts.data(), stride) == 0);
    }
  }
  if (ht_check_failures() != 0) {
    fprintf(stderr, "asan_h2c: the limb-bound checker fired: %s\n", ht_first_failure());
    return 1;
  }
  puts("ok");
  return 0;
}
