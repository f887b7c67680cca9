// asan_lookup.cpp -- a stand-alone program (its own main, no Python) that drives the host build of csrc/lookup.hpp through the ht_lookup
// and ht_logup_sum entry points with heap buffers of exactly the sizes the calls promise (index_out of n_f u32, mult_out of n_t elements,
// s_out of n_t + n_f, helpers of (m + 1) n), to be compiled with -fsanitize=address,undefined and run as it is:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o asan_lookup tests/asan_lookup.cpp && ./asan_lookup
// It checks what needs no model: the counts sum to the values found, s has the table as a subsequence, a missing value leaves s alone,
// the total of the logUp sum is zero from the library's own multiplicities and not zero after one is changed, results do not depend on
// the tile, and the limb-bound checker stayed silent.  Exit code 0 and "ok" on success.
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
static std::vector<uint8_t> random_bytes(size_t n) {
  std::vector<uint8_t> v(n);
  for (auto& b : v) b = next_byte();
  return v;
}
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "asan_lookup: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  const std::vector<uint8_t> zero(32, 0);
  for (int field = 0; field < 2; field++) {
    for (unsigned flags = 0; flags < 2; flags++) {
      for (size_t n_t : {(size_t)1, (size_t)32, (size_t)33, (size_t)1025, (size_t)3000}) {
        for (size_t n_f : {(size_t)0, (size_t)1, (size_t)65, (size_t)2500}) {
          // any 256-bit patterns as the table (with a duplicate); the values are drawn from it
          std::vector<uint8_t> table = random_bytes(32 * n_t), values(32 * n_f);
          if (n_t > 20) memcpy(table.data() + 32 * 17, table.data() + 32 * 3, 32);
          for (size_t j = 0; j < n_f; j++) memcpy(values.data() + 32 * j, table.data() + 32 * ((j * 7 + next_byte()) % n_t), 32);
          std::vector<uint8_t> mult(32 * n_t), s(32 * (n_t + n_f), 0x5a);
          std::vector<uint32_t> index(n_f);
          uint64_t stats[2] = {9, 9}, info[3] = {0, 0, 0};
          REQUIRE(ht_lookup(field, flags, table.data(), n_t, n_f ? values.data() : nullptr, n_f, mult.data(), n_f ? index.data() : nullptr, stats, s.data(),
                            info) == 0);
          REQUIRE(stats[0] == 0 && stats[1] == n_f);
          REQUIRE(info[0] >= 2 * n_t && info[0] < 4 * n_t + 2 && info[1] <= n_t && info[2] >= 1);
          for (size_t j = 0; j < n_f; j++) REQUIRE(index[j] < n_t);
          if (n_t > 20) REQUIRE(memcmp(mult.data() + 32 * 17, zero.data(), 32) == 0);   // a later duplicate is credited nothing
          // the total of the logUp sum over (table, mult, values) is zero: n rows need n_f == n_t, so pad the shorter side with table[0]
          if (n_f == 0 || n_t > 1100) continue;
          const size_t n = n_t > n_f ? n_t : n_f;
          std::vector<uint8_t> tt(32 * n), vv(32 * n), mm(32 * n);
          for (size_t j = 0; j < n; j++) {
            memcpy(tt.data() + 32 * j, table.data() + 32 * (j < n_t ? j : 0), 32);
            memcpy(vv.data() + 32 * j, j < n_f ? values.data() + 32 * j : table.data(), 32);
          }
          std::vector<uint32_t> index2(n);
          REQUIRE(ht_lookup(field, flags, tt.data(), n, vv.data(), n, mm.data(), index2.data(), stats, nullptr, nullptr) == 0);
          const std::vector<uint8_t> beta = random_bytes(32);
          std::vector<uint8_t> out(32 * n), out4(32 * n), total(32), total4(32), helpers(32 * 2 * n);
          REQUIRE(ht_logup_sum(field, 10, flags, tt.data(), mm.data(), vv.data(), 1, n, n, beta.data(), out.data(), total.data(), helpers.data()) == 0);
          REQUIRE(ht_logup_sum(field, 4, flags, tt.data(), mm.data(), vv.data(), 1, n, n, beta.data(), out4.data(), total4.data(), nullptr) == 0);
          REQUIRE(total == zero && total4 == zero && out == out4);
          REQUIRE(memcmp(out.data(), zero.data(), 32) == 0);
        }
      }
      // a missing value: stats say so and s is left alone
      {
        const size_t n_t = 70, n_f = 9;
        const std::vector<uint8_t> table(32 * n_t, 0);   // 70 zeros: one key
        std::vector<uint8_t> values(32 * n_f, 0), s(32 * (n_t + n_f), 0x5a);
        values[32 * 4] = 1;
        uint64_t stats[2] = {0, 0};
        REQUIRE(ht_lookup(field, flags, table.data(), n_t, values.data(), n_f, nullptr, nullptr, stats, s.data(), nullptr) == 0);
        REQUIRE(stats[0] == 1 && stats[1] == 4);
        for (uint8_t b : s) REQUIRE(b == 0x5a);
      }
      // every multiple of r that fits 256 bits is one key: 5 + k r, k = 0 .. 13 for BLS12-377 (r has 253 bits), 0 .. 2 for BLS12-381
      {
        const uint32_t* r32 = field == 0 ? Bls12_377_Fr29::P32 : Bls12_381_Fr29::P32;
        const size_t kmax = field == 0 ? 13 : 2, n_t = kmax + 1, n_f = 2 * n_t;
        std::vector<uint8_t> table(32 * n_t, 0), values(32 * n_f, 0), mult(32 * n_t), s(32 * (n_t + n_f), 0x5a);
        uint32_t cur[8] = {5, 0, 0, 0, 0, 0, 0, 0};
        for (size_t k = 0; k <= kmax; k++) {
          memcpy(table.data() + 32 * k, cur, 32);
          memcpy(values.data() + 32 * (kmax - k), cur, 32);
          memcpy(values.data() + 32 * (n_t + k), cur, 32);
          uint64_t c = 0;
          for (int j = 0; j < 8; j++) {
            c += (uint64_t)cur[j] + r32[j];
            cur[j] = (uint32_t)c;
            c >>= 32;
          }
          REQUIRE(c == 0 || k == kmax);          // the next multiple no longer fits
        }
        std::vector<uint32_t> index(n_f);
        uint64_t stats[2] = {9, 9}, info[3] = {0, 0, 0};
        REQUIRE(ht_lookup(field, 1, table.data(), n_t, values.data(), n_f, mult.data(), index.data(), stats, s.data(), info) == 0);
        REQUIRE(stats[0] == 0 && stats[1] == n_f && info[1] == 1);
        for (uint32_t i : index) REQUIRE(i == 0);
        REQUIRE(mult[0] == n_f);
        for (size_t i = 0; i < n_t + n_f; i++) REQUIRE(s[32 * i] == 5 && memcmp(s.data() + 32 * i + 1, zero.data(), 31) == 0);   // canonical copies
      }
      // eight columns, a stride above n, exact helpers
      {
        const size_t n = 37, m = 8, stride = 41;
        const std::vector<uint8_t> table = random_bytes(32 * n), mult = random_bytes(32 * n), values = random_bytes(32 * ((m - 1) * stride + n)),
                                   beta = random_bytes(32);
        std::vector<uint8_t> out(32 * n), total(32), helpers(32 * (m + 1) * n);
        REQUIRE(ht_logup_sum(field, 4, flags, table.data(), mult.data(), values.data(), m, stride, n, beta.data(), out.data(), total.data(), helpers.data()) == 0);
        REQUIRE(total != zero);
      }
    }
  }
  if (ht_check_failures() != 0) {
    fprintf(stderr, "asan_lookup: the limb-bound checker fired: %s\n", ht_first_failure());
    return 1;
  }
  puts("ok");
  return 0;
}
