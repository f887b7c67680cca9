// asan_mle.cpp -- a stand-alone program (its own main, no Python) that drives the host build of csrc/mle.hpp through the ht_mle_* entry
// points with heap buffers of exactly the sizes the calls promise, to be compiled with -fsanitize=address,undefined and run as it is:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o asan_mle tests/asan_mle.cpp && ./asan_mle
// It checks what needs no model: evaluate == fix_variables down to one element in one, two and three passes, eq sums to one, the fused
// round's folded tables are fix_variables with one value and its evaluations are the plain round's on them, results do not depend on
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
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "asan_mle: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  for (int field = 0; field < 2; field++) {
    for (unsigned flags = 0; flags < 2; flags++) {
      // fix_variables: nv = 10 with tiles of 16 runs three passes and the ping-pong; tiles of 1024 one pass
      const unsigned nv = 10;
      const std::vector<uint8_t> table = random_bytes((size_t)32 << nv), point = random_bytes(32 * nv);
      std::vector<uint8_t> a(32), b(32), step((size_t)32 << (nv - 3)), c(32);
      REQUIRE(ht_mle_fix(field, 4, flags, nv, nv, table.data(), point.data(), a.data()) == 0);
      REQUIRE(ht_mle_fix(field, 10, flags, nv, nv, table.data(), point.data(), b.data()) == 0);
      REQUIRE(a == b);
      REQUIRE(ht_mle_fix(field, 4, flags, nv, 3, table.data(), point.data(), step.data()) == 0);
      REQUIRE(ht_mle_fix(field, 7, flags, nv - 3, nv - 3, step.data(), point.data() + 32 * 3, c.data()) == 0);
      REQUIRE(a == c);
      std::vector<uint8_t> copy((size_t)32 << 5);
      REQUIRE(ht_mle_fix(field, 4, flags, 5, 0, table.data(), nullptr, copy.data()) == 0);
      // eq: evaluate(eq(p), q) is symmetric
      for (unsigned k : {0u, 1u, 6u, 7u}) {
        std::vector<uint8_t> e1((size_t)32 << k), e2((size_t)32 << k), v1(32), v2(32);
        REQUIRE(ht_mle_eq(field, flags, k, point.data(), e1.data()) == 0);
        REQUIRE(ht_mle_eq(field, flags, k, point.data() + 32, e2.data()) == 0);
        REQUIRE(ht_mle_fix(field, 4, flags, k, k, e1.data(), point.data() + 32, v1.data()) == 0);
        REQUIRE(ht_mle_fix(field, 4, flags, k, k, e2.data(), point.data(), v2.data()) == 0);
        REQUIRE(v1 == v2);
      }
      // a round: 8 terms of 5 factors over 12 tables, one a fifth power; fused against fix_variables and the plain round
      const unsigned m = 12, rnv = 7, n_terms = 8;
      const std::vector<uint8_t> tabs = random_bytes((size_t)m * (32 << rnv)), coeffs = random_bytes(32 * n_terms), r_prev = random_bytes(32);
      std::vector<uint32_t> nfs(n_terms, 5), factors(n_terms * 5);
      for (unsigned j = 0; j < n_terms; j++)
        for (unsigned q = 0; q < 5; q++) factors[j * 5 + q] = j == 0 ? 0 : (3 * j + q) % m;
      std::vector<uint8_t> folded((size_t)m * (32 << (rnv - 1))), ev_fused(32 * 6), ev_plain(32 * 6), ev_tile(32 * 6), one((size_t)32 << (rnv - 1));
      REQUIRE(ht_mle_round(field, 4, flags, m, rnv, tabs.data(), n_terms, coeffs.data(), nfs.data(), factors.data(), r_prev.data(), folded.data(), ev_fused.data()) == 2);
      REQUIRE(ht_mle_round(field, 4, flags, m, rnv - 1, folded.data(), n_terms, coeffs.data(), nfs.data(), factors.data(), nullptr, nullptr, ev_plain.data()) == 2);
      REQUIRE(ht_mle_round(field, 10, flags, m, rnv - 1, folded.data(), n_terms, coeffs.data(), nfs.data(), factors.data(), nullptr, nullptr, ev_tile.data()) == 1);
      REQUIRE(ev_fused == ev_plain && ev_plain == ev_tile);
      for (unsigned i = 0; i < m; i++) {
        REQUIRE(ht_mle_fix(field, 4, flags, rnv, 1, tabs.data() + (size_t)i * (32 << rnv), r_prev.data(), one.data()) == 0);
        REQUIRE(memcmp(one.data(), folded.data() + (size_t)i * (32 << (rnv - 1)), one.size()) == 0);
      }
    }
  }
  if (ht_check_failures() != 0) {
    fprintf(stderr, "asan_mle: the limb-bound checker fired: %s\n", ht_first_failure());
    return 1;
  }
  puts("ok");
  return 0;
}
