// asan_expr.cpp -- a stand-alone program (its own main, no Python) that drives the host build of csrc/expr.hpp through the ht_expr entry
// point with heap buffers of exactly the sizes the call promises (3 u32 per node, lens[j] elements per column, n_chal challenges, len
// outputs), to be compiled with -fsanitize=address,undefined and run as it is:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o asan_expr tests/asan_expr.cpp && ./asan_expr
// It checks what needs no model: polynomial identities that must evaluate to zero whatever the inputs ((a + b)^2 - a^2 - 2ab - b^2 with
// rotations and periodic columns, x - x after a doubling chain), two programs for one value (64 doublings against a product by 2^64),
// what create refuses (a forward reference, one slot too many) and that the limb-bound checker stayed silent.  Exit code 0 and "ok".
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
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "asan_expr: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Dag {
  std::vector<uint32_t> w;
  uint32_t add(uint32_t op, uint32_t a, uint32_t b = 0) {
    w.push_back(op);
    w.push_back(a);
    w.push_back(b);
    return (uint32_t)(w.size() / 3 - 1);
  }
  uint64_t n() const { return w.size() / 3; }
};

int main() {
  char msg[256];
  const std::vector<uint8_t> zero(32, 0);
  for (int field = 0; field < 2; field++) {
    for (unsigned flags = 0; flags < 2; flags++) {
      for (uint64_t len : {(uint64_t)1, (uint64_t)2, (uint64_t)63, (uint64_t)64, (uint64_t)130}) {
        // (a + b)^2 - a^2 - 2ab - b^2 with a = col0 at rotation +1, b = col1 (periodic: length 1 or 2) at rotation -3
        const uint64_t lb = len % 2 ? 1 : 2;
        Dag g;
        const uint32_t a = g.add(EXPR_COL, 0, 1), b = g.add(EXPR_COL, 1, (uint32_t)-3), s = g.add(EXPR_ADD, a, b), s2 = g.add(EXPR_SQR, s);
        const uint32_t a2 = g.add(EXPR_SQR, a), b2 = g.add(EXPR_MUL, b, b), ab = g.add(EXPR_MUL, a, b), ab2 = g.add(EXPR_ADD, ab, ab);
        const uint32_t t1 = g.add(EXPR_SUB, s2, a2), t2 = g.add(EXPR_SUB, t1, ab2);
        g.add(EXPR_SUB, t2, b2);
        std::vector<uint8_t> c0 = random_bytes(32 * len), c1 = random_bytes(32 * lb), out(32 * len, 0x5a);
        const uint8_t* cols[2] = {c0.data(), c1.data()};
        const uint64_t lens[2] = {len, lb};
        uint64_t info[8];
        REQUIRE(ht_expr(field, flags, g.w.data(), g.n(), nullptr, 0, 0, 2, cols, lens, len, 8, nullptr, out.data(), info, msg, sizeof msg) == 0);
        for (uint64_t i = 0; i < len; i++) REQUIRE(memcmp(out.data() + 32 * i, zero.data(), 32) == 0);
        REQUIRE(info[2] >= 1 && info[2] <= 8 && info[5] == info[2] * 8 * 4 * 64);
      }
      // 64 doublings of col0 against col0 * chal0 with chal0 = 2^64, and x - x behind them
      {
        const uint64_t len = 65;
        Dag g;
        uint32_t x = g.add(EXPR_COL, 0, 0);
        for (int k = 0; k < 64; k++) x = g.add(EXPR_ADD, x, x);
        const uint32_t c = g.add(EXPR_COL, 0, 0), h = g.add(EXPR_CHAL, 0), p = g.add(EXPR_MUL, c, h);
        g.add(EXPR_SUB, x, p);
        std::vector<uint8_t> c0 = random_bytes(32 * len), out(32 * len, 0x5a), chal(32, 0);
        chal[8] = 1;   // 2^64 as a plain integer
        const uint8_t* cols[1] = {c0.data()};
        const uint64_t lens[1] = {len};
        uint64_t info[8];
        REQUIRE(ht_expr(field, 1, g.w.data(), g.n(), nullptr, 0, 1, 1, cols, lens, len, 1, chal.data(), out.data(), info, msg, sizeof msg) == 0);
        for (uint64_t i = 0; i < len; i++) REQUIRE(memcmp(out.data() + 32 * i, zero.data(), 32) == 0);
        REQUIRE(info[4] > 0);   // the doubling chain forced reductions
      }
    }
    // what create refuses: a forward reference; one slot more than the kernel has (k products that all stay live)
    {
      Dag g;
      g.add(EXPR_COL, 0, 0);
      g.add(EXPR_ADD, 0, 1);
      REQUIRE(ht_expr(field, 0, g.w.data(), g.n(), nullptr, 0, 0, 1, nullptr, nullptr, 0, 1, nullptr, nullptr, nullptr, msg, sizeof msg) == -1);
      REQUIRE(strstr(msg, "topological"));
    }
    for (uint32_t k : {EXPR_MAX_SLOTS - 1, EXPR_MAX_SLOTS}) {
      Dag g;
      std::vector<uint32_t> p;
      const uint32_t c0 = g.add(EXPR_COL, 0, 0);
      for (uint32_t j = 0; j < k; j++) p.push_back(g.add(EXPR_ADD, g.add(EXPR_MUL, g.add(EXPR_COL, 0, j), g.add(EXPR_COL, 0, j + 1)), c0));
      uint32_t s = p[0], t = p[0];
      for (uint32_t j = 1; j < k; j++) s = g.add(EXPR_ADD, s, p[j]);
      for (uint32_t j = 1; j < k; j++) t = g.add(EXPR_MUL, t, p[j]);
      g.add(EXPR_SUB, s, t);
      uint64_t info[8];
      const int rc = ht_expr(field, 0, g.w.data(), g.n(), nullptr, 0, 0, 1, nullptr, nullptr, 0, 1, nullptr, nullptr, info, msg, sizeof msg);
      REQUIRE(info[2] == k + 1);
      REQUIRE(rc == (k + 1 <= EXPR_MAX_SLOTS ? 0 : -1));
      if (rc) REQUIRE(strstr(msg, "S = 33") && strstr(msg, "limit is 32"));
    }
  }
  REQUIRE(ht_check_failures() == 0);
  printf("ok\n");
  return 0;
}
