// asan_pairing.cpp -- a stand-alone program (its own main, no Python) that drives the host build of csrc/pairing.hpp through the
// ht_pairing_* entry points with heap buffers of exactly the sizes the calls promise, to be compiled with -fsanitize=address,undefined
// and run as it is:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o asan_pairing tests/asan_pairing.cpp
//   ./asan_pairing tests/golden/pairing
// It checks golden cases of both families in both output forms, batches and groups (the serial walk and the product tree), the
// check bytes of (P, Q), (-P, Q), and that the limb-bound checker stayed silent.  Exit code 0 and "ok" on success.
#include "../2022-entries_amd/csrc/host_test_api.cpp"

#include <cstdlib>
#include <string>
#include <vector>

#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "asan_pairing: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool read_file(const std::string& path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize((size_t)n);
  const bool ok = fread(out.data(), 1, out.size(), f) == out.size();
  fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "tests/golden/pairing";
  const char* names[2] = {"bls12_377.bin", "bls12_381.bin"};
  for (int family = 0; family < 2; family++) {
    std::vector<uint8_t> raw;
    REQUIRE(read_file(dir + "/" + names[family], raw));
    REQUIRE(raw.size() > 16 && memcmp(raw.data(), "PAIRGOLD", 8) == 0);
    uint32_t n;
    memcpy(&n, raw.data() + 8, 4);
    const size_t rec = 104 + 200 + 576 + 576;
    REQUIRE(raw.size() == 16 + n * rec && n >= 18);
    std::vector<uint8_t> g1(n * 104), g2(n * 200), em(n * 576), ec(n * 576);
    for (uint32_t i = 0; i < n; i++) {
      const uint8_t* at = raw.data() + 16 + i * rec;
      memcpy(g1.data() + 104 * i, at, 104);
      memcpy(g2.data() + 200 * i, at + 104, 200);
      memcpy(em.data() + 576 * i, at + 304, 576);
      memcpy(ec.data() + 576 * i, at + 880, 576);
    }
    // the first three cases in both forms, into buffers of the exact size
    const size_t m = 3;
    std::vector<uint8_t> out(m * 576);
    REQUIRE(ht_pairing_run(family, out.data(), g1.data(), 104, g2.data(), 200, m, 1, 0, 0) == 0);
    REQUIRE(memcmp(out.data(), em.data(), m * 576) == 0);
    REQUIRE(ht_pairing_run(family, out.data(), g1.data(), 104, g2.data(), 200, m, 1, 1, 0) == 0);
    REQUIRE(memcmp(out.data(), ec.data(), m * 576) == 0);
    // a flagged infinity with junk coordinates (the last but two) is one
    std::vector<uint8_t> junk(576);
    REQUIRE(ht_pairing_run(family, junk.data(), g1.data() + 104 * (n - 3), 104, g2.data() + 200 * (n - 3), 200, 1, 1, 1, 0) == 0);
    REQUIRE(memcmp(junk.data(), ec.data() + 576 * (n - 3), 576) == 0);
    // groups: 3 (one lane walks them) and 9 (the product tree, two levels), into buffers of the exact size
    for (size_t group : {(size_t)3, (size_t)9}) {
      std::vector<uint8_t> o(576), ok(1);
      REQUIRE(ht_pairing_run(family, o.data(), g1.data(), 104, g2.data(), 200, group, group, 1, 0) == 0);
      REQUIRE(ht_pairing_run(family, ok.data(), g1.data(), 104, g2.data(), 200, group, group, 0, 1) == 0);
      REQUIRE(ok[0] == 0);
    }
    // (P, Q), (-P, Q): cases 1 and 15
    std::vector<uint8_t> a(2 * 104), b(2 * 200), ok(1);
    memcpy(a.data(), g1.data() + 104 * 1, 104);
    memcpy(a.data() + 104, g1.data() + 104 * 15, 104);
    memcpy(b.data(), g2.data() + 200 * 1, 200);
    memcpy(b.data() + 200, g2.data() + 200 * 15, 200);
    REQUIRE(ht_pairing_run(family, ok.data(), a.data(), 104, b.data(), 200, 2, 2, 0, 1) == 0);
    REQUIRE(ok[0] == 1);
    memcpy(b.data() + 200, g2.data() + 200 * 2, 200);
    REQUIRE(ht_pairing_run(family, ok.data(), a.data(), 104, b.data(), 200, 2, 2, 0, 1) == 0);
    REQUIRE(ok[0] == 0);
    REQUIRE(ht_pairing_run(family, nullptr, nullptr, 104, nullptr, 200, 0, 1, 0, 0) == 0);
    REQUIRE(ht_pairing_run(family, ok.data(), a.data(), 100, b.data(), 200, 2, 2, 0, 1) == -1);
  }
  if (ht_check_failures() != 0) {
    fprintf(stderr, "asan_pairing: the limb-bound checker fired: %s\n", ht_first_failure());
    return 1;
  }
  puts("ok");
  return 0;
}
