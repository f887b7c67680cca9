// asan_poseidon.cpp -- a stand-alone program (its own main, no Python) that drives the host build of csrc/poseidon.hpp through the
// ht_poseidon_* entry points with heap buffers of exactly the sizes the calls promise, to be compiled with -fsanitize=address,undefined
// and run as it is:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o asan_poseidon tests/asan_poseidon.cpp && ./asan_poseidon
// It checks what needs no model: the sparse form gives the bytes of the dense one (a permutation, batches of sponges with and without a
// header, a Merkle tree), every node of a tree is the hash of its children under the node header and every padding leaf the empty hash,
// and the limb-bound checker stayed silent.  Exit code 0 and "ok" on success.
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
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "asan_poseidon: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
  for (int field = 0; field < 2; field++) {
    for (unsigned rate : {2u, 4u, 8u}) {
      for (unsigned flags = 0; flags < 2; flags++) {
        const unsigned t = rate + 1, alpha = flags ? 5 : 17, rf = flags ? 6 : 8, rp = flags ? 11 : 31;
        // any 256-bit values are residues: a random matrix has an invertible minor with overwhelming probability
        const std::vector<uint8_t> ark = random_bytes((size_t)32 * (rf + rp) * t), mds = random_bytes((size_t)32 * t * t);
        const std::vector<uint8_t> st = random_bytes(32 * t);
        std::vector<uint8_t> pd(32 * t), ps(32 * t);
        uint64_t info[4];
        REQUIRE(ht_poseidon_permute(field, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 0, st.data(), pd.data(), info) == 0);
        REQUIRE(ht_poseidon_permute(field, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 1, st.data(), ps.data(), info) == 0);
        REQUIRE(pd == ps);
        REQUIRE(info[1] < info[0]);
        const unsigned n = 3, in_len = 2 * rate + 1, n_out = rate + 1;
        const std::vector<uint8_t> in = random_bytes((size_t)32 * n * in_len), header = random_bytes(32 * rate);
        std::vector<uint8_t> od((size_t)32 * n * n_out), os((size_t)32 * n * n_out), oh((size_t)32 * n * n_out);
        REQUIRE(ht_poseidon_hash(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 0, n, in_len, n_out, nullptr, in.data(), od.data()) == 0);
        REQUIRE(ht_poseidon_hash(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 1, n, in_len, n_out, nullptr, in.data(), os.data()) == 0);
        REQUIRE(od == os);
        REQUIRE(ht_poseidon_hash(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 1, n, in_len, n_out, header.data(), in.data(), oh.data()) == 0);
        REQUIRE(oh != os);
        // nothing in, one out; something in, nothing out (no output pointer is touched)
        std::vector<uint8_t> one(32 * 2);
        REQUIRE(ht_poseidon_hash(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 1, 2, 0, 1, nullptr, nullptr, one.data()) == 0);
        REQUIRE(memcmp(one.data(), one.data() + 32, 32) == 0);
        REQUIRE(ht_poseidon_hash(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 1, n, in_len, 0, nullptr, in.data(), nullptr) == 0);
        // a tree of 5 leaves of 3 elements: P = 8, 15 nodes, three padding leaves
        const unsigned n_leaves = 5, leaf_len = 3, P = 8;
        const std::vector<uint8_t> leaves = random_bytes((size_t)32 * n_leaves * leaf_len), sep = random_bytes(32);
        std::vector<uint8_t> tree((size_t)32 * (2 * P - 1)), tree_d((size_t)32 * (2 * P - 1));
        REQUIRE(ht_poseidon_merkle(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 1, n_leaves, leaf_len, sep.data(), leaves.data(), tree.data()) == 0);
        REQUIRE(ht_poseidon_merkle(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 0, n_leaves, leaf_len, sep.data(), leaves.data(), tree_d.data()) == 0);
        REQUIRE(tree == tree_d);
        // with plain integers the header [domain, 3, 0 ..] and the leading 1 can be written down: every node is the hash of its children
        if (flags) {
          std::vector<uint8_t> hdr(32 * rate, 0), row(32 * 3, 0), node(32);
          memcpy(hdr.data(), sep.data(), 32);
          hdr[32] = 3;
          row[0] = 1;
          for (unsigned i = 0; i + 1 < P; i++) {
            memcpy(row.data() + 32, tree.data() + 32 * (2 * i + 1), 64);
            REQUIRE(ht_poseidon_hash(field, flags, flags, rate, alpha, rf, rp, ark.data(), mds.data(), 1, 1, 3, 1, hdr.data(), row.data(), node.data()) == 0);
            REQUIRE(memcmp(node.data(), tree.data() + 32 * i, 32) == 0);
          }
        }
        for (unsigned i = n_leaves; i < P; i++) REQUIRE(memcmp(tree.data() + 32 * (P - 1 + i), tree.data() + 32 * (P - 1 + n_leaves), 32) == 0);
        for (unsigned i = P - 1 + n_leaves; i < 2 * P - 1; i++) REQUIRE(memcmp(tree.data() + 32 * i, tree.data(), 32) != 0);
      }
    }
  }
  if (ht_check_failures() != 0) {
    fprintf(stderr, "asan_poseidon: the limb-bound checker fired: %s\n", ht_first_failure());
    return 1;
  }
  puts("ok");
  return 0;
}
