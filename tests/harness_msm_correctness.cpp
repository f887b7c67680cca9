// C++ restatement of the reference's `msm_correctness` test (P1A combined-top-solutions/tests/msm.rs:15-40) against the
// harness-named FFI (include/mi355_msm_shims.h) and the C++ mirror of the Rust operator API (include/mi355_msm.hpp):
// generate points/scalars, run the accelerator for `batches` batches on one context, compare each batch with the CPU
// oracle (here: oracle/liboracle.so standing in for arkworks' VariableBaseMSM).  Built and run by tests/test_harness_cpp.py,
// once per curve: the reference selects the curve at compile time with a cargo feature that becomes -DFEATURE_BLS12_377 /
// -DFEATURE_BLS12_381 (P1A 6block/build.rs:9,82), and so does this file (it then links libmi355msm_zprize_381.so).
//
// `load DIR` mirrors TEST_LOAD_DATA_FROM of the FPGA harness instead (P1B hardcaml/zprize/msm_pippenger/test_fpga_harness
// src/util.rs:151-171, tests/msm.rs:17-40): read DIR/{points,scalars,arkworks_results}.bin (serialize_unchecked: u64 count, then
// records), deserialize each scalar into its Fr limbs -- the normal-form integer a becomes a * 2^256 mod r, computed here on the
// CPU as arkworks' from_repr does -- hand those limbs to the MSM unchanged (the transmute to &[BigInteger256]) and compare every
// batch with arkworks_results.bin byte for byte.  No context option is involved: this checks the product ABI against the
// harness's own contract.
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <random>
#include <string>
#include <vector>

#define MI355_SHIM_ZPRIZE
#include "mi355_msm.hpp"
#include "mi355_msm_shims.h"

typedef int (*oracle_msm_t)(int, const void*, size_t, const void*, size_t, void*, int);

#if defined(FEATURE_BLS12_381)
static const int CURVE = MI355_BLS12_381_G1;
static const uint64_t R_TOP = 0x73eda753299d7d48ull;   // top limb of the BLS12-381 group order (ARKC bls12_381/src/fields/fr.rs:4)
static const uint64_t FR[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
#else
static const int CURVE = MI355_BLS12_377_G1;
static const uint64_t R_TOP = 0x12ab655e9a2ca556ull;   // ARKC bls12_377/src/fields/fr.rs:24
static const uint64_t FR[4] = {0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull, 0x12ab655e9a2ca556ull};
#endif

// a >= FR (little-endian 64-bit limbs)
static bool geq_r(const uint64_t* a) {
  for (int i = 3; i >= 0; i--)
    if (a[i] != FR[i]) return a[i] > FR[i];
  return true;
}
static void sub_r(uint64_t* a) {
  unsigned __int128 b = 0;
  for (int i = 0; i < 4; i++) {
    const unsigned __int128 d = (unsigned __int128)a[i] - FR[i] - b;
    a[i] = (uint64_t)d;
    b = (d >> 64) & 1;
  }
}
// a (< r) -> a * 2^256 mod r: 256 modular doublings (r < 2^255, so 2a < 2^256 never overflows the four limbs)
static void to_fr_limbs(uint64_t* a) {
  for (int k = 0; k < 256; k++) {
    for (int i = 3; i > 0; i--) a[i] = (a[i] << 1) | (a[i - 1] >> 63);
    a[0] <<= 1;
    if (geq_r(a)) sub_r(a);
  }
}

static std::vector<uint8_t> read_vec(const std::string& path, size_t rec, uint64_t& count) {
  std::vector<uint8_t> out;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(&count, 8, 1, f) != 1) {
    fprintf(stderr, "%s: cannot read\n", path.c_str());
    if (f) fclose(f);
    count = 0;
    return out;
  }
  out.resize(count * rec);
  if (fread(out.data(), 1, out.size(), f) != out.size()) {
    fprintf(stderr, "%s: short\n", path.c_str());
    out.clear();
    count = 0;
  }
  fclose(f);
  return out;
}

static int load_mode(const std::string& dir) {
  uint64_t n = 0, ns = 0, nr = 0;
  const std::vector<uint8_t> pts = read_vec(dir + "/points.bin", 96, n);
  const std::vector<uint8_t> sc = read_vec(dir + "/scalars.bin", 32, ns);
  const std::vector<uint8_t> res = read_vec(dir + "/arkworks_results.bin", 96, nr);
  if (n == 0 || ns % n || ns / n != nr) {
    fprintf(stderr, "%s: not a data set of whole batches\n", dir.c_str());
    return 2;
  }
  const size_t batches = ns / n;
  std::vector<mi355::BigInteger256> limbs(ns);   // Vec<Fr> as the MSM sees it after the transmute
  for (size_t i = 0; i < ns; i++) {
    memcpy(limbs[i].limbs, sc.data() + 32 * i, 32);
    if (geq_r(limbs[i].limbs)) {
      fprintf(stderr, "scalar %zu is not below r\n", i);
      return 2;
    }
    to_fr_limbs(limbs[i].limbs);
  }
  mi355::MultiScalarMultContext ctx;
  mi355::check(mi355_msm_create(&ctx.context, CURVE, -1));
  mi355::check(mi355_msm_set_bases_serialized(ctx.context, pts.data(), n));
  ctx.npoints = n;
  std::vector<mi355::G1Projective> got(batches);
  mi355::check(mi355_msm_run(ctx.context, got.data(), limbs.data(), n, batches));
  int bad = 0;
  for (size_t b = 0; b < batches; b++) {
    uint8_t rec[96];
    mi355::check(mi355_msm_point_to_serialized(CURVE, &got[b], rec));
    if (memcmp(rec, res.data() + 96 * b, 96) != 0) {
      fprintf(stderr, "batch %zu differs from arkworks_results.bin\n", b);
      bad++;
    }
  }
  printf("msm_correctness load curve=%d npoints=%llu batches=%zu: %s\n", CURVE, (unsigned long long)n, batches, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s liboracle.so npow [batches]  |  %s load DIR\n", argv[0], argv[0]);
    return 2;
  }
  if (std::string(argv[1]) == "load") {
    try {
      return load_mode(argv[2]);
    } catch (const mi355::MsmError& e) {
      fprintf(stderr, "%s\n", e.what());
      return 1;
    }
  }
  void* h = dlopen(argv[1], RTLD_NOW);
  if (!h) {
    fprintf(stderr, "dlopen oracle: %s\n", dlerror());
    return 2;
  }
  oracle_msm_t oracle_msm = (oracle_msm_t)dlsym(h, "oracle_msm");
  const size_t npoints = (size_t)1 << atoi(argv[2]);
  const size_t batches = argc > 3 ? atoi(argv[3]) : 4;

  std::vector<mi355::G1Affine> points(npoints);
  mi355::check(mi355_msm_generate_points(CURVE, 7, npoints < 2048 ? npoints : 2048, npoints, points.data(),
                                         sizeof(mi355::G1Affine)));
  points[3].infinity = 1;  // the baseline harness plants a point at infinity (P1A 6block/src/util.rs:26)
  std::mt19937_64 rng(12345);
  std::vector<mi355::BigInteger256> scalars(npoints * batches);
  for (auto& s : scalars) {
    for (int i = 0; i < 4; i++) s.limbs[i] = rng();
    s.limbs[3] %= R_TOP;  // below r
  }

  // (1) the Rust-API mirror
  mi355::MultiScalarMultContext ctx = mi355::multi_scalar_mult_init(points, CURVE);
  std::vector<mi355::G1Projective> got = mi355::multi_scalar_mult(ctx, points, scalars);
  if (got.size() != batches) return 1;

  // (2) the ZPrize harness FFI names
  RustContext rc{nullptr};
  mi355::check(mult_pippenger_init(&rc, points.data(), npoints, sizeof(mi355::G1Affine)));
  std::vector<mi355::G1Projective> got2(batches);
  mi355::check(mult_pippenger_inf(&rc, got2.data(), points.data(), npoints, batches, scalars.data(), sizeof(mi355::G1Affine)));

  int bad = 0;
  for (size_t b = 0; b < batches; b++) {
    mi355::G1Projective exp;
    if (oracle_msm(CURVE, points.data(), sizeof(mi355::G1Affine), scalars.data() + b * npoints, npoints, &exp, 0) != 0) return 2;
    if (memcmp(&exp, &got[b], sizeof exp) != 0 || memcmp(&exp, &got2[b], sizeof exp) != 0) {
      fprintf(stderr, "batch %zu differs from the CPU oracle\n", b);
      bad++;
    }
  }
  // (3) stateless msm() chops to the shorter input
  std::vector<mi355::BigInteger256> few(scalars.begin(), scalars.begin() + 10);
  mi355::G1Projective one = mi355::msm(points, few, CURVE), exp1;
  oracle_msm(CURVE, points.data(), sizeof(mi355::G1Affine), few.data(), 10, &exp1, 0);
  if (memcmp(&one, &exp1, sizeof one) != 0) bad++;
  // (4) the stream-ordered run (mi355::multi_scalar_mult_async): scalars in DEVICE memory, the call returns at once, wait() gives the same
  //     points.  This harness is plain g++ (no HIP headers), so the three runtime calls it needs come from the HIP library by name.
  {
    void* hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    typedef int (*malloc_t)(void**, size_t);
    typedef int (*memcpy_t)(void*, const void*, size_t, int);
    typedef int (*free_t)(void*);
    malloc_t hip_malloc = hip ? (malloc_t)dlsym(hip, "hipMalloc") : nullptr;
    memcpy_t hip_memcpy = hip ? (memcpy_t)dlsym(hip, "hipMemcpy") : nullptr;
    free_t hip_free = hip ? (free_t)dlsym(hip, "hipFree") : nullptr;
    if (!hip_malloc || !hip_memcpy || !hip_free) {
      fprintf(stderr, "libamdhip64.so: hipMalloc / hipMemcpy / hipFree not found\n");
      bad++;
    } else {
      void* d_scalars = nullptr;
      const size_t bytes = scalars.size() * sizeof(mi355::BigInteger256);
      if (hip_malloc(&d_scalars, bytes) != 0 || hip_memcpy(d_scalars, scalars.data(), bytes, 1 /* hipMemcpyHostToDevice */) != 0) {
        fprintf(stderr, "device allocation / copy failed\n");
        bad++;
      } else {
        mi355::MsmJob job = mi355::multi_scalar_mult_async(ctx, d_scalars, batches);
        std::vector<mi355::G1Projective>& got3 = job.wait();
        if (!job.done() || got3.size() != batches || memcmp(got3.data(), got.data(), batches * sizeof(mi355::G1Projective)) != 0) {
          fprintf(stderr, "the asynchronous run differs from the synchronous one\n");
          bad++;
        }
      }
      if (d_scalars) hip_free(d_scalars);
    }
  }
  printf("msm_correctness curve=%d npoints=2^%s batches=%zu: %s\n", CURVE, argv[2], batches, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
