// ntt.hpp -- radix-2 transforms over the scalar fields (arkworks' Radix2EvaluationDomain: fft, ifft, coset_fft, coset_ifft) and
// the pointwise product, on the arithmetic of fr.hpp.
//
// Reference behaviour: ARK poly/src/domain/mod.rs:99-170 (the four calls, distribute_powers), poly/src/domain/radix2/mod.rs:124-133
// (resize to the domain), ff/src/fields/mod.rs:440-480 (get_root_of_unity); the batch form is the reference's NTT_batch.
//
// Decomposition.  A transform of N = 2^k points is a chain of Stockham passes; a pass is one launch.  Pass i has a radix 2^P_i
// (sum P_i = k) and a stride s = 2^(P_0 + .. + P_(i-1)); with n = N / s and m = n / 2^P it computes, for every t = q + s p (q < s, p < m),
//
//     y[q + s (2^P p + j)] = w_n^(p j) * sum_i x[t + (N / 2^P) i] * w_(2^P)^(i j),      j < 2^P,
//
// so every pass reads and writes in natural order and no bit-reversal launch exists.  A block takes C = TILE / 2^P neighbouring t:
// for each i it reads C consecutive elements (C * 32 bytes), and it writes runs of min(s, C) elements or, while s < C, one contiguous
// run of the whole tile.  The 2^P-point transforms of a tile run in LDS across P butterfly levels (t = w * b; a' = a + t;
// b' = a - t), decimation in frequency order with the twiddle on the way in, which leaves bin j at position bitrev(j): the store reads
// it from there.  An LDS element is the nine limbs themselves -- 36 bytes, an odd number of banks, so the power-of-two strides of the
// butterflies spread over all banks without padding.
//
// Twiddles.  w_N^e = LO[e mod 2^h] * HI[e >> h] with h = min(k, 14): 2^h + 2^(k-h) entries, one extra product.  The butterfly twiddles
// w_(2^P)^i, i < 2^(P-1), come from one 512-entry table of w_1024^i.  The powers of a coset offset use the same two-level form.  The
// first pass converts from the ABI form as it loads (and zero-fills from in_len on), the last converts, scales by 1/N and reduces as
// it stores; the conversions, the offset powers and 1/N are folded into those loads and stores.
//
// Every per-element step is an MSM_HD function, so the host build (host_test_api.cpp, ht_ntt_*) runs the same code under MSM_CHECK.
#pragma once
#include "fr.hpp"

namespace msm {

constexpr uint32_t NTT_TILE_LOG = 10;            // elements of a tile in LDS: 1024 x 36 B
constexpr uint32_t NTT_TILE = 1u << NTT_TILE_LOG;
constexpr uint32_t NTT_MAX_PASS_LOG = NTT_TILE_LOG;
constexpr uint32_t NTT_DEFAULT_PASS_LOG = 8;     // C = 4: a run of 128 bytes per read
constexpr uint32_t NTT_LO_LOG = 14;
constexpr uint32_t NTT_SMALL_LOG = 10;           // the butterfly table holds w_1024^i, i < 512
constexpr uint32_t NTT_MAX_LOG = 28;
constexpr uint32_t NTT_THREADS = 256;

constexpr uint32_t kNttFirst = 1u, kNttLast = 2u, kNttNormal = 4u, kNttCosetIn = 8u, kNttCosetOut = 16u, kNttRevIn = 32u, kNttRevOut = 64u;

// the two-level tables of one root (or one offset): root^lo for lo < 2^h, root^(hi 2^h) for hi < 2^(k-h); canonical entries
struct NttTable {
  const Fr* lo;
  const Fr* hi;
};

struct NttPass {
  const uint32_t* src;   // 8 words per element, `batch` vectors N elements apart
  uint32_t* dst;
  uint32_t k, p, log_s, log_c, in_len, flags;
  NttTable w, g;         // the root's tables; the offset's (used with kNttCosetIn / kNttCosetOut only)
  const Fr* small;       // w_1024^i
  Fr scale;              // 1/N on the last pass of an inverse transform (class M), else unused
  uint32_t has_scale;
};

MSM_HD uint32_t ntt_bitrev(uint32_t x, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; i++) r |= ((x >> i) & 1u) << (bits - 1 - i);
  return r;
}

MSM_HD uint32_t ntt_lo_log(uint32_t k) { return k < NTT_LO_LOG ? k : NTT_LO_LOG; }

// root^e from the two-level tables: class M
template <class FR>
MSM_HD void ntt_table_mul(Fr& x, const NttTable& t, uint32_t k, uint32_t e) {
  const uint32_t h = ntt_lo_log(k);
  Fr f = t.lo[e & ((1u << h) - 1)];
  fr_mul<FR>(x, x, f);
  f = t.hi[e >> h];
  fr_mul<FR>(x, x, f);
}

// the radices of the passes: ceil(k / pass_log) passes, as even as they come; returns the pass count (k = 0: one pass of radix 1)
MSM_HD uint32_t ntt_plan(uint32_t k, uint32_t pass_log, uint32_t (&p)[NTT_MAX_LOG]) {
  const uint32_t n = k == 0 ? 1 : (k + pass_log - 1) / pass_log;
  for (uint32_t i = 0; i < n; i++) p[i] = k / n + (i < k % n ? 1 : 0);
  return n;
}

MSM_HD uint32_t ntt_log_c(uint32_t k, uint32_t p) { return (k - p) < (NTT_TILE_LOG - p) ? (k - p) : (NTT_TILE_LOG - p); }

// element i of tile `tile` on the way in: lds[i] = x[t + (N / 2^P) j], j = i >> log_c, t = tile * C + (i mod C)
template <class FR>
MSM_HD void ntt_load(Fr& x, const NttPass& ps, const uint32_t* src, uint32_t tile, uint32_t i) {
  const uint32_t c = i & ((1u << ps.log_c) - 1), j = i >> ps.log_c;
  const uint32_t idx = ((tile << ps.log_c) | c) + (j << (ps.k - ps.p));
  if (!(ps.flags & kNttFirst)) {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = src[(size_t)idx * 8 + q];
    fr_unpack(x, w);   // class M of the pass before
    return;
  }
  const uint32_t phys = (ps.flags & kNttRevIn) ? ntt_bitrev(idx, ps.k) : idx;
  if (phys >= ps.in_len) {
    fr_zero(x);
    return;
  }
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = src[(size_t)phys * 8 + q];
  fr_from_abi<FR>(x, w, (ps.flags & kNttNormal) != 0);
  if (ps.flags & kNttCosetIn) ntt_table_mul<FR>(x, ps.g, ps.k, idx);
}

// butterfly u of level l (l < P) on a tile: u = (jj << log_c) | c, jj < 2^(P-1)
template <class FR>
MSM_HD void ntt_butterfly(Fr* lds, const NttPass& ps, uint32_t l, uint32_t u) {
  const uint32_t c = u & ((1u << ps.log_c) - 1), jj = u >> ps.log_c;
  const uint32_t hl = ps.p - l - 1, grp = jj >> hl, pos = jj & ((1u << hl) - 1);
  const uint32_t ja = (grp << (hl + 1)) | pos, jb = ja + (1u << hl);
  // the group's twiddle: w_(2^P)^(bitrev_l(grp) 2^(P - l - 1)), looked up as a power of w_1024
  const uint32_t e = (ntt_bitrev(grp, l) << hl) << (NTT_SMALL_LOG - ps.p);
  const Fr w = ps.small[e];
  Fr a = lds[(ja << ps.log_c) | c], b = lds[(jb << ps.log_c) | c], t, d;
  fr_mul<FR>(t, b, w);
  fr_sub<FR>(d, a, t);
  fr_add(a, a, t);
  fr_carry(a);
  fr_carry(d);
  lds[(ja << ps.log_c) | c] = a;
  lds[(jb << ps.log_c) | c] = d;
}

// output i of a tile: bin j of column c times w_n^(p j), to y[q + s (2^P p + j)]
template <class FR>
MSM_HD void ntt_store(const Fr* lds, const NttPass& ps, uint32_t* dst, uint32_t tile, uint32_t i) {
  const uint32_t sc = ps.log_s < ps.log_c ? ps.log_s : ps.log_c;
  const uint32_t ql = i & ((1u << sc) - 1), j = (i >> sc) & ((1u << ps.p) - 1), pp = i >> (sc + ps.p);
  const uint32_t c = (pp << sc) | ql, t = (tile << ps.log_c) | c;
  const uint32_t q = t & ((1u << ps.log_s) - 1), sp = t - q;   // sp = s p
  const uint32_t o = q + (sp << ps.p) + (j << ps.log_s);
  Fr x = lds[(ntt_bitrev(j, ps.p) << ps.log_c) | c];
  uint32_t w[8];
  if (!(ps.flags & kNttLast)) {
    ntt_table_mul<FR>(x, ps.w, ps.k, sp * j);   // s p j < (N / 2^P) 2^P
    fr_pack(w, x);
#pragma unroll
    for (int z = 0; z < 8; z++) dst[(size_t)o * 8 + z] = w[z];
    return;
  }
  if (ps.has_scale) fr_mul<FR>(x, x, ps.scale);
  if (ps.flags & kNttCosetOut) ntt_table_mul<FR>(x, ps.g, ps.k, o);
  fr_to_abi<FR>(w, x, (ps.flags & kNttNormal) != 0);
  const uint32_t phys = (ps.flags & kNttRevOut) ? ntt_bitrev(o, ps.k) : o;
#pragma unroll
  for (int z = 0; z < 8; z++) dst[(size_t)phys * 8 + z] = w[z];
}

// out = a * b in the ABI form of `normal`; any 256-bit inputs
template <class FR>
MSM_HD void fr_mul_abi(uint32_t (&out)[8], const uint32_t (&a)[8], const uint32_t (&b)[8], bool normal) {
  Fr x, y, c;
  fr_unpack(x, a);
  fr_unpack(y, b);
  fr_mul<FR>(x, x, y);          // a b / R: below r + 2^251
  fr_const<FR>(c, normal ? 1 : 0);
  fr_mul<FR>(x, x, c);
  fr_pack(out, x);
  fr_canon<FR>(out);
}

// table entry i: base^i, canonical
template <class FR>
MSM_HD void ntt_table_entry(Fr& r, const Fr& base, uint32_t i) {
  fr_pow_u32<FR>(r, base, i);
}

// ---- what a handle derives once (host code in the engine and in the host test build alike) ---------------------------------------

// base^e for a 256-bit exponent, canonical
template <class FR>
MSM_HD void fr_pow_words(Fr& r, const Fr& base, const uint32_t (&e)[8]) {
  Fr acc;
  fr_set<FR>(acc, FR::ONE);
  for (int i = 255; i >= 0; i--) {
    fr_mul<FR>(acc, acc, acc);
    fr_reduce<FR>(acc);
    if ((e[i >> 5] >> (i & 31)) & 1) {
      fr_mul<FR>(acc, acc, base);
      fr_reduce<FR>(acc);
    }
  }
  r = acc;
}

// a^(r - 2): the inverse of a non-zero canonical a (0 for 0)
template <class FR>
MSM_HD void fr_inv(Fr& r, const Fr& a) {
  uint32_t e[8];
  int64_t b = -2;
  for (int i = 0; i < 8; i++) {
    b += FR::P32[i];
    e[i] = (uint32_t)b;
    b >>= 32;
  }
  fr_pow_words<FR>(r, a, e);
}

// get_root_of_unity(2^k): TWO_ADIC_ROOT squared TWO_ADICITY - k times
template <class FR>
MSM_HD void ntt_root(Fr& w, uint32_t k) {
  fr_set<FR>(w, FR::TWO_ADIC_ROOT);
  for (uint32_t i = k; i < (uint32_t)FR::TWO_ADICITY; i++) {
    fr_mul<FR>(w, w, w);
    fr_reduce<FR>(w);
  }
}

// 2^-k
template <class FR>
MSM_HD void ntt_size_inv(Fr& r, uint32_t k) {
  Fr two, one;
  fr_set<FR>(one, FR::ONE);
  fr_add(two, one, one);
  fr_carry(two);
  fr_reduce<FR>(two);
  fr_pow_u32<FR>(r, two, k);
  fr_inv<FR>(r, r);
}

// base^(2^h)
template <class FR>
MSM_HD void ntt_hi_base(Fr& r, const Fr& base, uint32_t h) {
  r = base;
  for (uint32_t i = 0; i < h; i++) {
    fr_mul<FR>(r, r, r);
    fr_reduce<FR>(r);
  }
}

constexpr unsigned kNttKindInverse = 1u, kNttKindCoset = 2u;                     // kind = 0 .. 3
constexpr unsigned kNttCallNormal = 1u, kNttCallNR = 2u, kNttCallRN = 4u;        // the flags of a call

// the shape and flags of pass i of npass (tables, pointers and the scale are the caller's)
MSM_HD void ntt_pass_shape(NttPass& ps, uint32_t k, const uint32_t* radix, uint32_t npass, uint32_t i, unsigned kind, unsigned call_flags, uint32_t in_len) {
  uint32_t log_s = 0;
  for (uint32_t z = 0; z < i; z++) log_s += radix[z];
  ps.k = k;
  ps.p = radix[i];
  ps.log_s = log_s;
  ps.log_c = ntt_log_c(k, radix[i]);
  ps.in_len = in_len;
  ps.flags = (call_flags & kNttCallNormal) ? kNttNormal : 0;
  ps.has_scale = 0;
  if (i == 0) {
    ps.flags |= kNttFirst;
    if (kind == kNttKindCoset) ps.flags |= kNttCosetIn;
    if (call_flags & kNttCallRN) ps.flags |= kNttRevIn;
  }
  if (i + 1 == npass) {
    ps.flags |= kNttLast;
    if (kind & kNttKindInverse) ps.has_scale = 1;
    if (kind == (kNttKindCoset | kNttKindInverse)) ps.flags |= kNttCosetOut;
    if (call_flags & kNttCallNR) ps.flags |= kNttRevOut;
  }
}

#if defined(__HIPCC__)
template <class FR>
__global__ void __launch_bounds__(NTT_THREADS) k_ntt_pass(NttPass ps) {
  __shared__ Fr lds[NTT_TILE];
  const uint32_t elems = 1u << (ps.p + ps.log_c);
  const size_t vec = (size_t)blockIdx.y << ps.k;
  const uint32_t* src = ps.src + vec * 8;
  uint32_t* dst = ps.dst + vec * 8;
  for (uint32_t i = threadIdx.x; i < elems; i += NTT_THREADS) ntt_load<FR>(lds[i], ps, src, blockIdx.x, i);
  for (uint32_t l = 0; l < ps.p; l++) {
    __syncthreads();
    for (uint32_t u = threadIdx.x; u < elems / 2; u += NTT_THREADS) ntt_butterfly<FR>(lds, ps, l, u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < elems; i += NTT_THREADS) ntt_store<FR>(lds, ps, dst, blockIdx.x, i);
}

template <class FR>
__global__ void __launch_bounds__(NTT_THREADS) k_fr_mul_vec(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, uint32_t normal) {
  const size_t i = (size_t)blockIdx.x * NTT_THREADS + threadIdx.x;
  if (i >= n) return;
  uint32_t x[8], y[8], z[8];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    x[q] = a[i * 8 + q];
    y[q] = b[i * 8 + q];
  }
  fr_mul_abi<FR>(z, x, y, normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) out[i * 8 + q] = z[q];
}

// out[i] = base^i, i < n: one lane per entry
template <class FR>
__global__ void __launch_bounds__(NTT_THREADS) k_ntt_table(Fr base, uint32_t n, Fr* out) {
  const uint32_t i = blockIdx.x * NTT_THREADS + threadIdx.x;
  if (i >= n) return;
  Fr r;
  ntt_table_entry<FR>(r, base, i);
  out[i] = r;
}

// the yardstick of tests/test_isa_ntt.py: one product, one add, one sub per element
template <class FR>
__global__ void __launch_bounds__(NTT_THREADS) k_fr_yardstick(const Fr* a, const Fr* b, Fr* out, uint32_t n) {
  const uint32_t i = blockIdx.x * NTT_THREADS + threadIdx.x;
  if (i >= n) return;
  Fr x = a[i], y = b[i], t, d;
  fr_mul<FR>(t, y, x);
  fr_sub<FR>(d, x, t);
  fr_add(x, x, t);
  out[2 * i] = x;
  out[2 * i + 1] = d;
}
#endif

}  // namespace msm
