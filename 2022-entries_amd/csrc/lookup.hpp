// lookup.hpp -- lookup-argument columns over the scalar fields: a resident hash table of Fr keys with a probe-and-count kernel (the
// multiplicities of logUp), the expansion into plookup's sorted vector s = (f, t) sorted by t, and the logUp running sum on the batch
// inversion of poly.hpp and the sum scan of scan.hpp.
//
// Reference behaviour: none to compare against (the prover half of the reference's Plonk entry is stripped).  The contract is stated on
// integers: two 256-bit patterns match when they are equal modulo r IN THE FORM OF THE CALL.  Arkworks images are in bijection with
// residues, so in either form the matching key is (the pattern) mod r -- a quotient estimate from the top word, one multiple of r
// subtracted and two conditional subtractions (lookup_canon), never a field product.
//
// The table.  `slots` = the power of two >= 2 n_t of u32 table indices (0xFFFFFFFF: empty), open addressing with linear probing; the
// hash is murmur3's over all eight words of the canonical key.
//   build   one lane per entry i walks from hash(t[i]): an empty slot is claimed with a compare-and-swap; a slot whose index j has
//           t[j] == t[i] is lowered with an atomic min, which makes the slot's final content min{i : t[i] == key} = first(i) whatever
//           the arrival order.  A slot, once claimed, keeps its KEY for ever (only equal keys lower it) and never empties, so equal keys
//           meet in one slot: a lane that loses the compare-and-swap looks at the winner's key like at any other occupant.  During the
//           build slots are read through agent-scope atomic loads only (another XCD's L2 may hold a stale line); the canonical keys come
//           from an earlier launch and are read plainly.
//   probe   a separate launch, one lane per value: the same walk with plain loads; an empty slot is a miss.  Before the add to the u32
//           counter of the entry found, a wave combines the lanes that found the same entry (k_lookup_probe): the usual real input is a
//           column padded with one default entry; a group of 16 lanes or more is carried over the runs of 256 values a block takes and
//           added once per block, since adds to one address are serialised.  Misses are carried the same way: a block that has any adds
//           their number to the missing count and lowers the first missing index (two 64-bit atomics per block).
// No lane ever waits on another: every iteration of a walk ends in a claim, a match or a step to the next slot, a walk is bounded by
// `slots` (at load <= 1/2 an empty slot always ends it earlier) and one that wraps sets an error word.  Nothing is polled.  Sums and
// minima of integers do not depend on their order, so every output byte is a function of the inputs alone.
//
//   mult    one lane per table entry writes its counter as an Fr element: the integer itself, or one product by 2^256 R for the image.
//   sorted  an exclusive u32 scan of 1 + count[i] (tiles of 1024 through LDS, levels as separate launches, as scan.hpp), then one lane
//           per OUTPUT position finds its entry by bisection over the offsets and copies the canonical key: the work per output element
//           is the same whatever the distribution.
//   logUp   one lane per row writes the m + 1 denominators beta + values_c[j], beta + table[j]; the batch inversion of poly.hpp runs
//           over the (m + 1) n of them in place (a zero stays zero); one lane per row forms mult[j] / (beta + table[j]) (into the last
//           helper column) and term[j] = sum_c helper_c[j] - that; the sum scan of scan.hpp runs over the terms.
//
// Lazy bounds (the host build runs every step under MSM_CHECK): a sum of up to 8 class-M values with a carry pass after each add stays
// below 16r; fr_sub adds 4r: 20r, inside what fr_mul takes as its first operand (R / r = 70.6 for BLS12-381).
#pragma once
#include "scan.hpp"

namespace msm {

constexpr unsigned kLookupNormal = 1u, kLookupDevice = 2u;            // the flags of a call
constexpr uint32_t LOOKUP_THREADS = 256;
constexpr uint32_t LOOKUP_EMPTY = 0xffffffffu;
constexpr uint32_t LOOKUP_MAX_TABLE_LOG = 28, LOOKUP_MAX_VALUES_LOG = 30;
constexpr uint32_t LOOKUP_SCAN_TILE_LOG = 10, LOOKUP_SCAN_RUN = 4;    // a block of 256 lanes, 4 neighbours each
constexpr uint32_t LOOKUP_SCAN_MAX_LEVELS = 4;
constexpr uint32_t LOOKUP_HOT_LANES = 16, LOOKUP_MAX_BATCHES = 16;     // the probe: a heavy group, and the most runs of 256 values a block takes
constexpr uint32_t LOGUP_MAX_COLUMNS = 8;

// the words every launch of a call shares: zeroed (first: all ones) before the launches
struct LookupHead {
  unsigned long long missing, first;   // values without a match; the smallest such j (all ones: none)
  uint32_t err, max_probe, distinct, pad;
};

struct LookupTab {
  const uint32_t* keys;     // n canonical keys of 8 words
  uint32_t* slots;          // mask + 1 table indices
  uint32_t n, mask;
};

struct LookupCanon {
  const uint32_t* src;
  uint32_t* dst;
  uint64_t n;
};

struct LookupBuild {
  LookupTab t;
  LookupHead* head;
};

struct LookupProbe {
  LookupTab t;
  const uint32_t* values;
  uint64_t n_f;
  uint32_t* index;          // may be NULL
  uint32_t* count;          // one per table entry, zeroed
  LookupHead* head;
  uint32_t batches;         // runs of 256 values a block takes (the kernel's grid; the host build has no blocks)
};

struct LookupMult {
  const uint32_t* count;
  uint32_t* dst;
  uint32_t n, normal;
  Fr image;                 // 2^256 R, canonical: count -> the arkworks image in one product
};

// one level of the u32 scan: dst[i] = carry[tile] + sum_(i' < i, same tile) (src[i'] + plus_one); totals[tile] = the tile's sum
struct LookupScan {
  const uint32_t* src;
  uint32_t* dst;            // down only; may be src
  uint32_t* totals;         // up only
  const uint32_t* carry;    // down; NULL at the top level
  uint64_t n;
  uint32_t plus_one;
};

struct LookupExpand {
  const uint32_t *keys, *off;   // off[i]: where entry i's run begins
  uint32_t* dst;
  uint32_t n_t;
  uint64_t total;               // n_t + n_f
};

struct LogupRows {
  const uint32_t *values, *table, *mult;   // m columns `stride` elements apart; n; n
  uint32_t* helpers;                       // (m + 1) n elements: the denominators, then their inverses, then the helper columns
  uint32_t* term;                          // n elements
  uint64_t n, stride;
  uint32_t m, normal;
  Fr beta;                                 // canonical
};

// ---- the atomics: agent scope on the device, plain sequential operations on the host ----------------------------------------------------

#if defined(__HIP_DEVICE_COMPILE__)
#define LOOKUP_ATOMIC(dev, host) (dev)
#else
#define LOOKUP_ATOMIC(dev, host) (host)
#endif

MSM_HD uint32_t lookup_slot_load(const uint32_t* p) {
  return LOOKUP_ATOMIC(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), *p);
}
// what the slot held before: LOOKUP_EMPTY when the claim won
MSM_HD uint32_t lookup_slot_claim(uint32_t* p, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t expected = LOOKUP_EMPTY;
  __hip_atomic_compare_exchange_strong(p, &expected, i, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return expected;
#else
  const uint32_t old = *p;
  if (old == LOOKUP_EMPTY) *p = i;
  return old;
#endif
}
MSM_HD void lookup_min_u32(uint32_t* p, uint32_t v) {
  LOOKUP_ATOMIC((void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (void)(*p = v < *p ? v : *p));
}
MSM_HD void lookup_max_u32(uint32_t* p, uint32_t v) {
  LOOKUP_ATOMIC((void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (void)(*p = v > *p ? v : *p));
}
MSM_HD void lookup_add_u32(uint32_t* p, uint32_t v) {
  LOOKUP_ATOMIC((void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (void)(*p += v));
}
MSM_HD void lookup_add_u64(unsigned long long* p, unsigned long long v) {
  LOOKUP_ATOMIC((void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (void)(*p += v));
}
MSM_HD void lookup_min_u64(unsigned long long* p, unsigned long long v) {
  LOOKUP_ATOMIC((void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (void)(*p = v < *p ? v : *p));
}

// ---- keys -------------------------------------------------------------------------------------------------------------------------------

// any 256-bit pattern -> its residue.  2^256 / r is 2.2 for BLS12-381 and 13.7 for BLS12-377 (r has 253 bits), so the quotient is
// estimated from the top words: with T the top word of r, q = floor(w_7 / (T + 1)) has q r <= q (T + 1) 2^224 <= w, and the true quotient
// is below (w_7 + 1) / T, which exceeds w_7 / (T + 1) by (w_7 + T + 1) / (T (T + 1)) < 10^-7: q is the quotient or one less.  One
// subtraction of q r (eight 32 x 32 multiply-adds, no field product) and two conditional subtractions of r, one of them for margin.
template <class FR>
MSM_HD void lookup_canon(uint32_t (&w)[8]) {
  static_assert((uint64_t)FR::P32[7] * FR::P32[7] > ((uint64_t)1 << 40), "the quotient estimate needs a top word of r well above 2^20");
  const uint32_t q = w[7] / (FR::P32[7] + 1u);
  uint64_t carry = 0;
  int64_t b = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    carry += (uint64_t)q * FR::P32[j];
    b += (int64_t)w[j] - (int64_t)(uint32_t)carry;
    carry >>= 32;
    w[j] = (uint32_t)b;
    b >>= 32;
  }
  MSM_CHECK(b == 0 && carry == 0);
#pragma unroll
  for (int it = 0; it < 2; it++) {
    uint32_t d[8];
    b = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      b += (int64_t)w[j] - FR::P32[j];
      d[j] = (uint32_t)b;
      b >>= 32;
    }
    if (b == 0) {
#pragma unroll
      for (int j = 0; j < 8; j++) w[j] = d[j];
    }
  }
}

template <class FR>
MSM_HD void lookup_load_key(uint32_t (&w)[8], const uint32_t* src, uint64_t i) {
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = src[i * 8 + q];
  lookup_canon<FR>(w);
}

MSM_HD uint32_t lookup_rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

// murmur3 (x86, 32 bits) over the eight words
MSM_HD uint32_t lookup_hash(const uint32_t (&w)[8]) {
  uint32_t h = 0x9747b28cu;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    uint32_t k = w[q] * 0xcc9e2d51u;
    k = lookup_rotl(k, 15) * 0x1b873593u;
    h = lookup_rotl(h ^ k, 13) * 5u + 0xe6546b64u;
  }
  h ^= 32u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}

MSM_HD bool lookup_key_is(const uint32_t* keys, uint32_t at, const uint32_t (&w)[8]) {
  uint32_t diff = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) diff |= keys[(uint64_t)at * 8 + q] ^ w[q];
  return diff == 0;
}

template <class FR>
MSM_HD void lookup_canon_elem(const LookupCanon& p, uint64_t i) {
  uint32_t w[8];
  lookup_load_key<FR>(w, p.src, i);
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[i * 8 + q] = w[q];
}

// ---- build --------------------------------------------------------------------------------------------------------------------------------

// entry i into the table; returns true when this lane claimed a slot (a key not seen before).  steps: the slots the walk looked at
MSM_HD bool lookup_insert(const LookupBuild& p, uint32_t i, uint32_t& steps) {
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = p.t.keys[(uint64_t)i * 8 + q];
  uint32_t h = lookup_hash(w) & p.t.mask;
  for (steps = 1;; steps++) {
    uint32_t cur = lookup_slot_load(p.t.slots + h);
    if (cur == LOOKUP_EMPTY) {
      cur = lookup_slot_claim(p.t.slots + h, i);
      if (cur == LOOKUP_EMPTY) return true;
    }
    if (lookup_key_is(p.t.keys, cur, w)) {
      lookup_min_u32(p.t.slots + h, i);
      return false;
    }
    if (steps > p.t.mask) {
      lookup_max_u32(&p.head->err, 1u);
      return false;
    }
    h = (h + 1) & p.t.mask;
  }
}

// the longest walk: most lanes see a maximum that is already theirs or above
MSM_HD void lookup_note_walk(const LookupBuild& p, uint32_t steps) {
  if (steps > lookup_slot_load(&p.head->max_probe)) lookup_max_u32(&p.head->max_probe, steps);
}

// ---- probe --------------------------------------------------------------------------------------------------------------------------------

// value j: the first table index of its key, or LOOKUP_EMPTY
template <class FR>
MSM_HD uint32_t lookup_find(const LookupProbe& p, uint64_t j) {
  uint32_t w[8];
  lookup_load_key<FR>(w, p.values, j);
  uint32_t h = lookup_hash(w) & p.t.mask, found = LOOKUP_EMPTY;
  for (uint32_t steps = 1;; steps++) {
    const uint32_t cur = p.t.slots[h];
    if (cur == LOOKUP_EMPTY) break;
    if (lookup_key_is(p.t.keys, cur, w)) {
      found = cur;
      break;
    }
    if (steps > p.t.mask) {
      lookup_max_u32(&p.head->err, 1u);
      break;
    }
    h = (h + 1) & p.t.mask;
  }
  if (p.index) p.index[j] = found;
  return found;
}

// `amount` values found entry `found`, the smallest of them value j
MSM_HD void lookup_credit(const LookupProbe& p, uint32_t found, uint64_t j, uint32_t amount) {
  if (found != LOOKUP_EMPTY) {
    lookup_add_u32(p.count + found, amount);
  } else {
    lookup_add_u64(&p.head->missing, amount);
    lookup_min_u64(&p.head->first, j);
  }
}

// ---- the multiplicities as elements -----------------------------------------------------------------------------------------------------------

template <class FR>
MSM_HD void lookup_mult_elem(const LookupMult& p, uint32_t i) {
  const uint32_t c = p.count[i];
  uint32_t w[8] = {c, 0, 0, 0, 0, 0, 0, 0};
  if (!p.normal) {
    Fr x, y;
    fr_unpack(x, w);
    fr_mul<FR>(y, x, p.image);
    fr_pack(w, y);
    fr_canon<FR>(w);
  }
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[(uint64_t)i * 8 + q] = w[q];
}

// 2^256 R mod r, canonical
template <class FR>
MSM_HD void lookup_image_const(Fr& c) {
  Fr a, b;
  fr_const<FR>(a, 2);   // 2^256
  fr_const<FR>(b, 1);   // R^2
  fr_mul<FR>(c, a, b);
  fr_reduce<FR>(c);
}

// ---- the u32 scan and the expansion -----------------------------------------------------------------------------------------------------------

MSM_HD uint32_t lookup_scan_elem(const LookupScan& p, uint64_t i) { return i < p.n ? p.src[i] + p.plus_one : 0u; }

// the lengths of the levels: len[0] = n, len[j + 1] = the tiles of level j, down to one tile
MSM_HD uint32_t lookup_scan_plan(uint64_t n, uint64_t (&len)[LOOKUP_SCAN_MAX_LEVELS + 1]) {
  uint32_t levels = 0;
  len[0] = n;
  while (len[levels] > ((uint64_t)1 << LOOKUP_SCAN_TILE_LOG)) {
    len[levels + 1] = (len[levels] + ((uint64_t)1 << LOOKUP_SCAN_TILE_LOG) - 1) >> LOOKUP_SCAN_TILE_LOG;
    levels++;
  }
  return levels + 1;
}

MSM_HD uint64_t lookup_scan_work_words(uint64_t n) {
  uint64_t len[LOOKUP_SCAN_MAX_LEVELS + 1], total = 4;
  const uint32_t levels = lookup_scan_plan(n, len);
  for (uint32_t j = 1; j < levels; j++) total += len[j];
  return total;
}

// off[i] = sum_(i' < i) (count[i'] + 1); RUN has scan_up(LookupScan) and scan_down(LookupScan)
template <class RUN>
void lookup_scan_chain(RUN& run, uint32_t* off, const uint32_t* count, uint64_t n, uint32_t* work) {
  uint64_t len[LOOKUP_SCAN_MAX_LEVELS + 1];
  const uint32_t levels = lookup_scan_plan(n, len);
  uint32_t* part[LOOKUP_SCAN_MAX_LEVELS + 1];
  uint32_t* at = work;
  for (uint32_t j = 1; j < levels; j++) {
    part[j] = at;
    at += len[j];
  }
  for (uint32_t j = 0; j + 1 < levels; j++) {
    LookupScan u{};
    u.src = j == 0 ? count : part[j];
    u.n = len[j];
    u.plus_one = j == 0 ? 1u : 0u;
    u.totals = part[j + 1];
    run.scan_up(u);
  }
  for (uint32_t j = levels; j-- > 0;) {
    LookupScan d{};
    d.src = j == 0 ? count : part[j];
    d.dst = j == 0 ? off : part[j];   // (a level above the first turns its totals into its carries in place)
    d.n = len[j];
    d.plus_one = j == 0 ? 1u : 0u;
    d.carry = j + 1 < levels ? part[j + 1] : nullptr;
    run.scan_down(d);
  }
}

// output position g: the entry whose run holds it, by bisection over the offsets
MSM_HD void lookup_expand_elem(const LookupExpand& p, uint64_t g) {
  uint32_t lo = 0, hi = p.n_t;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (p.off[mid] <= g) lo = mid; else hi = mid;
  }
#pragma unroll
  for (int q = 0; q < 8; q++) p.dst[g * 8 + q] = p.keys[(uint64_t)lo * 8 + q];
}

// ---- logUp ------------------------------------------------------------------------------------------------------------------------------------

// row j: the m + 1 denominators, column-major in `helpers`; the column loop stays rolled
template <class FR>
MSM_HD void logup_den_row(const LogupRows& p, uint64_t j) {
#pragma unroll 1
  for (uint32_t c = 0; c <= p.m; c++) {
    const uint32_t* src = c < p.m ? p.values + (c * p.stride + j) * 8 : p.table + j * 8;
    uint32_t w[8];
    Fr x;
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = src[q];
    fr_from_abi<FR>(x, w, p.normal != 0);
    fr_add(x, x, p.beta);
    fr_to_abi<FR>(w, x, p.normal != 0);
#pragma unroll
    for (int q = 0; q < 8; q++) p.helpers[(c * p.n + j) * 8 + q] = w[q];
  }
}

// row j after the inversion: helper_m = mult / (beta + table), term = sum_c helper_c - helper_m
template <class FR>
MSM_HD void logup_term_row(const LogupRows& p, uint64_t j) {
  uint32_t w[8];
  Fr acc, x, y;
  fr_zero(acc);
#pragma unroll 1
  for (uint32_t c = 0; c < p.m; c++) {
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = p.helpers[(c * p.n + j) * 8 + q];
    fr_from_abi<FR>(x, w, p.normal != 0);
    fr_add(acc, acc, x);
    fr_carry(acc);
  }
  uint32_t* last = p.helpers + ((uint64_t)p.m * p.n + j) * 8;
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = last[q];
  fr_from_abi<FR>(x, w, p.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = p.mult[j * 8 + q];
  fr_from_abi<FR>(y, w, p.normal != 0);
  fr_mul<FR>(x, x, y);
  fr_to_abi<FR>(w, x, p.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) last[q] = w[q];
  fr_sub<FR>(acc, acc, x);
  fr_carry(acc);
  fr_to_abi<FR>(w, acc, p.normal != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) p.term[j * 8 + q] = w[q];
}

#if defined(__HIPCC__)

template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_lookup_canon(LookupCanon p) {
  const uint64_t i = (uint64_t)blockIdx.x * LOOKUP_THREADS + threadIdx.x;
  if (i < p.n) lookup_canon_elem<FR>(p, i);
}

// (the field plays no part in this kernel, in the scans and in the expansion: the keys are canonical already)
template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_lookup_build(LookupBuild p) {
  const uint32_t i = blockIdx.x * LOOKUP_THREADS + threadIdx.x;
  bool claimed = false;
  if (i < p.t.n) {
    uint32_t steps;
    claimed = lookup_insert(p, i, steps);
    lookup_note_walk(p, steps);
  }
  // one add per wave: the lanes that claimed a slot
  const unsigned long long won = __ballot(claimed);
  if (won && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)won) - 1)) lookup_add_u32(&p.head->distinct, (uint32_t)__popcll(won));
}

// A block takes p.batches consecutive runs of 256 values.  Per run, the lanes of a wave that found the same entry add once: `rest` is
// wave-uniform and each turn retires its leader's group.  Adds to ONE address are serialised by the L2 (profiles/lookup.txt), so their
// number is what has to fall where many values meet: a group of a quarter wave or more -- the padding entry of a padded column -- is not
// added at once but kept in (hot, hot_amount), wave-uniform, until another heavy entry replaces it, and the misses of all runs are kept
// in (miss, miss_first); after the last run the four waves of the block hand both over through LDS and thread 0 adds what is equal once.
template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_lookup_probe(LookupProbe p) {
  constexpr uint32_t WAVES = LOOKUP_THREADS / 64;
  __shared__ uint32_t s_hot[WAVES], s_amount[WAVES];
  __shared__ unsigned long long s_miss[WAVES], s_first[WAVES];
  const uint32_t lane = threadIdx.x & 63, wave_at = threadIdx.x & ~63u;
  uint32_t hot = LOOKUP_EMPTY, hot_amount = 0;
  unsigned long long miss = 0, miss_first = ~0ull;
#pragma unroll 1
  for (uint32_t b = 0; b < p.batches; b++) {
    const uint64_t base = ((uint64_t)blockIdx.x * p.batches + b) * LOOKUP_THREADS;
    const uint64_t j = base + threadIdx.x;
    const bool active = j < p.n_f;
    uint32_t found = LOOKUP_EMPTY;
    if (active) found = lookup_find<FR>(p, j);
    unsigned long long rest = __ballot(active);
    while (rest) {
      const int lead = __ffsll((long long)rest) - 1;
      const uint32_t lf = (uint32_t)__shfl((int)found, lead);
      const unsigned long long same = __ballot(active && found == lf) & rest;
      const uint32_t amount = (uint32_t)__popcll(same);
      if (lf == LOOKUP_EMPTY) {
        if (miss == 0) miss_first = base + wave_at + (uint32_t)lead;   // the smallest: runs ascend, and so do the lanes of a run
        miss += amount;
      } else if (amount >= LOOKUP_HOT_LANES) {
        if (hot_amount && hot == lf) {
          hot_amount += amount;
        } else {
          if (hot_amount && lane == 0) lookup_credit(p, hot, 0, hot_amount);
          hot = lf;
          hot_amount = amount;
        }
      } else if (lane == (uint32_t)lead) {
        lookup_credit(p, lf, 0, amount);
      }
      rest &= ~same;
    }
  }
  if (lane == 0) {
    const uint32_t w = threadIdx.x >> 6;
    s_hot[w] = hot;
    s_amount[w] = hot_amount;
    s_miss[w] = miss;
    s_first[w] = miss_first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long gone = 0, first = ~0ull;
    for (uint32_t w = 0; w < WAVES; w++) {
      gone += s_miss[w];
      first = s_first[w] < first ? s_first[w] : first;
    }
    if (gone) lookup_credit(p, LOOKUP_EMPTY, first, (uint32_t)gone);
    for (uint32_t w = 0; w < WAVES; w++) {
      uint32_t amount = s_amount[w];
      if (!amount) continue;
      for (uint32_t v = w + 1; v < WAVES; v++)
        if (s_amount[v] && s_hot[v] == s_hot[w]) {
          amount += s_amount[v];
          s_amount[v] = 0;
        }
      lookup_credit(p, s_hot[w], 0, amount);
    }
  }
}

template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_lookup_mult(LookupMult p) {
  const uint32_t i = blockIdx.x * LOOKUP_THREADS + threadIdx.x;
  if (i < p.n) lookup_mult_elem<FR>(p, i);
}

template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_lookup_scan_up(LookupScan p) {
  __shared__ uint32_t sc[LOOKUP_THREADS];
  const uint64_t base = ((uint64_t)blockIdx.x << LOOKUP_SCAN_TILE_LOG) + LOOKUP_SCAN_RUN * threadIdx.x;
  uint32_t acc = 0;
#pragma unroll
  for (uint32_t q = 0; q < LOOKUP_SCAN_RUN; q++) acc += lookup_scan_elem(p, base + q);
  sc[threadIdx.x] = acc;
#pragma unroll 1
  for (uint32_t s = LOOKUP_THREADS / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (threadIdx.x < s) sc[threadIdx.x] += sc[threadIdx.x + s];
  }
  if (threadIdx.x == 0) p.totals[blockIdx.x] = sc[0];
}

template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_lookup_scan_down(LookupScan p) {
  __shared__ uint32_t sc[2][LOOKUP_THREADS];
  const uint64_t base = ((uint64_t)blockIdx.x << LOOKUP_SCAN_TILE_LOG) + LOOKUP_SCAN_RUN * threadIdx.x;
  uint32_t v[LOOKUP_SCAN_RUN], acc = 0;
#pragma unroll
  for (uint32_t q = 0; q < LOOKUP_SCAN_RUN; q++) {
    v[q] = acc;
    acc += lookup_scan_elem(p, base + q);
  }
  uint32_t cur = 0;
  sc[0][threadIdx.x] = acc;
#pragma unroll 1
  for (uint32_t s = 1; s < LOOKUP_THREADS; s <<= 1) {
    __syncthreads();
    uint32_t x = sc[cur][threadIdx.x];
    if (threadIdx.x >= s) x += sc[cur][threadIdx.x - s];
    cur ^= 1;
    sc[cur][threadIdx.x] = x;
  }
  __syncthreads();
  uint32_t off = p.carry ? p.carry[blockIdx.x] : 0u;
  if (threadIdx.x > 0) off += sc[cur][threadIdx.x - 1];
#pragma unroll
  for (uint32_t q = 0; q < LOOKUP_SCAN_RUN; q++)
    if (base + q < p.n) p.dst[base + q] = off + v[q];
}

template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_lookup_expand(LookupExpand p) {
  const uint64_t g = (uint64_t)blockIdx.x * LOOKUP_THREADS + threadIdx.x;
  if (g < p.total) lookup_expand_elem(p, g);
}

template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_logup_den(LogupRows p) {
  const uint64_t j = (uint64_t)blockIdx.x * LOOKUP_THREADS + threadIdx.x;
  if (j < p.n) logup_den_row<FR>(p, j);
}

template <class FR>
__global__ void __launch_bounds__(LOOKUP_THREADS) k_logup_term(LogupRows p) {
  const uint64_t j = (uint64_t)blockIdx.x * LOOKUP_THREADS + threadIdx.x;
  if (j < p.n) logup_term_row<FR>(p, j);
}
#endif

}  // namespace msm
