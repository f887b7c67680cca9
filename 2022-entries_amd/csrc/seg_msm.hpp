// seg_msm.hpp -- segmented MSM: S independent sums out[s] = sum_i scalars[i] * points[i] over the pairs of segment s, in one launch
// chain.  The big engine is built for one sum of 2^20 .. 2^26 pairs; this one for many sums of 1 to a few thousand terms (FK20 /
// PeerDAS cell proofs, short circuit columns over one SRS, IPA rounds, committee key aggregation).
//
//   digits      signed c-bit Booth digits, ceil(257 / c) of them, |d| <= 2^(c-1), digit j a function of bits [c j - 1, c j + c) alone
//               (sm_digit, the rule of pm_digit: see there; it holds for every c with c + 1 + 31 <= 64 bits in the shifted pair of
//               words, so for c <= 9 with room to spare).  The window size c comes from the segment's length (sm_window_for).
//   accumulate  a slice of 2^(c-1) lanes owns one (segment, window); lane k owns bucket k + 1.  The slice walks the segment in tiles of
//               T points: the keys (|d|, sign) of the tile go to LDS, a counting sort in LDS (LDS atomics only) lists the tile's points
//               by bucket, and every lane mixed-adds its own list into an accumulator it keeps in registers (xyzz_madd, the record
//               gathered from the caller's array).  Infinity records and zero digits never enter a list.
//   spread      before the tiles the slice finds R, the largest |digit| of its window over the segment rounded up to a power of two.
//               Where R < 2^(c-1) -- the top window of any scalar, the upper windows of scalars below r or of short challenges --
//               the pairs of digit d are dealt to the 2^(c-1) / R lanes d - 1 + R m in turn, so a window whose digits take few values
//               still keeps every lane busy instead of walking one long list; R = 0 skips the window.
//   reduce      over the slice's lanes, every lane's point in a slot of LDS: fold the spread lanes onto lanes 0 .. R - 1, then
//               sum_k k B_k as a suffix scan and a sum, at most 3 (c - 1) steps of sm_add (xyzz_add's law) with the operand read from the
//               neighbour's slot (a shuffled operand has to be whole in registers next to the lane's own point, which over Fp2 spills).
//   tail        one lane per segment: Horner over its window sums from the top, c doublings and one addition per window.
//   output      k_fb_normalize of fixed_base.hpp as it stands.
//
// No curve test and no subgroup test.  Every memory access is a function of lane index, offsets and digits alone, so a record on no
// curve gives an unspecified result but the call finishes.  The launch plan (sm_plan) is plain host code with no HIP in it.
// Every per-element step is an MSM_HD function, so the host build (host_test_api.cpp, ht_sm_*) runs the same code under MSM_CHECK.
#pragma once
#include <vector>

#include "point_mul.hpp"   // pm_load_point; fixed_base.hpp, check_scalar_word, CheckConsts, fr_from_montgomery through it

namespace msm {

constexpr uint32_t SM_MAX_WINDOW = 9;
constexpr uint32_t SM_MIN_TILE = 64, SM_MAX_TILE = 4096, SM_DEFAULT_TILE = 1024;
constexpr uint32_t SM_LDS_HEADER = 16;           // words in front of the slices: the block's tile count, then the largest |digit| per slice
constexpr uint32_t SM_LDS_BUDGET = 20u << 10;    // bytes of LDS a block's sort area may take: eight one-wave blocks share a CU's 160 KiB

MSM_HD uint32_t sm_digits(uint32_t c) { return (257 + c - 1) / c; }
MSM_HD uint32_t sm_buckets(uint32_t c) { return 1u << (c - 1); }
// slices of 2^(c-1) lanes per block (at most eight share a wave), and the block's lanes
MSM_HD uint32_t sm_slices(uint32_t c) {
  const uint32_t b = sm_buckets(c);
  return b >= 64 ? 1 : (64 / b < 8 ? 64 / b : 8);
}
MSM_HD uint32_t sm_block_threads(uint32_t c) { return sm_buckets(c) < 64 ? 64 : sm_buckets(c); }
// pairs of the tile that starts at `base` in a segment of len pairs (0 behind its end)
MSM_HD uint32_t sm_tile_len(uint64_t len, uint64_t base, uint32_t tile) { return base < len ? (len - base < tile ? (uint32_t)(len - base) : tile) : 0u; }
// where segment `seg` of a call lies: its first point, its first scalar, its pairs.  General form: offs[seg], offs[seg + 1] bound
// both; shared form (offs NULL): every segment reads the points from 0 and row seg0 + seg of the scalars.
MSM_HD void sm_segment_span(uint64_t& pt0, uint64_t& sc0, uint64_t& len, const uint64_t* offs, uint64_t seg, uint64_t shared_len, uint64_t seg0) {
  if (offs) {
    pt0 = offs[seg];
    len = offs[seg + 1] - pt0;
    sc0 = pt0;
  } else {
    pt0 = 0;
    len = shared_len;
    sc0 = (seg0 + seg) * shared_len;
  }
}

// Booth's rule on the c + 1 bits b(c j - 1) .. b(c j + c - 1) at the bottom of v
MSM_HD int32_t sm_booth(uint64_t v, uint32_t c) {
  const uint32_t t = (uint32_t)v & ((2u << c) - 1);
  return (int32_t)((t + 1) >> 1) - (int32_t)(((t >> c) & 1) << c);
}
// signed digit j of the scalar for window size c <= 9, the scalar in registers (words by uniform selects) ...
MSM_HD int32_t sm_digit(const uint32_t (&s)[8], uint32_t j, uint32_t c) {
  if (j == 0) return sm_booth((uint64_t)s[0] << 1, c);
  const uint32_t bit = j * c - 1, wi = bit >> 5, sh = bit & 31;
  const uint32_t lo = check_scalar_word<8>(s, (int)wi), hi = check_scalar_word<8>(s, (int)wi + 1);   // word 8 and up do not exist: 0
  return sm_booth((((uint64_t)hi << 32) | lo) >> sh, c);
}
// ... and in memory: only the two words the window lies in are read
MSM_HD int32_t sm_digit_mem(const uint32_t* s, uint32_t j, uint32_t c) {
  if (j == 0) return sm_booth((uint64_t)s[0] << 1, c);
  const uint32_t bit = j * c - 1, wi = bit >> 5, sh = bit & 31;
  const uint32_t lo = wi < 8 ? s[wi] : 0u, hi = wi + 1 < 8 ? s[wi + 1] : 0u;
  return sm_booth((((uint64_t)hi << 32) | lo) >> sh, c);
}

// the sort key of one pair in window j: (|d| << 1) | (d < 0), 0 when the pair adds nothing (a zero digit)
template <class FR>
MSM_HD uint32_t sm_key(const uint32_t* sc, uint32_t j, uint32_t c, bool from_mont) {
  int32_t d;
  if (from_mont) {
    uint32_t s[8];
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = sc[k];
    fr_from_montgomery<FR>(s);
    d = sm_digit(s, j, c);
  } else {
    d = sm_digit_mem(sc, j, c);
  }
  const uint32_t a = d < 0 ? (uint32_t)-d : (uint32_t)d;
  return a ? (a << 1) | (d < 0 ? 1u : 0u) : 0u;
}

// acc += (+/-) the record at `rec` (an Affine image the sort has found finite)
template <class E>
MSM_HD void sm_bucket_add(XyzzT<typename E::T>& acc, const uint8_t* rec, bool negate, const typename E::Md& md) {
  constexpr int W = E::WORDS;
  uint32_t w[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; k++) w[k] = reinterpret_cast<const uint32_t*>(rec)[k];
  AffineT<typename E::T> P;
  pm_load_point<E>(P, w, md);
  xyzz_madd<E>(acc, P, negate, false, md);
}

// the digit range a slice runs with: the largest |digit| seen, rounded up to a power of two (0: no pair adds anything)
MSM_HD uint32_t sm_digit_range(uint32_t maxd) {
  uint32_t r = maxd ? 1u : 0u;
  while (r < maxd) r <<= 1;
  return r;
}
// the lane of a pair with |digit| a in [1, R], the i-th of its tile: the lanes a - 1 + R m, m < B / R, in turn
MSM_HD uint32_t sm_lane_of(uint32_t a, uint32_t i, uint32_t R, uint32_t B) { return a - 1 + R * (i & (B / R - 1)); }
// the steps of the reduction over a slice of B lanes, lane k < R of the folded slice holding bucket k + 1:
//   fold   for off = B / 2, .. R:        S_k += S_(k + off) where k < off                 ->  S_k = sum_m S_(k + R m), k < R
//   (lanes k >= R then stand for infinity)
//   scan   for off = 1, 2, .. < R:       S_k += S_(k + off) where k + off < R             ->  S_k = sum_(R > m >= k) B_m
//   sum    for off = R / 2, .. 1:        S_k += S_(k + off) where k < off                 ->  S_0 = sum_k S_k = sum_m (m + 1) B_m
// Every slice of a block walks all 3 log2(B) steps (the barriers are the block's); the predicates say who adds.
MSM_HD bool sm_fold_takes(uint32_t k, uint32_t off, uint32_t R) { return R != 0 && off >= R && k < off; }
MSM_HD bool sm_scan_takes(uint32_t k, uint32_t off, uint32_t R) { return k + off < R; }
MSM_HD bool sm_sum_takes(uint32_t k, uint32_t off, uint32_t R) { return 2 * off <= R && k < off; }

// acc += b: xyzz_add (add-2008-s) operation for operation, so with its limb bounds.  What differs is what has to stay in registers:
// the caller has stored the lane's own point at `self` before the call, so its X and Y need not outlive the same-x test -- the
// doubling re-reads them -- and the addend is read from memory coordinate by coordinate.  Over Fp2 that is the difference between one
// lane's addition fitting the register file and spilling (xyzz_madd_common re-reads its base for the same reason).
// sm_add_common returns 0 when acc holds the sum, 1 when the sum is the double of the point, 2 when it is infinity.  In both
// rare cases acc still holds its value, but nothing after the same-x test reads its X and Y, so they need not stay in registers: the
// caller takes the point from `self` again.
MSM_HD void sm_fence() { asm volatile("" ::: "memory"); }   // (as h2c_fence: a coordinate is fetched where it is used, not hoisted ahead of the products)
template <class T>
MSM_HD T sm_fetch(const T& m) {
  sm_fence();
  const T v = m;
  sm_fence();
  return v;
}
template <class E>
MSM_HD int sm_add_common(XyzzT<typename E::T>& acc, const XyzzT<typename E::T>& b, const typename E::Md& md) {
  typename E::T u1, u2, s1, s2, P, R, PP;
  E::template mul_c<false>(u1, acc.x, sm_fetch(b.zz), md);
  E::template mul_c<false>(u2, sm_fetch(b.x), acc.zz, md);
  E::template mul_c<false>(s1, acc.y, sm_fetch(b.zzz), md);
  E::template mul_c<false>(s2, sm_fetch(b.y), acc.zzz, md);
  E::sub(P, u2, u1, E::Fld::BIAS2_28);  // (0, 4p), limbs < 3*2^28
  E::sub(R, s2, s1, E::Fld::BIAS2_28);
  E::prep(P);
  E::sqr_c(PP, P, md);
  if (E::is_zero_M(PP)) {
    typename E::T r2;
    E::sqr(r2, R, md);
    return E::is_zero_M(r2) ? 1 : 2;
  }
  typename E::T x3, y3, ppp, t;
  add_tail<E>(x3, y3, ppp, P, R, PP, u1, s1, md);
  acc.x = x3;
  acc.y = y3;
  E::template mul_c<false>(t, acc.zz, sm_fetch(b.zz), md);
  E::template mul_c<false>(acc.zz, t, PP, md);
  E::template mul_c<false>(t, acc.zzz, sm_fetch(b.zzz), md);
  E::template mul_c<false>(acc.zzz, t, ppp, md);
  return 0;
}
template <class E>
MSM_HD void sm_add(XyzzT<typename E::T>& acc, const XyzzT<typename E::T>& b, const XyzzT<typename E::T>& self, const typename E::Md& md) {
  if (xyzz_is_inf<E>(b)) return;
  if (xyzz_is_inf<E>(acc)) {
    acc = b;
    return;
  }
  const int rare = sm_add_common<E>(acc, b, md);
  if (rare == 1) {
    acc = self;
    xyzz_dbl<E>(acc, md);
  } else if (rare == 2) {
    xyzz_set_inf<E>(acc);
  }
}

// acc = sum_j 2^(c j) wsum[j * pitch], from the top window; *slot: memory of the lane's own for the running point (sm_add)
template <class E>
MSM_HD void sm_tail(XyzzT<typename E::T>& acc, const XyzzT<typename E::T>* wsum, size_t pitch, uint32_t nwin, uint32_t c, XyzzT<typename E::T>* slot,
                    const typename E::Md& md) {
  xyzz_set_inf<E>(acc);
#pragma unroll 1
  for (int j = (int)nwin - 1; j >= 0; j--) {
    if (!xyzz_is_inf<E>(acc)) {
#pragma unroll 1
      for (uint32_t k = 0; k < c; k++) xyzz_dbl<E>(acc, md);
    }
    *slot = acc;
    sm_add<E>(acc, wsum[(size_t)j * pitch], *slot, md);
  }
}

// ---- the launch plan: host code, no HIP ----------------------------------------------------------------------------------------
// Window size for a segment of len pairs.  The count behind it, in point additions on the lanes a (segment, window) occupies:
// ceil(257 / c) windows, each 2^(c-1) lanes for (len / 2^(c-1) + 2 (c - 1)) additions, so cost(c) = ceil(257 / c) (len + 2^c (c - 1));
// neighbouring sizes cross at len = 272, 789, 2442, 7680, 14912, rounded here.  (Below c = 4 a slice fills less than an eighth of a
// wave: 1..3 are test hooks.)
inline uint32_t sm_window_for(uint64_t len) {
  if (len <= 256) return 4;
  if (len <= 768) return 5;
  if (len <= 2560) return 6;
  if (len <= 8192) return 7;
  if (len <= 16384) return 8;
  return 9;
}
// LDS words of a block: per slice the counts, the cursors, the list and the 16-bit keys of a tile; or, for the reduction, one point
// per lane, whichever is larger
inline uint32_t sm_lds_words(uint32_t c, uint32_t tile, uint32_t xyzz_words) {
  const uint32_t b = sm_buckets(c), sort = sm_slices(c) * (tile + tile / 2 + 2 * b);
  const uint32_t xch = sm_block_threads(c) * xyzz_words;
  return SM_LDS_HEADER + (sort > xch ? sort : xch);
}
// the tile a class runs with: no longer than its longest segment needs, and within the LDS budget
inline uint32_t sm_tile_for(uint32_t c, uint32_t tile_opt, uint64_t maxlen) {
  uint32_t t = tile_opt ? tile_opt : SM_DEFAULT_TILE;
  while (t > SM_MIN_TILE && t / 2 >= maxlen) t /= 2;
  while (t > SM_MIN_TILE && (size_t)4 * sm_lds_words(c, t, 0) > SM_LDS_BUDGET) t /= 2;
  return t;
}

struct SmClass {
  uint32_t c, nwin, tile, nseg;
  size_t ids_at;    // its segments: ids[ids_at .. ids_at + nseg) of the chunk, chunk-local indices
  size_t wsum_at;   // its window sums: records [wsum_at, wsum_at + nwin * nseg) of the chunk's buffer, [window * nseg + k]
};
struct SmChunk {
  size_t s0 = 0, s1 = 0;          // segments [s0, s1)
  std::vector<SmClass> classes;   // the non-empty segments by window size
  std::vector<uint32_t> ids;
  size_t wsum_records = 0, work_bytes = 0;
};
struct SmPlan {
  std::vector<SmChunk> chunks;
  size_t max_segs = 0, max_wsum_records = 0;
  bool fits = true;   // false: one segment alone exceeds the work limit
};

// work memory one segment of window size c takes: its window sums, its result slot, its prefix element, its id
inline size_t sm_seg_work(uint32_t c, size_t xyzz_bytes, size_t el_bytes) { return (size_t)sm_digits(c) * xyzz_bytes + xyzz_bytes + el_bytes + 4; }

// offsets: nseg + 1 values (general form), or NULL with every segment shared_len long.  force_c 0 = by length; max_segs 0 = by the
// work limit alone.
inline void sm_plan(SmPlan& plan, const uint64_t* offsets, size_t nseg, uint64_t shared_len, uint32_t force_c, uint32_t tile_opt, size_t max_segs,
                    size_t work_limit, size_t xyzz_bytes, size_t el_bytes) {
  plan = SmPlan();
  size_t s = 0;
  while (s < nseg) {
    SmChunk ch;
    ch.s0 = s;
    std::vector<uint32_t> cs;   // window size per segment of the chunk, 0 = empty
    while (s < nseg && (max_segs == 0 || s - ch.s0 < max_segs) && s - ch.s0 < 0x7fffffffu) {
      const uint64_t len = offsets ? offsets[s + 1] - offsets[s] : shared_len;
      const uint32_t c = len == 0 ? 0 : (force_c ? force_c : sm_window_for(len));
      const size_t need = c ? sm_seg_work(c, xyzz_bytes, el_bytes) : xyzz_bytes + el_bytes + 4;
      if (ch.work_bytes + need > work_limit) {
        if (s == ch.s0) plan.fits = false;
        break;
      }
      ch.work_bytes += need;
      cs.push_back(c);
      s++;
    }
    if (!plan.fits) return;
    ch.s1 = s;
    for (uint32_t c = 1; c <= SM_MAX_WINDOW; c++) {
      SmClass k{c, sm_digits(c), 0, 0, ch.ids.size(), ch.wsum_records};
      uint64_t maxlen = 0;
      for (size_t i = 0; i < cs.size(); i++) {
        if (cs[i] != c) continue;
        const uint64_t len = offsets ? offsets[ch.s0 + i + 1] - offsets[ch.s0 + i] : shared_len;
        maxlen = len > maxlen ? len : maxlen;
        ch.ids.push_back((uint32_t)i);
        k.nseg++;
      }
      if (!k.nseg) continue;
      k.tile = sm_tile_for(c, tile_opt, maxlen);
      ch.wsum_records += (size_t)k.nwin * k.nseg;
      ch.classes.push_back(k);
    }
    plan.max_segs = cs.size() > plan.max_segs ? cs.size() : plan.max_segs;
    plan.max_wsum_records = ch.wsum_records > plan.max_wsum_records ? ch.wsum_records : plan.max_wsum_records;
    plan.chunks.push_back(std::move(ch));
  }
}

// ---- the whole of one segment, serially: what the kernels below compute, lane by lane (host build, tests) ------------------
// points: Affine images `stride` bytes apart; scalars: 8 words each.  The sort of a tile is a counting sort like the kernel's, in
// index order.
template <class E>
inline void sm_serial_segment(XyzzT<typename E::T>& out, const uint8_t* points, size_t stride, const uint32_t* scalars, uint64_t len, uint32_t c, uint32_t tile,
                              bool from_mont, const typename E::Md& md) {
  using X = XyzzT<typename E::T>;
  using FR = typename CheckConsts<E>::FR;
  const uint32_t nwin = sm_digits(c), B = sm_buckets(c);
  std::vector<X> wsum(nwin), bucket(B), nxt(B);
  std::vector<uint32_t> cnt(B), cur(B), list(tile), keys(tile);
  for (uint32_t win = 0; win < nwin; win++) {
    for (uint32_t k = 0; k < B; k++) xyzz_set_inf<E>(bucket[k]);
    uint32_t maxd = 0;
    for (uint64_t i = 0; i < len; i++) {
      const uint32_t key = points[i * stride + 8 * E::WORDS] ? 0u : sm_key<FR>(scalars + 8 * i, win, c, from_mont);
      maxd = (key >> 1) > maxd ? (key >> 1) : maxd;
    }
    const uint32_t R = sm_digit_range(maxd);
    for (uint64_t base = 0; R && base < len; base += tile) {
      const uint32_t tl = sm_tile_len(len, base, tile);
      for (uint32_t k = 0; k < B; k++) cnt[k] = 0;
      for (uint32_t i = 0; i < tl; i++) {
        const uint8_t flag = points[(base + i) * stride + 8 * E::WORDS];
        keys[i] = flag ? 0u : sm_key<FR>(scalars + 8 * (base + i), win, c, from_mont);
        if (keys[i]) cnt[sm_lane_of(keys[i] >> 1, i, R, B)]++;
      }
      uint32_t run = 0;
      for (uint32_t k = 0; k < B; k++) {
        cur[k] = run;
        run += cnt[k];
      }
      for (uint32_t i = 0; i < tl; i++)
        if (keys[i]) list[cur[sm_lane_of(keys[i] >> 1, i, R, B)]++] = (i << 1) | (keys[i] & 1);
      for (uint32_t k = 0; k < B; k++)
        for (uint32_t e = cur[k] - cnt[k]; e < cur[k]; e++) sm_bucket_add<E>(bucket[k], points + (base + (list[e] >> 1)) * stride, (list[e] & 1) != 0, md);
    }
    // the reduction as the lanes run it: every step reads what the step before left
    X* S = bucket.data();
    for (uint32_t off = B >> 1; off >= 1; off >>= 1) {
      for (uint32_t k = 0; k < B; k++) nxt[k] = S[k];
      for (uint32_t k = 0; k < B; k++)
        if (sm_fold_takes(k, off, R)) sm_add<E>(S[k], nxt[k + off], nxt[k], md);
    }
    for (uint32_t k = R; k < B; k++) xyzz_set_inf<E>(S[k]);
    for (uint32_t off = 1; off < B; off <<= 1) {
      for (uint32_t k = 0; k < B; k++) nxt[k] = S[k];
      for (uint32_t k = 0; k < B; k++)
        if (sm_scan_takes(k, off, R)) sm_add<E>(S[k], nxt[k + off], nxt[k], md);
    }
    for (uint32_t off = B >> 1; off >= 1; off >>= 1) {
      for (uint32_t k = 0; k < B; k++) nxt[k] = S[k];
      for (uint32_t k = 0; k < B; k++)
        if (sm_sum_takes(k, off, R)) sm_add<E>(S[k], nxt[k + off], nxt[k], md);
    }
    wsum[win] = S[0];
  }
  X slot;
  sm_tail<E>(out, wsum.data(), 1, nwin, c, &slot, md);
}

#if defined(__HIPCC__)
// the arguments of one class's launch
struct SmLaunch {
  const uint8_t* points;
  size_t stride;
  const uint32_t* scalars;
  const uint64_t* offs;   // general form: offs[s], offs[s + 1] bound segment s of the chunk; NULL: the shared form
  const uint32_t* ids;    // the class's segments, chunk-local; NULL: segment k is k
  uint64_t shared_len, shared_seg0;   // shared form: pairs per segment, and the chunk's first segment in the call
  uint32_t nseg, c, nwin, tile, from_mont;
};

// One block: sm_slices(c) slices of 2^(c-1) lanes, slice i of block b owning item b * slices + i = segment-of-class * nwin + window.
// Every lane runs to the end (the barriers and the shuffles want whole waves); a lane without an item has an empty segment.
template <class E>
__global__ void __launch_bounds__(256) k_sm_accumulate(const SmLaunch a, XyzzDevT<typename E::T>* __restrict__ wsum) {
  using El = typename E::T;
  using FR = typename CheckConsts<E>::FR;
  extern __shared__ uint32_t sm_lds[];
  const uint32_t c = a.c, B = sm_buckets(c), T = a.tile;
  const uint32_t slices = sm_slices(c);
  const uint32_t k = threadIdx.x & (B - 1), sl = threadIdx.x >> (c - 1);
  const bool live = sl < slices;   // (c < 4: the lanes behind the eighth slice idle)
  const uint64_t item = (uint64_t)blockIdx.x * slices + sl;
  const bool active = live && item < (uint64_t)a.nseg * a.nwin;
  uint32_t* cnt = sm_lds + SM_LDS_HEADER + (live ? sl : 0u) * (T + T / 2 + 2 * B);
  uint32_t* cur = cnt + B;
  uint32_t* list = cur + B;
  uint16_t* keys = reinterpret_cast<uint16_t*>(list + T);
  uint32_t segk = 0, win = 0;
  uint64_t pt0 = 0, sc0 = 0, len = 0;
  if (active) {
    segk = (uint32_t)(item / a.nwin);
    win = (uint32_t)(item % a.nwin);
    const uint32_t seg = a.ids ? a.ids[segk] : segk;
    sm_segment_span(pt0, sc0, len, a.offs, seg, a.shared_len, a.shared_seg0);
  }
  // the digit range of the slice's window over its whole segment
  if (threadIdx.x < SM_LDS_HEADER) sm_lds[threadIdx.x] = 0;
  __syncthreads();
  {
    uint32_t maxd = 0;
#pragma unroll 1
    for (uint64_t i = k; i < len; i += B) {
      const uint8_t flag = a.points[(pt0 + i) * a.stride + 8 * E::WORDS];
      const uint32_t key = flag ? 0u : sm_key<FR>(a.scalars + 8 * (sc0 + i), win, c, a.from_mont != 0);
      maxd = (key >> 1) > maxd ? (key >> 1) : maxd;
    }
    if (maxd) atomicMax(&sm_lds[4 + sl], maxd);
  }
  __syncthreads();
  const uint32_t R = live ? sm_digit_range(sm_lds[4 + sl]) : 0u;
  if (R == 0) len = 0;
  if (active && k == 0) atomicMax(&sm_lds[0], (uint32_t)((len + T - 1) / T));
  __syncthreads();
  const uint32_t ntiles = sm_lds[0];

  typename E::Md md;
  XyzzT<El> acc;
  xyzz_set_inf<E>(acc);
#pragma unroll 1
  for (uint32_t t = 0; t < ntiles; t++) {
    const uint64_t base = (uint64_t)t * T;
    const uint32_t tl = sm_tile_len(len, base, T);
    if (live) cnt[k] = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t i = k; i < tl; i += B) {
      const uint8_t flag = a.points[(pt0 + base + i) * a.stride + 8 * E::WORDS];
      const uint32_t key = flag ? 0u : sm_key<FR>(a.scalars + 8 * (sc0 + base + i), win, c, a.from_mont != 0);
      keys[i] = (uint16_t)key;
      if (key) atomicAdd(&cnt[sm_lane_of(key >> 1, i, R, B)], 1u);
    }
    __syncthreads();
    uint32_t start = 0;
#pragma unroll 1
    for (uint32_t m = 0; m < B; m++) {
      const uint32_t v = cnt[m];
      start += m < k ? v : 0u;
    }
    const uint32_t mine = live ? cnt[k] : 0u;
    if (live) cur[k] = start;
    __syncthreads();
#pragma unroll 1
    for (uint32_t i = k; i < tl; i += B) {
      const uint32_t key = keys[i];
      if (key) list[atomicAdd(&cur[sm_lane_of(key >> 1, i, R, B)], 1u)] = (i << 1) | (key & 1);
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t e = 0; e < mine; e++) {
      const uint32_t ent = list[start + e];
      sm_bucket_add<E>(acc, a.points + (pt0 + base + (ent >> 1)) * a.stride, (ent & 1) != 0, md);
    }
    __syncthreads();
  }

  // sum_k (k + 1) B_k over the slice.  Every lane of the block has a slot in LDS (the sort area is dead by now); the addend is
  // read from its slot coordinate by coordinate, so only the lane's own point is held in registers across an addition.
  XyzzT<El>* xch = reinterpret_cast<XyzzT<El>*>(sm_lds + SM_LDS_HEADER);
#pragma unroll 1
  for (uint32_t off = B >> 1; off >= 1; off >>= 1) {
    xch[threadIdx.x] = acc;
    __syncthreads();
    if (live && sm_fold_takes(k, off, R)) sm_add<E>(acc, xch[threadIdx.x + off], xch[threadIdx.x], md);
    __syncthreads();
  }
  if (k >= R) xyzz_set_inf<E>(acc);
#pragma unroll 1
  for (uint32_t off = 1; off < B; off <<= 1) {
    xch[threadIdx.x] = acc;
    __syncthreads();
    if (live && sm_scan_takes(k, off, R)) sm_add<E>(acc, xch[threadIdx.x + off], xch[threadIdx.x], md);
    __syncthreads();
  }
#pragma unroll 1
  for (uint32_t off = B >> 1; off >= 1; off >>= 1) {
    xch[threadIdx.x] = acc;
    __syncthreads();
    if (live && sm_sum_takes(k, off, R)) sm_add<E>(acc, xch[threadIdx.x + off], xch[threadIdx.x], md);
    __syncthreads();
  }
  if (active && k == 0) wsum[(size_t)win * a.nseg + segk].p = acc;
}

// one lane per segment of a class: its window sums [window * nseg + k] -> stage[ids[k]]
template <class E>
__global__ void __launch_bounds__(64) k_sm_tail(const XyzzDevT<typename E::T>* __restrict__ wsum, const uint32_t* __restrict__ ids, uint32_t nseg, uint32_t nwin,
                                                uint32_t c, XyzzDevT<typename E::T>* __restrict__ stage) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= nseg) return;
  typename E::Md md;
  XyzzDevT<typename E::T>* slot = stage + (ids ? ids[i] : i);   // (the result's slot holds the running point between windows)
  XyzzDevT<typename E::T> o;
  sm_tail<E>(o.p, reinterpret_cast<const XyzzT<typename E::T>*>(wsum + i), nseg, nwin, c, &slot->p, md);
  *slot = o;
}
#endif

}  // namespace msm
