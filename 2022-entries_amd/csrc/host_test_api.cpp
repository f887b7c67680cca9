// host_test_api.cpp -- builds libmsm_hosttest.so (plain g++, no HIP): the SAME fp28/curve templates the
// kernels use, compiled for the host with the limb-bound checker (MSM_CHECK) armed.  tests/ drive it
// through ctypes against oracle/pymodel.py.  It is test scaffolding for the arithmetic, not a product
// path: nothing in the engine or the C ABI links it.
#include <stdint.h>
#include <stdio.h>

static long g_check_failures = 0;
static char g_first_failure[256];
static void msm_check_fail(const char* file, int line, const char* cond) {
  if (g_check_failures++ == 0) snprintf(g_first_failure, sizeof g_first_failure, "%s:%d %s", file, line, cond);
}
#define MSM_CHECK(cond) do { if (!(cond)) msm_check_fail(__FILE__, __LINE__, #cond); } while (0)
#define MSM_CHECK_COL_BEGIN() unsigned __int128 chk_col_ = col
#define MSM_CHECK_COL_ADD(x) chk_col_ += (x)
#define MSM_CHECK_COL_END(col) MSM_CHECK(chk_col_ == (unsigned __int128)(col))

#include "host_curve.hpp"
#include "te.hpp"

using namespace msm;

// ---- base-field primitives (curve ids 0/1 select the modulus) ------------------------------------------------
template <class F>
static void t_fe_mul(const uint8_t* a, const uint8_t* b, uint8_t* out) {
  Modulus<F> md;
  Fe x, y, z;
  uint32_t wa[12], wb[12], wo[12];
  memcpy(wa, a, 48);
  memcpy(wb, b, 48);
  fe_from_abi<F>(x, wa, md);
  fe_from_abi<F>(y, wb, md);
  fe_mul<F>(z, x, y, md);
  fe_to_abi<F>(wo, z, md);
  memcpy(out, wo, 48);
}

template <class F>
static void t_fe_sqr(const uint8_t* a, uint8_t* out) {
  Modulus<F> md;
  Fe x, z;
  uint32_t wa[12], wo[12];
  memcpy(wa, a, 48);
  fe_from_abi<F>(x, wa, md);
  fe_sqr<F>(z, x, md);
  fe_to_abi<F>(wo, z, md);
  memcpy(out, wo, 48);
}

// worst-case limbs for the column bounds: every limb at the largest value a multiply may see; only the checker matters
template <class F>
static void t_fe_extreme(int) {
  Modulus<F> md;
  Fe x, z;
  for (int i = 0; i < NL - 1; i++) x.v[i] = (1u << 30) - 1;
  x.v[NL - 1] = F::P[NL - 1] * 16;  // keeps the VALUE below 32p while every other limb sits at its bound
  fe_mul<F>(z, x, x, md);
  fe_sqr<F>(z, x, md);
  Fe y;
  for (int i = 0; i < NL - 1; i++) y.v[i] = (1u << 29) - 1;
  y.v[NL - 1] = F::P[NL - 1] * 8;
  fe_mul2<F>(z, y, y, y, y, md);
}

// k * a for small k through lazy limbs, then the weak reduction: out = canonical(k * a)
template <class F>
static void t_fe_weak_reduce(const uint8_t* a, int k, uint8_t* out) {
  Modulus<F> md;
  Fe x, z;
  uint32_t wa[12], wo[12];
  memcpy(wa, a, 48);
  fe_from_abi<F>(x, wa, md);
  fe_reduce<F>(x);
  // k = k1 * k2 (k1 <= 7, k2 <= 4) through lazy limbs: multiply, parallel carry, multiply again -> limbs < 2^31
  const int k1 = k > 7 ? 7 : k, k2 = k / k1;
  for (int i = 0; i < NL; i++) z.v[i] = x.v[i] * (uint32_t)k1;
  fe_carry(z);
  for (int i = 0; i < NL; i++) z.v[i] *= (uint32_t)k2;
  fe_weak_reduce<F>(z);
  Fe three_p;  // result must be < 3p
  for (int i = 0; i < NL; i++) three_p.v[i] = F::P[i] * 3;
  fe_normalize(three_p);
  MSM_CHECK(!fe_geq(z, three_p.v));
  fe_to_abi<F>(wo, z, md);
  memcpy(out, wo, 48);
}

template <class F>
static void t_fe_roundtrip(const uint8_t* a, uint8_t* out) {
  Modulus<F> md;
  Fe x;
  uint32_t wa[12], wo[12];
  memcpy(wa, a, 48);
  fe_from_abi<F>(x, wa, md);
  fe_to_abi<F>(wo, x, md);
  memcpy(out, wo, 48);
}

template <class F>
static void t_fe_inv(const uint8_t* a, uint8_t* out) {
  Modulus<F> md;
  Fe x, y;
  uint32_t wa[12], wo[12];
  memcpy(wa, a, 48);
  fe_from_abi<F>(x, wa, md);
  fe_inv<F>(y, x, md);
  fe_to_abi<F>(wo, y, md);
  memcpy(out, wo, 48);
}

// ---- coordinate-field and curve level (curve ids 0/1/2 = 377 G1, 381 G1, 377 G2) -----------------------------
template <class C>
static void t_el_mul(const uint8_t* a, const uint8_t* b, uint8_t* out) {
  using E = typename C::E;
  typename E::Md md;
  typename E::T x, y, z;
  uint32_t wa[E::WORDS], wb[E::WORDS], wo[E::WORDS];
  memcpy(wa, a, 4 * E::WORDS);
  memcpy(wb, b, 4 * E::WORDS);
  E::from_abi(x, wa, md);
  E::from_abi(y, wb, md);
  E::mul(z, x, y, md);
  E::to_abi(wo, z, md);
  memcpy(out, wo, 4 * E::WORDS);
}

template <class C>
static void t_el_inv(const uint8_t* a, uint8_t* out) {
  using E = typename C::E;
  typename E::Md md;
  typename E::T x, z;
  uint32_t wa[E::WORDS], wo[E::WORDS];
  memcpy(wa, a, 4 * E::WORDS);
  E::from_abi(x, wa, md);
  el_inv(z, x, md, (E*)nullptr);
  E::to_abi(wo, z, md);
  memcpy(out, wo, 4 * E::WORDS);
}

// acc = inf; for each i: acc += (+/-) points[i] (mixed add); out = normalised projective.
template <class C>
static void t_madd_chain(const uint8_t* pts, size_t stride, const uint8_t* neg, size_t n, uint8_t* out) {
  using E = typename C::E;
  typename E::Md md;
  XyzzT<typename E::T> acc;
  xyzz_set_inf<E>(acc);
  for (size_t i = 0; i < n; i++) {
    AffineT<typename E::T> p;
    if (affine_from_abi<E>(p, pts + i * stride, md)) continue;
    xyzz_madd<E>(acc, p, neg[i] != 0, false, md);
  }
  xyzz_to_projective_abi<E>(out, acc, md);
}

// out = (chain over first na points) + (chain over the remaining nb points), through the full XYZZ add.
template <class C>
static void t_add_chains(const uint8_t* pts, size_t stride, size_t na, size_t nb, uint8_t* out) {
  using E = typename C::E;
  typename E::Md md;
  XyzzT<typename E::T> a, b;
  xyzz_set_inf<E>(a);
  xyzz_set_inf<E>(b);
  for (size_t i = 0; i < na + nb; i++) {
    AffineT<typename E::T> p;
    if (affine_from_abi<E>(p, pts + i * stride, md)) continue;
    xyzz_madd<E>(i < na ? a : b, p, false, false, md);
  }
  xyzz_add<E>(a, b, md);
  xyzz_to_projective_abi<E>(out, a, md);
}

// sum k_i P_i by per-point double-and-add (XYZZ dbl + XYZZ add), then one running total.
template <class C>
static void t_msm_naive(const uint8_t* pts, size_t stride, const uint8_t* scalars, size_t n, uint8_t* out) {
  using E = typename C::E;
  typename E::Md md;
  XyzzT<typename E::T> total;
  xyzz_set_inf<E>(total);
  for (size_t i = 0; i < n; i++) {
    AffineT<typename E::T> p;
    if (affine_from_abi<E>(p, pts + i * stride, md)) continue;
    const uint8_t* k = scalars + 32 * i;
    XyzzT<typename E::T> r;
    xyzz_set_inf<E>(r);
    for (int bit = 255; bit >= 0; bit--) {
      if (!xyzz_is_inf<E>(r)) xyzz_dbl<E>(r, md);
      if ((k[bit >> 3] >> (bit & 7)) & 1) xyzz_madd<E>(r, p, false, false, md);
    }
    xyzz_add<E>(total, r, md);
  }
  xyzz_to_projective_abi<E>(out, total, md);
}

// projective (Jacobian, any Z) -> normalised projective, through XYZZ.
template <class C>
static void t_normalize(const uint8_t* in, uint8_t* out) {
  using E = typename C::E;
  typename E::Md md;
  XyzzT<typename E::T> a;
  xyzz_from_projective_abi<E>(a, in, md);
  xyzz_to_projective_abi<E>(out, a, md);
}

// ---- twisted-Edwards image of BLS12-377 G1 (te.hpp) ------------------------------------------------------------
using TF = Bls12_377_Fq;   // the shape the birational map runs in (14 x 28)
using TEF = TeFq;          // the shape the law runs in (13 x 29 unless built with -DMSM_TE_LIMBS29=0): te.hpp

// arkworks Affine image -> TE base record; false when the point has no image (or is flagged infinite).
static bool te_map_host(TeAffine& out, const uint8_t* img, const Modulus<TF>& md) {
  using E = FpEl<TF>;
  Affine p;
  if (affine_from_abi<E>(p, img, md)) return false;
  fe_reduce<TF>(p.x);
  fe_reduce<TF>(p.y);
  Fe u, v, w, den, inv;
  te_map_prepare<TF>(u, v, w, den, p, md);
  if (fe_is_zero_slow<TF>(den)) return false;
  fe_inv<TF>(inv, den, md);
  te_map_finish<TF>(out, u, v, w, inv, md);
  return true;
}

static int te_finish_host(uint8_t* out, const Xyzz& acc_te, const Modulus<TF>& md) {
  if (te_failed<TEF>(acc_te)) return 2;
  Xyzz sw, acc;
  te_point_to_28<TEF>(acc, acc_te, md);
  te_to_sw<TF>(sw, acc, md);
  xyzz_to_projective_abi<FpEl<TF>>(out, sw, md);
  return 0;
}

#define DISPATCH_F(curve, fn, ...)                        \
  switch (curve) {                                        \
    case 0: fn<Bls12_377_Fq>(__VA_ARGS__); return 0;      \
    case 1: fn<Bls12_381_Fq>(__VA_ARGS__); return 0;      \
    default: return -1;                                   \
  }
#define DISPATCH_C(curve, fn, ...)                        \
  switch (curve) {                                        \
    case 0: fn<Bls12_377_G1>(__VA_ARGS__); return 0;      \
    case 1: fn<Bls12_381_G1>(__VA_ARGS__); return 0;      \
    case 2: fn<Bls12_377_G2>(__VA_ARGS__); return 0;      \
    case 3: fn<Bls12_381_G2>(__VA_ARGS__); return 0;      \
    default: return -1;                                   \
  }

extern "C" {
long ht_check_failures(void) { return g_check_failures; }
const char* ht_first_failure(void) { return g_first_failure; }
void ht_reset_checks(void) { g_check_failures = 0; g_first_failure[0] = 0; }
int ht_fe_mul(int curve, const uint8_t* a, const uint8_t* b, uint8_t* out) { DISPATCH_F(curve, t_fe_mul, a, b, out) }
int ht_fe_sqr(int curve, const uint8_t* a, uint8_t* out) { DISPATCH_F(curve, t_fe_sqr, a, out) }
int ht_fe_extreme(int curve) { DISPATCH_F(curve, t_fe_extreme, 0) }
int ht_fe_weak_reduce(int curve, const uint8_t* a, int k, uint8_t* out) { DISPATCH_F(curve, t_fe_weak_reduce, a, k, out) }
int ht_fe_roundtrip(int curve, const uint8_t* a, uint8_t* out) { DISPATCH_F(curve, t_fe_roundtrip, a, out) }
int ht_fe_inv(int curve, const uint8_t* a, uint8_t* out) { DISPATCH_F(curve, t_fe_inv, a, out) }
int ht_el_mul(int curve, const uint8_t* a, const uint8_t* b, uint8_t* out) { DISPATCH_C(curve, t_el_mul, a, b, out) }
int ht_el_inv(int curve, const uint8_t* a, uint8_t* out) { DISPATCH_C(curve, t_el_inv, a, out) }
int ht_madd_chain(int curve, const uint8_t* pts, size_t stride, const uint8_t* neg, size_t n, uint8_t* out) { DISPATCH_C(curve, t_madd_chain, pts, stride, neg, n, out) }
int ht_add_chains(int curve, const uint8_t* pts, size_t stride, size_t na, size_t nb, uint8_t* out) { DISPATCH_C(curve, t_add_chains, pts, stride, na, nb, out) }
int ht_msm_naive(int curve, const uint8_t* pts, size_t stride, const uint8_t* scalars, size_t n, uint8_t* out) { DISPATCH_C(curve, t_msm_naive, pts, stride, scalars, n, out) }
int ht_normalize(int curve, const uint8_t* in, uint8_t* out) { DISPATCH_C(curve, t_normalize, in, out) }

// (Y - X, Y + X, 2dXY) -- the base record -- of the image of an arkworks Affine image, as three ABI Montgomery field images; 1 = no image.
int ht_te_map(const uint8_t* img, uint8_t* out) {
  Modulus<TF> md;
  TeAffine t;
  if (!te_map_host(t, img, md)) return 1;
  uint32_t w[36];
  fe_to_abi<TF>(w, t.ymx, md);
  fe_to_abi<TF>(w + 12, t.ypx, md);
  fe_to_abi<TF>(w + 24, t.td, md);
  memcpy(out, w, 144);
  return 0;
}
// sum of (+/-) points through te_madd, starting from the identity as the kernels do, mapped back: a Projective image.
// 1 = a point without image, 2 = an addition hit a vanishing denominator (Z = 0).
int ht_te_madd_chain(const uint8_t* pts, size_t stride, const uint8_t* neg, size_t n, uint8_t* out) {
  Modulus<TF> md;
  Modulus<TEF> tmd;
  Xyzz acc;
  te_set_identity<TEF>(acc);
  for (size_t i = 0; i < n; i++) {
    if (pts[i * stride + 96]) continue;
    TeAffine t28, t;
    if (!te_map_host(t28, pts + i * stride, md)) return 1;
    te_record_to<TEF>(t, t28, tmd);
    te_madd<TEF>(acc, t, neg[i] != 0, tmd);
    if (te_failed<TEF>(acc)) return 2;
  }
  return te_finish_host(out, acc, md);
}
// (chain over the first na points) + (chain over the rest) through the unified extended addition, then `dbl` doublings.
int ht_te_add_chains(const uint8_t* pts, size_t stride, size_t na, size_t nb, int dbl, uint8_t* out) {
  Modulus<TF> md;
  Modulus<TEF> tmd;
  Xyzz a, b;
  te_set_identity<TEF>(a);
  te_set_identity<TEF>(b);
  for (size_t i = 0; i < na + nb; i++) {
    if (pts[i * stride + 96]) continue;
    TeAffine t28, t;
    if (!te_map_host(t28, pts + i * stride, md)) return 1;
    te_record_to<TEF>(t, t28, tmd);
    te_madd<TEF>(i < na ? a : b, t, false, tmd);
  }
  te_add<TEF>(a, b, tmd);
  if (te_failed<TEF>(a)) return 2;
  for (int i = 0; i < dbl; i++) {
    te_dbl<TEF>(a, tmd);
    if (te_failed<TEF>(a)) return 2;
  }
  return te_finish_host(out, a, md);
}
// The 13 x 29 shape of BLS12-377 Fq on its own: out = a * b (ABI Montgomery images in and out), the product formed by
// fe_mul<Bls12_377_Fq29> between the two re-radixing steps (fe_28_to_29 / fe_29_to_28).
int ht_fe29_mul(const uint8_t* a, const uint8_t* b, uint8_t* out) {
  Modulus<TF> md;
  Modulus<Bls12_377_Fq29> md29;
  Fe x, y, x29, y29, z29, z;
  fe_from_abi<TF>(x, (const uint32_t*)a, md);
  fe_from_abi<TF>(y, (const uint32_t*)b, md);
  fe_reduce<TF>(x);
  fe_reduce<TF>(y);
  fe_28_to_29(x29, x, md29);
  fe_28_to_29(y29, y, md29);
  fe_mul<Bls12_377_Fq29>(z29, x29, y29, md29);
  fe_29_to_28(z, z29, md);
  uint32_t w[12];
  fe_to_abi<TF>(w, z, md);
  memcpy(out, w, 48);
  return 0;
}
// Worst-case limbs through the 13 x 29 Edwards law: every coordinate / record field is forced to the LARGEST limbs its class
// allows (class M: 2^29 - 1 everywhere and the top limb of 1.5p; records: canonical, i.e. the limbs of p - 1 raised to 2^29 - 1 below
// the top), `rounds` mixed additions and one full addition are run, and the MSM_CHECK column sums decide.  Values are meaningless.
int ht_te29_extreme(int rounds) {
  using F = Bls12_377_Fq29;
  Modulus<F> md;
  Fe big;
  for (int i = 0; i < F::N - 1; i++) big.v[i] = (1u << 29) - 1;
  big.v[F::N - 1] = F::P[F::N - 1] + (F::P[F::N - 1] >> 1) + 1;   // the top limb of 1.5p
  for (int i = F::N; i < NL; i++) big.v[i] = 0;
  Fe rec = big;
  rec.v[F::N - 1] = F::P[F::N - 1];
  Xyzz acc{big, big, big, big}, other{big, big, big, big};
  TeAffine b{rec, rec, rec};
  for (int r = 0; r < rounds; r++) {
    Xyzz t = acc;
    te_madd<F>(t, b, (r & 1) != 0, md);
    t = acc;
    te_madd<F, true>(t, b, (r & 1) != 0, md);
  }
  te_add<F>(acc, other, md);
  return 0;
}
}

// ---- the 64-bit host tail (host_fold64.hpp) against the generic arithmetic ------------------------------------------------
#include <type_traits>

#include "host_fold64.hpp"

template <class F>
static const Fp64& test_fp64() {
  static Fp64 f = [] {
    Fp64 g{};
    g.init<F>();
    if (F::P[0] == 1) {   // BLS12-377: the twisted-Edwards constants
      g.const_from_device<F>(g.two_d, Bls12_377_Te::K2D);
      g.const_from_device<F>(g.sqrt3, Bls12_377_Te::SQRT3);
      g.const_from_device<F>(g.fsc_sqrt3, Bls12_377_Te::FSC_SQRT3);
    }
    return g;
  }();
  return f;
}

// field: out = a * b (ABI Montgomery images in and out), through Fp64::mul / add / sub / invert; op selects
template <class F>
static int t_f64_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  const Fp64& f = test_fp64<F>();
  F64 x, y, z;
  memcpy(x.l, a, 48);
  memcpy(y.l, b, 48);
  switch (op) {
    case 0: f.mul(z, x, y); break;
    case 1: f.add(z, x, y); break;
    case 2: f.sub(z, x, y); break;
    case 3: f.invert(z, x); break;
    case 4: f.mul_portable(z, x, y); break;   // the C loop that runs where mulx / adcx / adox are missing
    default: return 1;
  }
  memcpy(out, z.l, 48);
  return 0;
}
extern "C" int ht_f64_op(int curve, int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  return curve == 1 ? t_f64_op<Bls12_381_Fq>(op, a, b, out) : t_f64_op<Bls12_377_Fq>(op, a, b, out);
}

// Window sums S_w = k_w * P_w (affine images + 64-bit multipliers) folded with window size c, both ways; the two Projective
// images go to out_generic / out_fold64.  te = 1 (BLS12-377 only): the sums live on the twisted-Edwards image.
// Returns 0, or 2 when an Edwards addition hit a vanishing denominator (both implementations must agree on that too).
template <class E>
struct Fold64Of;   // the 64-bit field object that mirrors a device coordinate field
template <class F>
struct Fold64Of<FpEl<F>> {
  static const Fp64& get() { return test_fp64<F>(); }
};
template <class F, int NB>
struct Fold64Of<Fp2El<F, NB>> {
  static const Fp2_64<NB>& get() {
    static const Fp2_64<NB> f{&test_fp64<F>()};
    return f;
  }
};

template <class C>
static int t_fold_both(const uint8_t* pts, size_t stride, const uint64_t* mult, int windows, int c, int te, uint8_t* out_generic,
                       uint8_t* out_fold64) {
  using E = typename C::E;
  using F = typename E::Fld;
  using El = typename E::T;
  typename E::Md md;
  const auto& f = Fold64Of<E>::get();
  using FC = std::decay_t<decltype(f)>;
  constexpr size_t PB = 3 * 4 * E::WORDS;   // bytes of a Projective image
  XyzzT<El> sums[64];
  if (windows > 64) return 1;
  for (int w = 0; w < windows; w++) {
    AffineT<El> a;
    const bool inf = affine_from_abi<E>(a, pts + (size_t)w * stride, md);
    if (te) {
      if constexpr (std::is_same<E, FpEl<Bls12_377_Fq>>::value) {
        te_set_identity<F>(sums[w]);
        if (!inf) {
          TeAffine t;
          if (!te_map_host(t, pts + (size_t)w * stride, md)) return 1;
          for (int bit = 63; bit >= 0; bit--) {
            te_dbl<F>(sums[w], md);
            if ((mult[w] >> bit) & 1) te_madd<F>(sums[w], t, false, md);
          }
        }
      } else {
        return 1;
      }
    } else {
      xyzz_set_inf<E>(sums[w]);
      if (!inf) {
        const uint64_t k[4] = {mult[w], 0, 0, 0};
        xyzz_mul_u64x4<E>(sums[w], a, k, md);
      }
    }
  }
  XyzzT<El> g;
  XyzzG64<typename FC::El> h;
  bool ok_g = true, ok_h = true;
  if (te) {
    if constexpr (std::is_same<E, FpEl<Bls12_377_Fq>>::value) {
      ok_g = fold_windows_te<F>(g, sums, windows, c, md);
      ok_h = fold_windows_te64<F>(f, h, sums, windows, c);
    }
  } else {
    fold_windows<E>(g, sums, windows, c, md);
    fold_windows64<F>(f, h, sums, windows, c);
  }
  if (ok_g != ok_h) return 3;
  if (!ok_g) return 2;
  xyzz_to_projective_abi<E>(out_generic, g, md);
  sw64_to_abi(f, out_fold64, h);
  // the chunk sum as well: h + h against the generic doubling
  XyzzG64<typename FC::El> hh = h;
  sw64_add(f, hh, h);
  XyzzT<El> gg = g;
  xyzz_add<E>(gg, g, md);
  uint8_t b1[PB], b2[PB];
  xyzz_to_projective_abi<E>(b1, gg, md);
  sw64_to_abi(f, b2, hh);
  return memcmp(b1, b2, PB) == 0 ? 0 : 4;
}
extern "C" int ht_fold_both(int curve, const uint8_t* pts, size_t stride, const uint64_t* mult, int windows, int c, int te,
                            uint8_t* out_generic, uint8_t* out_fold64) {
  if (curve == 1) return te ? 1 : t_fold_both<Bls12_381_G1>(pts, stride, mult, windows, c, 0, out_generic, out_fold64);
  if (curve == 2) return te ? 1 : t_fold_both<Bls12_377_G2>(pts, stride, mult, windows, c, 0, out_generic, out_fold64);
  if (curve == 3) return te ? 1 : t_fold_both<Bls12_381_G2>(pts, stride, mult, windows, c, 0, out_generic, out_fold64);
  return t_fold_both<Bls12_377_G1>(pts, stride, mult, windows, c, te, out_generic, out_fold64);
}

// The fold of a wide anchored window (host_fold64.hpp fold_windows64 / fold_windows_te64 with `wide_a`): `windows + 1` window sums given
// as affine images -- rows 0 .. windows - 1 the bucket sets, row `windows` the plain sum R of bucket set wide_a + 1 -- folded on the
// short-Weierstrass image into out_sw and, te != 0 (BLS12-377 G1 only), on the twisted-Edwards image into out_te.  ok[0], ok[1]: what the
// two folds returned (the short-Weierstrass one cannot fail: 1; -1: not run).  wide_a = -1 is the plain fold of rows 0 .. windows - 1.
template <class C>
static int t_fold_wide(const uint8_t* pts, size_t stride, int windows, int c, int wide_a, int te, uint8_t* out_sw, uint8_t* out_te, int* ok) {
  using E = typename C::E;
  using F = typename E::Fld;
  using El = typename E::T;
  typename E::Md md;
  const auto& f = Fold64Of<E>::get();
  using FC = std::decay_t<decltype(f)>;
  if (windows < 1 || windows + 1 > 64 || c < 2 || wide_a < -1 || (wide_a >= 0 && wide_a + 2 != windows)) return 1;
  XyzzT<El> sums[64];
  ok[0] = ok[1] = -1;
  for (int w = 0; w <= windows; w++) {
    AffineT<El> a;
    xyzz_set_inf<E>(sums[w]);
    if (!affine_from_abi<E>(a, pts + (size_t)w * stride, md)) {
      const uint64_t k[4] = {1, 0, 0, 0};
      xyzz_mul_u64x4<E>(sums[w], a, k, md);
    }
  }
  XyzzG64<typename FC::El> h;
  fold_windows64<F>(f, h, sums, windows, c, wide_a);
  ok[0] = 1;
  sw64_to_abi(f, out_sw, h);
  if (te) {
    if constexpr (std::is_same<E, FpEl<Bls12_377_Fq>>::value) {
      for (int w = 0; w <= windows; w++) {
        AffineT<El> a;
        te_set_identity<F>(sums[w]);
        if (!affine_from_abi<E>(a, pts + (size_t)w * stride, md)) {
          TeAffine t;
          if (!te_map_host(t, pts + (size_t)w * stride, md)) return 1;
          te_madd<F>(sums[w], t, false, md);
        }
      }
      ok[1] = fold_windows_te64<F>(f, h, sums, windows, c, wide_a) ? 1 : 0;
      if (ok[1]) sw64_to_abi(f, out_te, h);
    } else {
      return 1;
    }
  }
  return 0;
}
extern "C" int ht_fold_wide(int curve, const uint8_t* pts, size_t stride, int windows, int c, int wide_a, int te, uint8_t* out_sw, uint8_t* out_te,
                            int* ok) {
  if (!pts || !out_sw || !ok || (te && !out_te)) return 1;
  if (curve == 0) return t_fold_wide<Bls12_377_G1>(pts, stride, windows, c, wide_a, te, out_sw, out_te, ok);
  if (curve == 2) return te ? 1 : t_fold_wide<Bls12_377_G2>(pts, stride, windows, c, wide_a, 0, out_sw, out_te, ok);
  return 1;
}

// ---- the op table of devtest_ops.hpp on the host: the twin of libmsm_devtest.so's msm_devtest_run ------------------------
// Same raw limb records in, same limbs out (the device build replaces the portable multiply loops, the Montgomery step and
// the selects with GCN assembly); MSM_CHECK is armed here, so a record that would overflow a 64-bit column or underflow a
// biased subtraction is caught on this side.
#include "devtest_ops.hpp"

template <class C, bool TE>
static int t_devop(int op, const uint32_t* in, int iw, uint32_t* out, int ow, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t* a = in + i * iw;
    uint32_t* r = out + i * ow;
    switch (op) {
#define DT_CASE(OP) case OP: devtest_apply<C, OP>(a, r); break;
      DT_CASE(DT_FE_MUL)
      DT_CASE(DT_FE_SQR)
      DT_CASE(DT_FE_MUL2)
      DT_CASE(DT_NOT_AND_LMASK)
      DT_CASE(DT_FE_WEAK_REDUCE)
      DT_CASE(DT_FR_FROM_MONT)
      DT_CASE(DT_FR_TO_MONT)
      DT_CASE(DT_SQRT)
      DT_CASE(DT_SQRT2)
      DT_CASE(DT_LEX_LARGEST)
      DT_CASE(DT_EL_MUL)
      DT_CASE(DT_EL_SQR)
      DT_CASE(DT_EL_MUL_C)
      DT_CASE(DT_EL_MUL_C_BIG)
      DT_CASE(DT_EL_SQR_C)
      DT_CASE(DT_EL_MUL_SUB_C)
      DT_CASE(DT_MADD_COMMON)
      DT_CASE(DT_MADD)
      DT_CASE(DT_ADD)
      DT_CASE(DT_DBL)
      default:
        if constexpr (TE) {
          switch (op) {
            DT_CASE(DT_TE_MADD)
            DT_CASE(DT_TE_MADD_SWAPPED)
            DT_CASE(DT_TE_ADD)
            DT_CASE(DT_TE_DBL)
            default: return -1;
          }
        } else {
          return -1;
        }
#undef DT_CASE
    }
  }
  return 0;
}

// the op subset of the 13 x 29 shape (devtest_ops.hpp: DT_CURVE_TE29)
static int t_devop_te29(int op, const uint32_t* in, int iw, uint32_t* out, int ow, size_t n) {
  using C = Bls12_377_G1_29;
  for (size_t i = 0; i < n; i++) {
    const uint32_t* a = in + i * iw;
    uint32_t* r = out + i * ow;
    switch (op) {
#define DT_CASE(OP) case OP: devtest_apply<C, OP>(a, r); break;
      DT_CASE(DT_FE_MUL)
      DT_CASE(DT_TE_MADD)
      DT_CASE(DT_TE_MADD_SWAPPED)
      DT_CASE(DT_TE_ADD)
      DT_CASE(DT_TE_DBL)
#undef DT_CASE
      default: return -1;
    }
  }
  return 0;
}

extern "C" int ht_devop(int curve, int op, const uint32_t* in, uint32_t* out, size_t n) {
  int iw = 0, ow = 0;
  if (curve < 0 || curve > DT_CURVE_TE29 || !in || !out) return -1;
  if (curve == DT_CURVE_TE29) {
    if (!dt_op_in_te29(op)) return -1;
    devtest_shape(op, NL, iw, ow);
    return iw ? t_devop_te29(op, in, iw, out, ow, n) : -1;
  }
  devtest_shape(op, curve >= 2 ? 2 * NL : NL, iw, ow);
  if (!iw) return -1;
  switch (curve) {
    case 0: return t_devop<Bls12_377_G1, true>(op, in, iw, out, ow, n);
    case 1: return t_devop<Bls12_381_G1, false>(op, in, iw, out, ow, n);
    case 2: return t_devop<Bls12_377_G2, false>(op, in, iw, out, ow, n);
    default: return t_devop<Bls12_381_G2, false>(op, in, iw, out, ow, n);
  }
}

extern "C" int ht_devop_shape(int curve, int op, int* in_words, int* out_words) {
  if (!in_words || !out_words || curve < 0 || curve > DT_CURVE_TE29) return -1;
  if (curve == DT_CURVE_TE29) {
    *in_words = *out_words = 0;
    if (dt_op_in_te29(op)) devtest_shape(op, NL, *in_words, *out_words);
    return (*in_words) ? 0 : -1;
  }
  devtest_shape(op, curve >= 2 ? 2 * NL : NL, *in_words, *out_words);
  if (curve != 0 && ((op >= DT_TE_MADD && op <= DT_TE_DBL) || op == DT_TE_ADD_QUAD)) *in_words = *out_words = 0;
  return (*in_words) ? 0 : -1;
}

// ---- per-point classification (check_points.hpp) with the limb-bound checker armed ---------------------------------------------
// `in`: n records, `stride` bytes apart (serialized != 0: uncompressed CanonicalSerialize records, stride = 2 coordinates);
// method: 0 exact, 1 endomorphism.  One status byte per record.  The device twin is k_check_points (kernels_check.hip).
#include "check_points.hpp"

template <class C>
static int t_check_points(int serialized, int method, const uint8_t* in, size_t stride, size_t n, uint8_t* status) {
  using E = typename C::E;
  typename E::Md md;
  constexpr size_t CB = E::WORDS * 4;
  if (stride < (serialized ? 2 * CB : 2 * CB + 1)) return -1;
  for (size_t i = 0; i < n; i++) {
    uint32_t w[2 * E::WORDS];
    memcpy(w, in + i * stride, 2 * CB);
    const uint8_t flag = serialized ? 0 : in[i * stride + 2 * CB];
    if (serialized)
      status[i] = method ? check_point<E, true, CHECK_ENDO>(w, flag, md) : check_point<E, true, CHECK_EXACT>(w, flag, md);
    else
      status[i] = method ? check_point<E, false, CHECK_ENDO>(w, flag, md) : check_point<E, false, CHECK_EXACT>(w, flag, md);
  }
  return 0;
}

extern "C" int ht_check_points(int curve, int serialized, int method, const uint8_t* in, size_t stride, size_t n, uint8_t* status) {
  if (curve < 0 || curve > 3 || (n && (!in || !status)) || method < 0 || method > 1) return -1;
  switch (curve) {
    case 0: return t_check_points<Bls12_377_G1>(serialized, method, in, stride, n, status);
    case 1: return t_check_points<Bls12_381_G1>(serialized, method, in, stride, n, status);
    case 2: return t_check_points<Bls12_377_G2>(serialized, method, in, stride, n, status);
    default: return t_check_points<Bls12_381_G2>(serialized, method, in, stride, n, status);
  }
}

// ---- batch fixed-base multiplication (fixed_base.hpp) with the limb-bound checker armed ----------------------------------------
// The SAME MSM_HD functions the kernels of kernels_fixed.hip wrap: level bases, table runs, windowed_mul, output normalisation.
// The device twin of fb_host_table's normalisation step is k_pre_normalize (msm_kernels.hpp), whose record contract it restates:
// canonical coordinates, all-zero for the point at infinity.
#include <vector>

#include "fixed_base.hpp"

template <class E>
static void fb_host_records(AffineDevT<typename E::T>* out, const XyzzT<typename E::T>* in, size_t n, const typename E::Md& md) {
  using El = typename E::T;
  std::vector<El> prefix(n);
  El run, inv;
  E::set_one(run);
  for (size_t j = 0; j < n; j++) {
    prefix[j] = run;
    if (!xyzz_is_inf<E>(in[j])) {
      El z;
      E::mul(z, in[j].zz, in[j].zzz, md);
      E::mul(run, run, z, md);
    }
  }
  el_inv(inv, run, md, (E*)nullptr);
  for (size_t j = n; j-- > 0;) {
    if (xyzz_is_inf<E>(in[j])) {
      E::zero(out[j].p.x);
      E::zero(out[j].p.y);
      continue;
    }
    El z, ti, zzi, zzzi;
    E::mul(ti, inv, prefix[j], md);
    E::mul(z, in[j].zz, in[j].zzz, md);
    E::mul(inv, inv, z, md);
    E::mul(zzi, ti, in[j].zzz, md);
    E::mul(zzzi, ti, in[j].zz, md);
    E::mul(out[j].p.x, in[j].x, zzi, md);
    E::mul(out[j].p.y, in[j].y, zzzi, md);
    E::reduce(out[j].p.x);
    E::reduce(out[j].p.y);
  }
}

// levels [j0, j1) of the table of g for window size w, as XYZZ (2^w entries per level), built the way the device builds them
template <class E>
static void fb_host_levels(std::vector<XyzzT<typename E::T>>& xyzz, const uint8_t* g_img, uint32_t w, uint32_t j0, uint32_t j1, const typename E::Md& md) {
  using El = typename E::T;
  const uint32_t levels = fb_levels(w), per = 1u << w;
  uint32_t rec[2 * E::WORDS];
  memcpy(rec, g_img, 8 * E::WORDS);
  std::vector<XyzzT<El>> lb(levels);
  fb_level_bases<E>(lb.data(), rec, g_img[8 * E::WORDS], w, levels, md);
  std::vector<AffineDevT<El>> lba(levels);
  fb_host_records<E>(lba.data(), lb.data(), levels, md);
  xyzz.resize((size_t)(j1 - j0) * per);
  for (uint32_t j = j0; j < j1; j++)
    for (uint32_t d0 = 0; d0 < per; d0 += FB_TABLE_RUN)
      fb_table_run<E>(xyzz.data() + (size_t)(j - j0) * per + d0, lba[j].p, xyzz_is_inf<E>(lb[j]), d0, d0 + FB_TABLE_RUN <= per ? FB_TABLE_RUN : per - d0, md);
}

// one table level as 2^w arkworks Affine images, `stride` bytes apart
template <class C>
static int t_fb_table_level(const uint8_t* g_img, int w, int level, uint8_t* out, size_t stride) {
  using E = typename C::E;
  using El = typename E::T;
  typename E::Md md;
  std::vector<XyzzT<El>> xyzz;
  fb_host_levels<E>(xyzz, g_img, (uint32_t)w, (uint32_t)level, (uint32_t)level + 1, md);
  const size_t n = xyzz.size();
  std::vector<XyzzDevT<El>> dev(n);
  for (size_t i = 0; i < n; i++) dev[i].p = xyzz[i];
  std::vector<El> prefix(n);
  fb_normalize_run<E, false>(dev.data(), 0, n, prefix.data(), out, stride, md);
  return 0;
}

// out[i] = scalar_i * g: the whole table, windowed_mul per scalar, normalisation in runs of FB_NORM_RUN.  flags as mi355_msm_fixed_mul.
template <class C>
static int t_fb_mul(const uint8_t* g_img, int w, const uint8_t* scalars, size_t n, unsigned flags, uint8_t* out, size_t stride) {
  using E = typename C::E;
  using El = typename E::T;
  typename E::Md md;
  const uint32_t levels = fb_levels((uint32_t)w);
  std::vector<XyzzT<El>> xyzz;
  fb_host_levels<E>(xyzz, g_img, (uint32_t)w, 0, levels, md);
  std::vector<AffineDevT<El>> table(xyzz.size());
  fb_host_records<E>(table.data(), xyzz.data(), xyzz.size(), md);
  std::vector<XyzzDevT<El>> res(n);
  for (size_t i = 0; i < n; i++) {
    uint32_t s[8];
    memcpy(s, scalars + 32 * i, 32);
    fb_windowed_mul<E>(res[i].p, table.data(), s, (flags & 1) != 0, (uint32_t)w, levels, md);
  }
  std::vector<El> prefix(n);
  for (size_t lo = 0; lo < n; lo += FB_NORM_RUN) {
    const size_t hi = lo + FB_NORM_RUN < n ? lo + FB_NORM_RUN : n;
    if (flags & 2)
      fb_normalize_run<E, true>(res.data(), lo, hi, prefix.data(), out, stride, md);
    else
      fb_normalize_run<E, false>(res.data(), lo, hi, prefix.data(), out, stride, md);
  }
  return 0;
}

extern "C" {
// the digits of one 32-byte scalar for window size w: fb_levels(w) words
int ht_fb_digits(const uint8_t* scalar, int w, uint32_t* out) {
  if (!scalar || !out || w < 1 || w > (int)FB_MAX_WINDOW) return -1;
  uint32_t s[8];
  memcpy(s, scalar, 32);
  const uint32_t levels = fb_levels((uint32_t)w);
  for (uint32_t j = 0; j < levels; j++) out[j] = fb_digit(s, j, (uint32_t)w);
  return (int)levels;
}
int ht_fb_table_level(int curve, const uint8_t* g_img, int w, int level, uint8_t* out, size_t stride) {
  if (!g_img || !out || w < 1 || w > (int)FB_MAX_WINDOW || level < 0 || level >= (int)fb_levels((uint32_t)w) || stride % 4) return -1;
  DISPATCH_C(curve, t_fb_table_level, g_img, w, level, out, stride)
}
int ht_fb_mul(int curve, const uint8_t* g_img, int w, const uint8_t* scalars, size_t n, unsigned flags, uint8_t* out, size_t stride) {
  if (!g_img || (n && (!scalars || !out)) || w < 1 || w > (int)FB_MAX_WINDOW || stride % 4 || (flags & ~3u)) return -1;
  DISPATCH_C(curve, t_fb_mul, g_img, w, scalars, n, flags, out, stride)
}
}

// ---- square roots, the y ordering and the compressed-record codec (sqrt.hpp, point_codec.hpp) with the limb-bound checker armed ----
// Elements cross as ABI images (x * 2^384 mod p, canonical; Fp2: c0 | c1), as in ht_el_mul.  The device twins are the sqrt / sqrt2 /
// lex_largest ops of libmsm_devtest.so and k_decompress_points / k_compress_points (kernels_codec.hip).
#include "point_codec.hpp"

template <class C>
static void t_el_sqrt(const uint8_t* a, uint8_t* out, int* has_root) {
  using E = typename C::E;
  typename E::Md md;
  typename E::T x, z;
  uint32_t wa[E::WORDS], wo[E::WORDS];
  memcpy(wa, a, 4 * E::WORDS);
  E::from_abi(x, wa, md);
  *has_root = el_sqrt(z, x, md, (E*)nullptr) ? 1 : 0;
  E::to_abi(wo, z, md);
  memcpy(out, wo, 4 * E::WORDS);
}

template <class C>
static void t_lex_largest(const uint8_t* a, int* larger) {
  using E = typename C::E;
  typename E::Md md;
  typename E::T x;
  uint32_t wa[E::WORDS];
  memcpy(wa, a, 4 * E::WORDS);
  E::from_abi(x, wa, md);
  *larger = el_lex_largest<E>(x, md) ? 1 : 0;
}

template <class C>
static int t_decompress_points(int serialized, const uint8_t* in, size_t n, uint8_t* out, size_t stride, uint8_t* status) {
  using E = typename C::E;
  typename E::Md md;
  constexpr size_t CB = E::WORDS * 4;
  if (serialized) stride = 2 * CB;
  if (stride < 2 * CB + (serialized ? 0 : 1) || (stride & 3)) return -1;
  for (size_t i = 0; i < n; i++) {
    uint32_t w[E::WORDS], o[2 * E::WORDS];
    uint8_t inf = 0;
    memcpy(w, in + i * CB, CB);
    status[i] = serialized ? decompress_point<E, true>(o, inf, w, md) : decompress_point<E, false>(o, inf, w, md);
    memset(out + i * stride, 0, stride);
    memcpy(out + i * stride, o, 2 * CB);
    if (!serialized) out[i * stride + 2 * CB] = inf;
  }
  return 0;
}

template <class C>
static int t_compress_points(int serialized, const uint8_t* in, size_t stride, size_t n, uint8_t* out, uint8_t* status) {
  using E = typename C::E;
  typename E::Md md;
  constexpr size_t CB = E::WORDS * 4;
  if (serialized) stride = 2 * CB;
  if (stride < 2 * CB + (serialized ? 0 : 1)) return -1;
  for (size_t i = 0; i < n; i++) {
    uint32_t w[2 * E::WORDS], o[E::WORDS];
    uint8_t inf = 0;
    memcpy(w, in + i * stride, 2 * CB);
    const uint8_t flag = serialized ? 0 : in[i * stride + 2 * CB];
    status[i] = serialized ? compress_point<E, true>(o, inf, w, flag, md) : compress_point<E, false>(o, inf, w, flag, md);
    memcpy(out + i * CB, o, CB);
  }
  return 0;
}

extern "C" {

// curve 0 / 1: Fp of BLS12-377 / BLS12-381 (48-byte images)
int ht_fe_sqrt(int curve, const uint8_t* a, uint8_t* out, int* has_root) {
  if (!a || !out || !has_root) return -1;
  switch (curve) {
    case 0: t_el_sqrt<Bls12_377_G1>(a, out, has_root); return 0;
    case 1: t_el_sqrt<Bls12_381_G1>(a, out, has_root); return 0;
    default: return -1;
  }
}
// curve 2 / 3: Fp2 of BLS12-377 / BLS12-381 (96-byte images)
int ht_fe2_sqrt(int curve, const uint8_t* a, uint8_t* out, int* has_root) {
  if (!a || !out || !has_root) return -1;
  switch (curve) {
    case 2: t_el_sqrt<Bls12_377_G2>(a, out, has_root); return 0;
    case 3: t_el_sqrt<Bls12_381_G2>(a, out, has_root); return 0;
    default: return -1;
  }
}
// the coordinate field of curve 0..3
int ht_lex_largest(int curve, const uint8_t* a, int* larger) {
  if (!a || !larger) return -1;
  DISPATCH_C(curve, t_lex_largest, a, larger)
}
int ht_decompress_points(int curve, int serialized, const uint8_t* in, size_t n, uint8_t* out, size_t stride, uint8_t* status) {
  if (curve < 0 || curve > 3 || (n && (!in || !out || !status))) return -1;
  switch (curve) {
    case 0: return t_decompress_points<Bls12_377_G1>(serialized, in, n, out, stride, status);
    case 1: return t_decompress_points<Bls12_381_G1>(serialized, in, n, out, stride, status);
    case 2: return t_decompress_points<Bls12_377_G2>(serialized, in, n, out, stride, status);
    default: return t_decompress_points<Bls12_381_G2>(serialized, in, n, out, stride, status);
  }
}
int ht_compress_points(int curve, int serialized, const uint8_t* in, size_t stride, size_t n, uint8_t* out, uint8_t* status) {
  if (curve < 0 || curve > 3 || (n && (!in || !out || !status))) return -1;
  switch (curve) {
    case 0: return t_compress_points<Bls12_377_G1>(serialized, in, stride, n, out, status);
    case 1: return t_compress_points<Bls12_381_G1>(serialized, in, stride, n, out, status);
    case 2: return t_compress_points<Bls12_377_G2>(serialized, in, stride, n, out, status);
    default: return t_compress_points<Bls12_381_G2>(serialized, in, stride, n, out, status);
  }
}

}  // extern "C"

// ---- batch variable-base multiplication (point_mul.hpp) with the limb-bound checker armed ---------------------------------------
// The SAME MSM_HD functions the kernels of kernels_pmul.hip wrap: signed digits, the per-point table, the windowed walk, the
// non-adjacent form and the one-scalar walk; records by fb_host_records (the restatement of k_pre_normalize above), output by
// fb_normalize_run.  The walk starts at the scalar's own top window (the device takes the maximum over a wave).
#include "point_mul.hpp"

template <class E, class Dev>
static void pm_host_output(const std::vector<Dev>& res, unsigned flags, uint8_t* out, size_t out_stride, const typename E::Md& md) {
  const size_t n = res.size();
  std::vector<typename E::T> prefix(n);
  for (size_t lo = 0; lo < n; lo += FB_NORM_RUN) {
    const size_t hi = lo + FB_NORM_RUN < n ? lo + FB_NORM_RUN : n;
    if (flags & 2)
      fb_normalize_run<E, true>(res.data(), lo, hi, prefix.data(), out, out_stride, md);
    else
      fb_normalize_run<E, false>(res.data(), lo, hi, prefix.data(), out, out_stride, md);
  }
}

// 1P .. 2^(w-1) P of one point as arkworks Affine images
template <class C>
static int t_pm_table(const uint8_t* img, int w, uint8_t* out, size_t stride) {
  using E = typename C::E;
  using El = typename E::T;
  typename E::Md md;
  const uint32_t entries = pm_table_entries((uint32_t)w);
  uint32_t rec[2 * E::WORDS];
  memcpy(rec, img, 8 * E::WORDS);
  std::vector<XyzzT<El>> x(entries);
  pm_table<E>(x.data(), 1, rec, img[8 * E::WORDS], entries, md);
  std::vector<XyzzDevT<El>> dev(entries);
  for (uint32_t e = 0; e < entries; e++) dev[e].p = x[e];
  pm_host_output<E>(dev, 0, out, stride, md);
  return 0;
}

template <class C>
static int t_pm_mul(const uint8_t* points, size_t stride, size_t n, const uint8_t* scalars, int w, unsigned flags, uint8_t* out, size_t out_stride) {
  using E = typename C::E;
  using El = typename E::T;
  typename E::Md md;
  const uint32_t entries = pm_table_entries((uint32_t)w);
  std::vector<XyzzDevT<El>> res(n);
  std::vector<XyzzT<El>> x(entries);
  std::vector<AffineDevT<El>> table(entries);
  for (size_t i = 0; i < n; i++) {
    const uint8_t* img = points + i * stride;
    uint32_t rec[2 * E::WORDS], s[8];
    memcpy(rec, img, 8 * E::WORDS);
    pm_table<E>(x.data(), 1, rec, img[8 * E::WORDS], entries, md);
    fb_host_records<E>(table.data(), x.data(), entries, md);
    memcpy(s, scalars + 32 * i, 32);
    if (flags & 1) fr_from_montgomery<typename CheckConsts<E>::FR>(s);
    pm_windowed_mul<E>(res[i].p, table.data(), 1, s, (uint32_t)w, pm_top_window(pm_bit_length(s), (uint32_t)w), md);
  }
  pm_host_output<E>(res, flags, out, out_stride, md);
  return 0;
}

template <class C>
static int t_pm_mul_uniform(const uint8_t* points, size_t stride, size_t n, const PmNaf* naf, unsigned flags, uint8_t* out, size_t out_stride) {
  using E = typename C::E;
  using El = typename E::T;
  typename E::Md md;
  std::vector<XyzzDevT<El>> res(n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t* img = points + i * stride;
    uint32_t rec[2 * E::WORDS];
    memcpy(rec, img, 8 * E::WORDS);
    pm_mul_uniform<E>(res[i].p, rec, img[8 * E::WORDS], *naf, md);
  }
  pm_host_output<E>(res, flags, out, out_stride, md);
  return 0;
}

#include "cofactor_consts.inc"

extern "C" {
// the signed digits of one 32-byte scalar for window size w: pm_digits(w) values
int ht_pm_digits(const uint8_t* scalar, int w, int32_t* out) {
  if (!scalar || !out || w < 1 || w > (int)PM_MAX_WINDOW) return -1;
  uint32_t s[8];
  memcpy(s, scalar, 32);
  const uint32_t nd = pm_digits((uint32_t)w);
  for (uint32_t j = 0; j < nd; j++) out[j] = pm_digit(s, j, (uint32_t)w);
  return (int)nd;
}
// the highest window the walk starts at for this scalar
int ht_pm_top_window(const uint8_t* scalar, int w) {
  if (!scalar || w < 1 || w > (int)PM_MAX_WINDOW) return -1;
  uint32_t s[8];
  memcpy(s, scalar, 32);
  return (int)pm_top_window(pm_bit_length(s), (uint32_t)w);
}
// the non-adjacent form of a little-endian integer of nbytes bytes (a multiple of 4, at most 64): 544 digits in {-1, 0, 1};
// returns the index of the top non-zero digit, -1 for zero, -2 for bad arguments
int ht_pm_naf(const uint8_t* k, size_t nbytes, int8_t* out) {
  if (!k || !out || nbytes % 4 || nbytes < 4 || nbytes > 64) return -2;
  uint32_t w[16] = {0};
  memcpy(w, k, nbytes);
  PmNaf naf;
  pm_naf_recode(naf, w, 16);
  for (uint32_t i = 0; i < 32 * PM_NAF_WORDS; i++) {
    const int nz = (naf.nz[i >> 5] >> (i & 31)) & 1, ng = (naf.neg[i >> 5] >> (i & 31)) & 1;
    out[i] = (int8_t)(nz ? (ng ? -1 : 1) : 0);
  }
  return naf.top;
}
// the cofactor of curve 0..3 as 64 little-endian bytes
int ht_pm_cofactor(int curve, uint8_t* out) {
  if (curve < 0 || curve > 3 || !out) return -1;
  memcpy(out, kCofactorWords[curve], 64);
  return (int)kCofactorBits[curve];
}
int ht_pm_table(int curve, const uint8_t* img, int w, uint8_t* out, size_t stride) {
  if (!img || !out || w < 1 || w > (int)PM_MAX_WINDOW || stride % 4) return -1;
  DISPATCH_C(curve, t_pm_table, img, w, out, stride)
}
// flags as mi355_msm_mul_points: bit 0 Fr Montgomery scalars, bit 1 Projective images
int ht_pm_mul(int curve, const uint8_t* points, size_t stride, size_t n, const uint8_t* scalars, int w, unsigned flags, uint8_t* out, size_t out_stride) {
  if ((n && (!points || !scalars || !out)) || w < 1 || w > (int)PM_MAX_WINDOW || out_stride % 4 || (flags & ~3u)) return -1;
  DISPATCH_C(curve, t_pm_mul, points, stride, n, scalars, w, flags, out, out_stride)
}
// one scalar for all points: k as in ht_pm_naf; flags bit 1 Projective images, bit 3 the curve's cofactor (k is then ignored)
int ht_pm_mul_uniform(int curve, const uint8_t* points, size_t stride, size_t n, const uint8_t* k, size_t nbytes, unsigned flags, uint8_t* out,
                      size_t out_stride) {
  if ((n && (!points || !out)) || out_stride % 4 || (flags & ~10u) || curve < 0 || curve > 3) return -1;
  uint32_t w[16] = {0};
  if (flags & 8) {
    memcpy(w, kCofactorWords[curve], 64);
  } else {
    if (!k || nbytes % 4 || nbytes < 4 || nbytes > 64) return -1;
    memcpy(w, k, nbytes);
  }
  PmNaf naf;
  pm_naf_recode(naf, w, 16);
  DISPATCH_C(curve, t_pm_mul_uniform, points, stride, n, &naf, flags, out, out_stride)
}
}

// ---- scalar fields and radix-2 domains (fr.hpp, ntt.hpp): the kernels' per-element functions, a block's loops run in order ------
#include <vector>
#include "ntt.hpp"

template <class FR>
static void t_fr_table(std::vector<Fr>& out, const Fr& base, uint32_t n) {
  out.resize(n);
  for (uint32_t i = 0; i < n; i++) ntt_table_entry<FR>(out[i], base, i);
}

template <class FR>
static void t_ntt_two_level(std::vector<Fr>& lo, std::vector<Fr>& hi, const Fr& base, uint32_t k) {
  const uint32_t h = ntt_lo_log(k);
  Fr hb;
  ntt_hi_base<FR>(hb, base, h);
  t_fr_table<FR>(lo, base, 1u << h);
  t_fr_table<FR>(hi, hb, 1u << (k - h));
}

template <class FR>
static int t_ntt_transform(uint32_t k, uint32_t pass_log, unsigned kind, unsigned flags, const uint8_t* offset, const uint8_t* in, uint32_t in_len,
                           uint32_t batch, uint8_t* out) {
  const size_t n = (size_t)1 << k;
  Fr root, small_root, g;
  ntt_root<FR>(root, k);
  ntt_root<FR>(small_root, NTT_SMALL_LOG);
  if (offset) {
    uint32_t w[8];
    memcpy(w, offset, 32);
    fr_from_abi<FR>(g, w, (flags & kNttCallNormal) != 0);
    fr_reduce<FR>(g);
  } else {
    fr_set<FR>(g, FR::GENERATOR);
  }
  if (kind & kNttKindInverse) {
    fr_inv<FR>(root, root);
    fr_inv<FR>(small_root, small_root);
    fr_inv<FR>(g, g);
  }
  std::vector<Fr> wlo, whi, glo, ghi, small;
  t_ntt_two_level<FR>(wlo, whi, root, k);
  t_ntt_two_level<FR>(glo, ghi, g, k);
  t_fr_table<FR>(small, small_root, 1u << (NTT_SMALL_LOG - 1));
  uint32_t radix[NTT_MAX_LOG];
  const uint32_t npass = ntt_plan(k, pass_log, radix);
  std::vector<uint32_t> bufa(n * 8), bufb(n * 8);
  std::vector<Fr> lds(NTT_TILE);
  for (uint32_t b = 0; b < batch; b++) {
    const uint32_t* src = (const uint32_t*)(in + b * n * 32);
    for (uint32_t i = 0; i < npass; i++) {
      NttPass ps;
      ntt_pass_shape(ps, k, radix, npass, i, kind, flags, in_len);
      ps.w = NttTable{wlo.data(), whi.data()};
      ps.g = NttTable{glo.data(), ghi.data()};
      ps.small = small.data();
      if (ps.has_scale) ntt_size_inv<FR>(ps.scale, k);
      uint32_t* dst = i + 1 == npass ? (uint32_t*)(out + b * n * 32) : (i & 1) ? bufb.data() : bufa.data();
      const uint32_t elems = 1u << (ps.p + ps.log_c), tiles = 1u << (k - ps.p - ps.log_c);
      for (uint32_t tile = 0; tile < tiles; tile++) {
        for (uint32_t e = 0; e < elems; e++) ntt_load<FR>(lds[e], ps, src, tile, e);
        for (uint32_t l = 0; l < ps.p; l++)
          for (uint32_t u = 0; u < elems / 2; u++) ntt_butterfly<FR>(lds.data(), ps, l, u);
        for (uint32_t e = 0; e < elems; e++) ntt_store<FR>(lds.data(), ps, dst, tile, e);
      }
      src = dst;
    }
  }
  return 0;
}

template <class FR>
static int t_fr_op(int op, const uint8_t* a, const uint8_t* b, int normal, uint8_t* out) {
  uint32_t wa[8], wb[8], wo[8];
  memcpy(wa, a, 32);
  memcpy(wb, b, 32);
  if (op == 0) {
    fr_mul_abi<FR>(wo, wa, wb, normal != 0);
  } else {
    Fr x, y, z;
    fr_from_abi<FR>(x, wa, normal != 0);
    fr_from_abi<FR>(y, wb, normal != 0);
    if (op == 1) fr_add(z, x, y); else fr_sub<FR>(z, x, y);
    fr_carry(z);
    fr_to_abi<FR>(wo, z, normal != 0);
  }
  memcpy(out, wo, 32);
  return 0;
}

template <class FR>
static int t_ntt_element(uint32_t k, uint64_t i, uint8_t* out) {
  Fr root, r;
  ntt_root<FR>(root, k);
  uint32_t e[8] = {(uint32_t)i, (uint32_t)(i >> 32), 0, 0, 0, 0, 0, 0}, w[8];
  fr_pow_words<FR>(r, root, e);
  fr_to_abi<FR>(w, r, false);
  memcpy(out, w, 32);
  return 0;
}

// the worst case the butterfly chain may reach: a level-10 chain on limbs at their bounds; only the checker matters
template <class FR>
static int t_fr_extreme() {
  Fr a, b, w, t, d;
  for (int i = 0; i < FR_NL - 1; i++) a.v[i] = b.v[i] = FR_MASK;
  a.v[FR_NL - 1] = b.v[FR_NL - 1] = 2 * FR::P[FR_NL - 1] + 1;   // just under 2r + 2^232: the top of class M
  for (int i = 0; i < FR_NL; i++) w.v[i] = FR::P[i];
  w.v[0] -= 1;                                                   // r - 1: the largest twiddle
  for (int l = 0; l < (int)NTT_MAX_PASS_LOG; l++) {
    fr_mul<FR>(t, b, w);
    for (int i = 0; i < FR_NL - 1; i++) t.v[i] = FR_MASK;        // the largest normalised limbs a product can leave
    fr_sub<FR>(d, a, t);
    fr_add(a, a, t);
    fr_carry(a);
    fr_carry(d);
    b = d;                                                       // the difference is the faster-growing side
    a = d;
  }
  fr_mul<FR>(t, b, w);
  return 0;
}

extern "C" {
// field: 0 BLS12-377 Fr, 1 BLS12-381 Fr.  op 0 product, 1 sum, 2 difference of two 32-byte elements (any 256-bit value), ABI form in and out
int ht_fr_op(int field, int op, const uint8_t* a, const uint8_t* b, int normal, uint8_t* out) {
  if (!a || !b || !out || op < 0 || op > 2) return -1;
  return field == 0 ? t_fr_op<Bls12_377_Fr29>(op, a, b, normal, out) : field == 1 ? t_fr_op<Bls12_381_Fr29>(op, a, b, normal, out) : -1;
}
int ht_fr_extreme(int field) { return field == 0 ? t_fr_extreme<Bls12_377_Fr29>() : field == 1 ? t_fr_extreme<Bls12_381_Fr29>() : -1; }
// one call of mi355_msm_domain_transform on the host: kind 0 forward, 1 inverse, 2 coset forward, 3 coset inverse; flags bit 0 normal
// form, bit 1 bit-reversed output (forward), bit 2 bit-reversed input (inverse); offset NULL: GENERATOR
int ht_ntt_transform(int field, unsigned k, unsigned pass_log, unsigned kind, unsigned flags, const uint8_t* offset, const uint8_t* in, unsigned in_len,
                     unsigned batch, uint8_t* out) {
  if (k > 20 || pass_log < 1 || pass_log > NTT_MAX_PASS_LOG || kind > 3 || (flags & ~7u) || !in || !out || in_len > (1u << k)) return -1;
  if (((flags & kNttCallNR) && (kind & kNttKindInverse)) || ((flags & kNttCallRN) && !(kind & kNttKindInverse))) return -1;
  return field == 0   ? t_ntt_transform<Bls12_377_Fr29>(k, pass_log, kind, flags, offset, in, in_len, batch, out)
         : field == 1 ? t_ntt_transform<Bls12_381_Fr29>(k, pass_log, kind, flags, offset, in, in_len, batch, out)
                      : -1;
}
// element(i) = omega^i of the domain of size 2^k, as an arkworks image
int ht_ntt_element(int field, unsigned k, uint64_t i, uint8_t* out) {
  if (!out) return -1;
  return field == 0 ? t_ntt_element<Bls12_377_Fr29>(k, i, out) : field == 1 ? t_ntt_element<Bls12_381_Fr29>(k, i, out) : -1;
}
}

// ---- the steps between a transform and an MSM (poly.hpp): the kernels' per-element functions, a block's loops run in order, and the
// chains of launches the engine runs ------------------------------------------------------------------------------------------------
#include "poly.hpp"

template <class FR>
struct HostPolyRun {
  std::vector<Fr> lds, sa, sb, na, nb;
  HostPolyRun() : lds(POLY_MAX_TILE), sa(POLY_MAX_LANES), sb(POLY_MAX_LANES), na(POLY_MAX_LANES), nb(POLY_MAX_LANES) {}
  void eval(const PolyEval& p) {
    const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log);
    for (uint64_t tile = 0; tile < poly_tiles(p.t.n, p.t.tile_log); tile++) {
      for (uint32_t i = 0; i < T; i++) poly_load<FR>(lds[i], p.t, (tile << p.t.tile_log) + i);
      for (uint32_t l = 0; l < lanes; l++) poly_eval_lane<FR>(lds.data(), p.z, l);
      for (uint32_t s = 0; (2u << s) <= lanes; s++)
        for (uint32_t j = 0; j < (lanes >> (s + 1)); j++) poly_eval_tree<FR>(lds.data(), p.z, s, j);
      poly_store_m<FR>(p.dst + tile, lds[0]);
    }
  }
  void div(const PolyDiv& p) {
    const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log);
    std::vector<PolyDivLane> st(lanes);
    for (uint64_t tile = 0; tile < poly_tiles(p.t.n, p.t.tile_log); tile++) {
      for (uint32_t i = 0; i < T; i++) poly_load<FR>(lds[i], p.t, (tile << p.t.tile_log) + i);
      for (uint32_t l = 0; l < lanes; l++) poly_div_lane<FR>(st[l], lds.data(), sa.data(), p, tile, l);
      for (uint32_t s = 0; (1u << s) < lanes; s++) {
        for (uint32_t l = 0; l < lanes; l++) poly_div_scan<FR>(na[l], sa.data(), p.z, lanes, s, l);
        for (uint32_t l = 0; l < lanes; l++) sa[l] = na[l];
      }
      for (uint32_t l = 0; l < lanes; l++) poly_div_finish<FR>(st[l], lds.data(), sa.data(), p.z, lanes, l);
      for (uint32_t i = 0; i < T; i++) poly_div_store<FR>(lds.data(), p, tile, i);
    }
  }
  void inv_prod(const PolyInv& p) {
    const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log);
    for (uint64_t tile = 0; tile < poly_tiles(p.t.n, p.t.tile_log); tile++) {
      bool zero;
      for (uint32_t i = 0; i < T; i++) poly_inv_load<FR>(lds[i], zero, p.t, (tile << p.t.tile_log) + i);
      for (uint32_t l = 0; l < lanes; l++) poly_prod_lane<FR>(lds.data(), l);
      for (uint32_t s = 0; (2u << s) <= lanes; s++)
        for (uint32_t j = 0; j < (lanes >> (s + 1)); j++) poly_prod_tree<FR>(lds.data(), s, j);
      p.tiles[tile] = lds[0];
    }
  }
  void inv_tiles(Fr* tiles, uint64_t count, const Fr& coeff) {
    for (uint64_t t = 0; t < count; t++) poly_inv_tile<FR>(tiles, coeff, t);
  }
  void inv_apply(const PolyInv& p) {
    const uint32_t T = 1u << p.t.tile_log, lanes = poly_lanes(p.t.tile_log);
    std::vector<PolyInvLane> st(lanes);
    std::vector<char> zeros(T);
    for (uint64_t tile = 0; tile < poly_tiles(p.t.n, p.t.tile_log); tile++) {
      for (uint32_t i = 0; i < T; i++) {
        bool zero;
        poly_inv_load<FR>(lds[i], zero, p.t, (tile << p.t.tile_log) + i);
        zeros[i] = zero;
      }
      for (uint32_t l = 0; l < lanes; l++) poly_inv_lane<FR>(st[l], lds.data(), sa.data(), sb.data(), l);
      for (uint32_t s = 0; (1u << s) < lanes; s++) {
        for (uint32_t l = 0; l < lanes; l++) poly_inv_scan<FR>(na[l], nb[l], sa.data(), sb.data(), lanes, s, l);
        for (uint32_t l = 0; l < lanes; l++) {
          sa[l] = na[l];
          sb[l] = nb[l];
        }
      }
      for (uint32_t l = 0; l < lanes; l++) poly_inv_finish<FR>(st[l], lds.data(), sa.data(), sb.data(), p.tiles[tile], lanes, l);
      for (uint32_t i = 0; i < T; i++) poly_inv_store<FR>(lds.data(), p, tile, i, zeros[i] != 0);
    }
  }
};

template <class FR>
static int t_poly_inverse(uint32_t tile_log, unsigned flags, const uint8_t* coeff, const uint8_t* in, uint64_t n, uint8_t* out) {
  if (n == 0) return 0;
  std::vector<Fr> work(poly_work_elems(n, tile_log));
  std::vector<uint32_t> src(n * 8);
  memcpy(src.data(), in, n * 32);
  Fr c;
  if (coeff) poly_scalar<FR>(c, coeff, (flags & kPolyNormal) != 0); else fr_set<FR>(c, FR::ONE);
  HostPolyRun<FR> run;
  poly_chain_inverse<FR>(run, src.data(), src.data(), n, (flags & kPolyNormal) != 0, tile_log, c, work.data());   // in place, as out == in
  memcpy(out, src.data(), n * 32);
  return 0;
}

template <class FR>
static int t_poly_evaluate(uint32_t tile_log, unsigned flags, const uint8_t* coeffs, uint64_t n, const uint8_t* z, uint8_t* out32) {
  memset(out32, 0, 32);
  if (n == 0) return 0;
  std::vector<Fr> work(poly_work_elems(n, tile_log));
  std::vector<uint32_t> src(n * 8);
  memcpy(src.data(), coeffs, n * 32);
  Fr zz;
  poly_scalar<FR>(zz, z, (flags & kPolyNormal) != 0);
  HostPolyRun<FR> run;
  const Fr* res = poly_chain_evaluate<FR>(run, src.data(), n, (flags & kPolyNormal) != 0, tile_log, zz, work.data());
  poly_scalar_out<FR>(out32, *res, (flags & kPolyNormal) != 0);
  return 0;
}

template <class FR>
static int t_poly_divide(uint32_t tile_log, unsigned flags, const uint8_t* coeffs, uint64_t n, const uint8_t* z, uint8_t* q, uint8_t* rem32) {
  memset(rem32, 0, 32);
  if (n == 0) return 0;
  std::vector<Fr> work(poly_work_elems(n, tile_log));
  std::vector<uint32_t> src(n * 8), dst(n * 8);
  memcpy(src.data(), coeffs, n * 32);
  Fr zz;
  poly_scalar<FR>(zz, z, (flags & kPolyNormal) != 0);
  HostPolyRun<FR> run;
  const Fr* res = poly_chain_divide<FR>(run, dst.data(), src.data(), n, (flags & kPolyNormal) != 0, tile_log, zz, work.data());
  poly_scalar_out<FR>(rem32, *res, (flags & kPolyNormal) != 0);
  if (n > 1) memcpy(q, dst.data(), (n - 1) * 32);
  return 0;
}

template <class FR>
static int t_poly_vec_op(unsigned flags, unsigned op, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint64_t n, uint8_t* out) {
  std::vector<uint32_t> va(n * 8 + 8), vb(n * 8 + 8), vc(n * 8 + 8), vo(n * 8 + 8);
  memcpy(va.data(), a, n * 32);
  if (op != kPolyScale) memcpy(vb.data(), b, n * 32);
  if (op == kPolyMulSub) memcpy(vc.data(), c, n * 32);
  PolyVecOp p{va.data(), vb.data(), vc.data(), vo.data(), n, op, (flags & kPolyNormal) ? 1u : 0u, Fr{}};
  if (op == kPolyScale) poly_scalar<FR>(p.s, b, (flags & kPolyNormal) != 0);
  for (uint64_t i = 0; i < n; i++) poly_vec_op<FR>(p, i);
  memcpy(out, vo.data(), n * 32);
  return 0;
}

// 1 / Z(g) for the offset g (NULL: GENERATOR); -1 when g is zero or lies in the domain
template <class FR>
static int t_poly_coset_factor(uint32_t k, unsigned flags, const uint8_t* offset, uint8_t* out32) {
  Fr g, zg, zero, s;
  fr_zero(zero);
  if (offset) poly_scalar<FR>(g, offset, (flags & kPolyNormal) != 0); else fr_set<FR>(g, FR::GENERATOR);
  if (memcmp(g.v, zero.v, sizeof g.v) == 0) return -1;
  poly_vanishing<FR>(zg, g, k);
  if (memcmp(zg.v, zero.v, sizeof zg.v) == 0) return -1;
  fr_inv<FR>(s, zg);
  poly_scalar_out<FR>(out32, s, (flags & kPolyNormal) != 0);
  return 0;
}

template <class FR>
static int t_poly_vanishing(uint32_t k, unsigned flags, const uint8_t* tau, uint8_t* out32) {
  Fr x, zt;
  poly_scalar<FR>(x, tau, (flags & kPolyNormal) != 0);
  poly_vanishing<FR>(zt, x, k);
  poly_scalar_out<FR>(out32, zt, (flags & kPolyNormal) != 0);
  return 0;
}

template <class FR>
static int t_poly_lagrange(uint32_t k, uint32_t tile_log, unsigned flags, const uint8_t* tau, uint8_t* out) {
  const uint64_t n = (uint64_t)1 << k;
  const bool normal = (flags & kPolyNormal) != 0;
  Fr root, iroot, zt, zero, size_inv;
  fr_zero(zero);
  ntt_root<FR>(root, k);
  fr_inv<FR>(iroot, root);
  ntt_size_inv<FR>(size_inv, k);
  std::vector<Fr> wlo, whi, ilo, ihi;
  t_ntt_two_level<FR>(wlo, whi, root, k);
  t_ntt_two_level<FR>(ilo, ihi, iroot, k);
  std::vector<uint32_t> dst(n * 8);
  PolyLagrange p{};
  p.dst = dst.data();
  p.k = k;
  p.normal = normal ? 1u : 0u;
  p.w = NttTable{wlo.data(), whi.data()};
  p.wi = NttTable{ilo.data(), ihi.data()};
  poly_scalar<FR>(p.tau, tau, normal);
  poly_vanishing<FR>(zt, p.tau, k);
  p.in_domain = memcmp(zt.v, zero.v, sizeof zt.v) == 0;
  p.c = zero;
  if (!p.in_domain) {
    fr_mul<FR>(zt, zt, size_inv);
    fr_reduce<FR>(zt);
    fr_inv<FR>(p.c, zt);
  }
  for (uint32_t i = 0; i < n; i++) poly_lagrange_entry<FR>(p, i);
  if (!p.in_domain) {
    std::vector<Fr> work(poly_work_elems(n, tile_log));
    Fr one;
    fr_set<FR>(one, FR::ONE);
    HostPolyRun<FR> run;
    poly_chain_inverse<FR>(run, dst.data(), dst.data(), n, normal, tile_log, one, work.data());
  }
  memcpy(out, dst.data(), n * 32);
  return 0;
}

#define POLY_FIELD(fn, ...) (field == 0 ? fn<Bls12_377_Fr29>(__VA_ARGS__) : field == 1 ? fn<Bls12_381_Fr29>(__VA_ARGS__) : -1)
static bool poly_args_ok(unsigned tile_log, unsigned flags, uint64_t n) {
  return tile_log >= POLY_TILE_LOG_MIN && tile_log <= POLY_TILE_LOG_MAX && !(flags & ~kPolyNormal) && n <= ((uint64_t)1 << 24);
}

extern "C" {
// the calls of msm_poly.hpp on the host, a block's loops in order.  field: 0 BLS12-377 Fr, 1 BLS12-381 Fr; flags bit 0: normal form;
// tile_log 4 .. 10; scalars are one 32-byte element in the form of the call
int ht_poly_batch_inverse(int field, unsigned tile_log, unsigned flags, const uint8_t* coeff, const uint8_t* in, uint64_t n, uint8_t* out) {
  if (!poly_args_ok(tile_log, flags, n) || (n && (!in || !out))) return -1;
  return POLY_FIELD(t_poly_inverse, tile_log, flags, coeff, in, n, out);
}
int ht_poly_evaluate(int field, unsigned tile_log, unsigned flags, const uint8_t* coeffs, uint64_t n, const uint8_t* z, uint8_t* out32) {
  if (!poly_args_ok(tile_log, flags, n) || (n && !coeffs) || !z || !out32) return -1;
  return POLY_FIELD(t_poly_evaluate, tile_log, flags, coeffs, n, z, out32);
}
int ht_poly_divide_by_linear(int field, unsigned tile_log, unsigned flags, const uint8_t* coeffs, uint64_t n, const uint8_t* z, uint8_t* q, uint8_t* rem32) {
  if (!poly_args_ok(tile_log, flags, n) || (n && !coeffs) || (n > 1 && !q) || !z || !rem32) return -1;
  return POLY_FIELD(t_poly_divide, tile_log, flags, coeffs, n, z, q, rem32);
}
// op 0 a + b, 1 a - b, 2 a*b - c, 3 b[0] * a (b: one element)
int ht_poly_vec_op(int field, unsigned flags, unsigned op, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint64_t n, uint8_t* out) {
  if (!poly_args_ok(POLY_DEFAULT_TILE_LOG, flags, n) || op > kPolyScale || !a || !b || (op == kPolyMulSub && !c) || !out) return -1;
  return POLY_FIELD(t_poly_vec_op, flags, op, a, b, c, n, out);
}
int ht_poly_lagrange(int field, unsigned k, unsigned tile_log, unsigned flags, const uint8_t* tau, uint8_t* out) {
  if (!poly_args_ok(tile_log, flags, 0) || k > 16 || !tau || !out) return -1;
  return POLY_FIELD(t_poly_lagrange, k, tile_log, flags, tau, out);
}
int ht_poly_vanishing(int field, unsigned k, unsigned flags, const uint8_t* tau, uint8_t* out32) {
  if ((flags & ~kPolyNormal) || k > 28 || !tau || !out32) return -1;
  return POLY_FIELD(t_poly_vanishing, k, flags, tau, out32);
}
// the factor of divide_by_vanishing_on_coset, 1 / (g^(2^k) - 1); -1 for an offset that is zero or lies in the domain
int ht_poly_coset_factor(int field, unsigned k, unsigned flags, const uint8_t* offset, uint8_t* out32) {
  if ((flags & ~kPolyNormal) || k > 28 || !out32) return -1;
  return POLY_FIELD(t_poly_coset_factor, k, flags, offset, out32);
}
}

// ---- prefix scans and the permutation product (scan.hpp): a block's loops run in order, and the chains of launches the engine runs --
#include "scan.hpp"

template <class FR>
struct HostScanRun {
  std::vector<Fr> lds, sc, nv;
  HostScanRun() : lds(POLY_MAX_TILE), sc(POLY_MAX_LANES), nv(POLY_MAX_LANES) {}
  template <unsigned OP>
  void up(const ScanUp& p) {
    const uint32_t T = 1u << p.s.t.tile_log, lanes = poly_lanes(p.s.t.tile_log);
    for (uint64_t tile = 0; tile < poly_tiles(p.s.t.n, p.s.t.tile_log); tile++) {
      for (uint32_t i = 0; i < T; i++) scan_load<FR, OP>(lds[i], p.s, (tile << p.s.t.tile_log) + i);
      for (uint32_t l = 0; l < lanes; l++) scan_up_lane<FR, OP>(lds.data(), l);
      for (uint32_t s = 0; (2u << s) <= lanes; s++)
        for (uint32_t j = 0; j < (lanes >> (s + 1)); j++) scan_up_tree<FR, OP>(lds.data(), s, j);
      scan_store_m<FR, OP>(p.dst + tile, lds[0]);
    }
  }
  template <unsigned OP>
  void down(const ScanDown& p) {
    const uint32_t T = 1u << p.s.t.tile_log, lanes = poly_lanes(p.s.t.tile_log);
    std::vector<ScanLane> st(lanes);
    for (uint64_t tile = 0; tile < poly_tiles(p.s.t.n, p.s.t.tile_log); tile++) {
      for (uint32_t i = 0; i < T; i++) scan_load<FR, OP>(lds[i], p.s, (tile << p.s.t.tile_log) + i);
      for (uint32_t l = 0; l < lanes; l++) scan_down_lane<FR, OP>(st[l], lds.data(), sc.data(), l);
      for (uint32_t s = 0; (1u << s) < lanes; s++) {
        for (uint32_t l = 0; l < lanes; l++) scan_down_step<FR, OP>(nv[l], sc.data(), s, l);
        for (uint32_t l = 0; l < lanes; l++) sc[l] = nv[l];
      }
      for (uint32_t l = 0; l < lanes; l++) scan_down_finish<FR, OP>(st[l], lds.data(), sc.data(), p, tile, lanes, l);
      for (uint32_t i = 0; i < T; i++) scan_down_store<FR, OP>(lds.data(), p, tile, i);
    }
  }
};

// in_place: the chain runs with dst == src, as a call with out == in does
template <class FR>
static int t_scan(uint32_t tile_log, unsigned flags, unsigned op, int in_place, const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* total32) {
  const bool normal = (flags & kScanNormal) != 0, inclusive = (flags & kScanInclusive) != 0;
  Fr id;
  if (op == kScanProduct) fr_set<FR>(id, FR::ONE); else fr_zero(id);
  if (n == 0) {
    if (total32) poly_scalar_out<FR>(total32, id, normal);
    return 0;
  }
  std::vector<Fr> work(scan_work_elems(n, tile_log));
  std::vector<uint32_t> src(n * 8), other(in_place ? 0 : n * 8);
  memcpy(src.data(), in, n * 32);
  uint32_t* dst = in_place ? src.data() : other.data();
  HostScanRun<FR> run;
  const Fr* res = op == kScanProduct ? scan_chain<FR, kScanProduct>(run, dst, src.data(), nullptr, n, normal, inclusive, tile_log, work.data())
                                     : scan_chain<FR, kScanSum>(run, dst, src.data(), nullptr, n, normal, inclusive, tile_log, work.data());
  if (total32) poly_scalar_out<FR>(total32, *res, normal);
  memcpy(out, dst, n * 32);
  return 0;
}

template <class FR>
static int t_scan_permutation(uint32_t k, uint32_t tile_log, unsigned flags, uint32_t m, uint64_t stride, const uint8_t* wires, const uint8_t* sigmas,
                              const uint8_t* ks, const uint8_t* beta, const uint8_t* gamma, uint8_t* out, uint8_t* total32) {
  const uint64_t n = (uint64_t)1 << k, span = (m - 1) * stride + n;
  const bool normal = (flags & kScanNormal) != 0;
  Fr root;
  ntt_root<FR>(root, k);
  std::vector<Fr> wlo, whi;
  t_ntt_two_level<FR>(wlo, whi, root, k);
  std::vector<uint32_t> w(span * 8), sg(span * 8), num(n * 8), den(n * 8), dst(n * 8);
  memcpy(w.data(), wires, span * 32);
  memcpy(sg.data(), sigmas, span * 32);
  ScanPerm p{};
  p.wires = w.data();
  p.sigmas = sg.data();
  p.num = num.data();
  p.den = den.data();
  p.stride = stride;
  p.k = k;
  p.m = m;
  p.normal = normal ? 1u : 0u;
  p.w = NttTable{wlo.data(), whi.data()};
  poly_scalar<FR>(p.beta, beta, normal);
  poly_scalar<FR>(p.gamma, gamma, normal);
  for (uint32_t i = 0; i < m; i++) poly_scalar<FR>(p.ks[i], ks + 32 * i, normal);
  for (uint32_t j = 0; j < n; j++) scan_perm_row<FR>(p, j);
  std::vector<Fr> iwork(poly_work_elems(n, tile_log)), work(scan_work_elems(n, tile_log));
  Fr one;
  fr_set<FR>(one, FR::ONE);
  HostPolyRun<FR> inv;
  poly_chain_inverse<FR>(inv, den.data(), den.data(), n, normal, tile_log, one, iwork.data());
  HostScanRun<FR> run;
  const Fr* res = scan_chain<FR, kScanProduct>(run, dst.data(), num.data(), den.data(), n, normal, false, tile_log, work.data());
  if (total32) poly_scalar_out<FR>(total32, *res, normal);
  memcpy(out, dst.data(), n * 32);
  return 0;
}

extern "C" {
// mi355_msm_domain_scan on the host: op 0 product, 1 sum; flags bit 0 normal form, bit 1 inclusive; total32 may be NULL
int ht_scan_scan(int field, unsigned tile_log, unsigned flags, unsigned op, int in_place, const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* total32) {
  if (tile_log < POLY_TILE_LOG_MIN || tile_log > POLY_TILE_LOG_MAX || (flags & ~(kScanNormal | kScanInclusive)) || op > kScanSum || n > ((uint64_t)1 << 24) ||
      (n && (!in || !out)))
    return -1;
  return POLY_FIELD(t_scan, tile_log, flags, op, in_place, in, n, out, total32);
}
// mi355_msm_domain_permutation_product on the host, for the domain of 2^k rows
int ht_scan_permutation_product(int field, unsigned k, unsigned tile_log, unsigned flags, unsigned m, uint64_t stride, const uint8_t* wires,
                                const uint8_t* sigmas, const uint8_t* ks, const uint8_t* beta, const uint8_t* gamma, uint8_t* out, uint8_t* total32) {
  if (tile_log < POLY_TILE_LOG_MIN || tile_log > POLY_TILE_LOG_MAX || (flags & ~kScanNormal) || k > 16 || m < 1 || m > SCAN_MAX_COLUMNS ||
      stride < ((uint64_t)1 << k) || stride > ((uint64_t)1 << 20) || !wires || !sigmas || !ks || !beta || !gamma || !out)
    return -1;
  return POLY_FIELD(t_scan_permutation, k, tile_log, flags, m, stride, wires, sigmas, ks, beta, gamma, out, total32);
}
}

// ---- the rows of the Plonk quotient and the linear combination (quotient.hpp): every row in order, and the chain of launches the
// engine runs ------------------------------------------------------------------------------------------------------------------------
#include "quotient.hpp"

template <class FR>
struct HostQuotRun : HostPolyRun<FR> {
  void xm1(const QuotXm1& p) {
    for (uint32_t i = 0; (i >> p.k) == 0; i++) quot_xm1_row<FR>(p, i);
  }
  void rows(const QuotRows& p) {
    for (uint32_t i = 0; (i >> p.k) == 0; i++) quot_row<FR>(p, i);
  }
};

// -1: refused as the engine refuses it (the offset is zero, or its n-th power is a root of unity of order `ratio`)
template <class FR>
static int t_quotient_rows(uint32_t k, uint32_t log_n, uint32_t tile_log, unsigned flags, uint32_t m, uint64_t stride, const uint8_t* wires,
                           const uint8_t* sigmas, const uint8_t* selectors, const uint8_t* z, const uint8_t* pi, const uint8_t* ks, const uint8_t* alpha,
                           const uint8_t* beta, const uint8_t* gamma, const uint8_t* offset, uint8_t* out) {
  const uint64_t M = (uint64_t)1 << k, span = (m - 1) * stride + M, sel_span = (QUOT_SELECTORS - 1) * stride + M;
  const bool normal = (flags & kQuotNormal) != 0;
  Fr root, zero, al, a2n;
  fr_zero(zero);
  ntt_root<FR>(root, k);
  std::vector<Fr> wlo, whi;
  t_ntt_two_level<FR>(wlo, whi, root, k);
  std::vector<uint32_t> w(span * 8), sg(span * 8), sel(selectors ? sel_span * 8 : 0), zz(M * 8), pp(pi ? M * 8 : 0), dst(M * 8);
  memcpy(w.data(), wires, span * 32);
  memcpy(sg.data(), sigmas, span * 32);
  if (selectors) memcpy(sel.data(), selectors, sel_span * 32);
  memcpy(zz.data(), z, M * 32);
  if (pi) memcpy(pp.data(), pi, M * 32);
  QuotRows p{};
  p.wires = w.data();
  p.sigmas = sg.data();
  p.selectors = selectors ? sel.data() : nullptr;
  p.z = zz.data();
  p.pi = pi ? pp.data() : nullptr;
  p.dst = dst.data();
  p.stride = stride;
  p.k = k;
  p.m = m;
  p.ratio = 1u << (k - log_n);
  quot_form<FR>(p.cin, p.cout, normal);
  p.w = NttTable{wlo.data(), whi.data()};
  if (offset) poly_scalar<FR>(p.g, offset, normal); else fr_set<FR>(p.g, FR::GENERATOR);
  if (memcmp(p.g.v, zero.v, sizeof zero.v) == 0) return -1;
  poly_scalar<FR>(al, alpha, normal);
  poly_scalar<FR>(p.beta, beta, normal);
  poly_scalar<FR>(p.gamma, gamma, normal);
  for (uint32_t j = 0; j < m; j++) poly_scalar<FR>(p.bks[j], ks + 32 * j, normal);
  if (!quot_constants<FR>(p, a2n, al, log_n)) return -1;
  std::vector<Fr> work(quot_work_elems(M, tile_log));
  HostQuotRun<FR> run;
  quot_chain<FR>(run, p, a2n, tile_log, work.data());
  memcpy(out, dst.data(), M * 32);
  return 0;
}

// in_place: the output is column 0, as a call with out == cols[0] has it
template <class FR>
static int t_linear_combination(unsigned flags, uint32_t m, const uint8_t* const* cols, const uint64_t* lens, const uint8_t* coeffs, int in_place,
                                uint8_t* out) {
  LinComb p{};
  std::vector<std::vector<uint32_t>> v(m);
  uint64_t n = 0;
  for (uint32_t j = 0; j < m; j++) n = lens[j] > n ? lens[j] : n;
  if (n == 0) return 0;
  for (uint32_t j = 0; j < m; j++) {
    v[j].resize((in_place && j == 0 ? n : lens[j]) * 8 + 8);
    if (lens[j]) memcpy(v[j].data(), cols[j], lens[j] * 32);
    p.cols[j] = v[j].data();
    p.lens[j] = (uint32_t)lens[j];
    poly_scalar<FR>(p.coeffs[j], coeffs + 32 * j, (flags & kQuotNormal) != 0);
  }
  std::vector<uint32_t> dst(n * 8);
  p.dst = in_place ? v[0].data() : dst.data();
  p.n = (uint32_t)n;
  p.m = m;
  quot_form<FR>(p.cin, p.cout, (flags & kQuotNormal) != 0);
  for (uint32_t i = 0; i < p.n; i++) lincomb_elem<FR>(p, i);
  memcpy(out, p.dst, n * 32);
  return 0;
}

extern "C" {
// mi355_msm_domain_plonk_quotient on the host, for the quotient domain of 2^k points over a constraint domain of 2^log_n rows;
// selectors, pi and offset may be NULL
int ht_quotient_rows(int field, unsigned k, unsigned log_n, unsigned tile_log, unsigned flags, unsigned m, uint64_t stride, const uint8_t* wires,
                     const uint8_t* sigmas, const uint8_t* selectors, const uint8_t* z, const uint8_t* pi, const uint8_t* ks, const uint8_t* alpha,
                     const uint8_t* beta, const uint8_t* gamma, const uint8_t* offset, uint8_t* out) {
  if (tile_log < POLY_TILE_LOG_MIN || tile_log > POLY_TILE_LOG_MAX || (flags & ~kQuotNormal) || k > 16 || log_n >= k || k - log_n > 4 || log_n == 0 ||
      (selectors ? m != QUOT_GATE_WIRES : (m < 1 || m > QUOT_MAX_COLUMNS)) || stride < ((uint64_t)1 << k) || stride > ((uint64_t)1 << 20) || !wires ||
      !sigmas || !z || !ks || !alpha || !beta || !gamma || !out)
    return -1;
  return POLY_FIELD(t_quotient_rows, k, log_n, tile_log, flags, m, stride, wires, sigmas, selectors, z, pi, ks, alpha, beta, gamma, offset, out);
}
// mi355_msm_domain_linear_combination on the host
int ht_quotient_linear_combination(int field, unsigned flags, unsigned m, const uint8_t* const* cols, const uint64_t* lens, const uint8_t* coeffs,
                                   int in_place, uint8_t* out) {
  if ((flags & ~kQuotNormal) || m < 1 || m > LINCOMB_MAX_COLUMNS || !cols || !lens || !coeffs || !out) return -1;
  for (unsigned j = 0; j < m; j++)
    if (lens[j] > ((uint64_t)1 << 24) || (lens[j] && !cols[j])) return -1;
  return POLY_FIELD(t_linear_combination, flags, m, cols, lens, coeffs, in_place, out);
}
}

// ---- sparse matrices and y = M z (sparse.hpp): the plan create derives, the coefficients slot by slot, and the chain of launches the
// engine runs, every lane in order --------------------------------------------------------------------------------------------------
#include "sparse.hpp"

template <class FR>
struct HostSparseRun {
  uint32_t tile_log;
  void z(const SparseZ& p) {
    for (uint32_t i = 0; i < p.cols; i++) sparse_z_elem<FR>(p, i);
  }
  void totals(const SparseRun& p) {
    for (uint32_t t = 0; t < p.m.nlanes; t++) sparse_total<FR>(p, t);
  }
  void rows(const SparseRun& p) {
    for (uint32_t t = 0; t < p.m.nlanes; t++) sparse_rows_lane<FR>(p, t);
  }
  void cross(const SparseRun& p) {
    for (uint32_t r = 0; r < p.m.rows; r++) sparse_cross_row<FR>(p, r);
  }
  void scan(uint32_t* v, uint64_t n) {
    std::vector<Fr> work(scan_work_elems(n, tile_log));
    HostScanRun<FR> run;
    scan_chain<FR, kScanSum>(run, v, v, nullptr, n, false, false, tile_log, work.data());
  }
};

template <class FR>
static int t_sparse_apply(uint32_t tile_log, unsigned create_flags, unsigned flags, uint64_t rows, uint64_t cols, const uint64_t* row_ptr,
                          const uint32_t* col_idx, const uint8_t* values, const uint8_t* z, uint8_t* out) {
  char why[256];
  if (!sparse_validate(rows, cols, row_ptr, col_idx, why, sizeof why)) return -1;
  SparsePlan pl;
  sparse_plan(pl, rows, row_ptr, col_idx);
  std::vector<uint32_t> raw((size_t)pl.nnz * 8 + 8), vals((size_t)pl.slots * 8 + 8), zz(cols * 8 + 8), dst(rows * 8 + 8, 0xa5a5a5a5u);
  if (pl.nnz) memcpy(raw.data(), values, (size_t)pl.nnz * 32);
  if (cols) memcpy(zz.data(), z, cols * 32);
  const SparseVals vp{raw.data(), vals.data(), pl.nnz, pl.slots, (create_flags & kSparseNormal) ? 1u : 0u};
  for (uint32_t s = 0; s < pl.slots; s++) sparse_val_slot<FR>(vp, s);
  const SparseMat m{vals.data(),  pl.col.data(), pl.ne_end.data(), pl.ne_row.data(), pl.lane_row.data(), pl.row_ptr.data(),
                    (uint32_t)rows, (uint32_t)cols, pl.nnz,        pl.nne,           pl.nlanes,          pl.slots};
  std::vector<uint64_t> work(sparse_work_bytes(cols, pl.nlanes) / 8 + 4);
  void* w32 = (void*)(((uintptr_t)work.data() + 31) & ~(uintptr_t)31);
  HostSparseRun<FR> run{tile_log};
  sparse_chain<FR>(run, m, dst.data(), zz.data(), (flags & kSparseNormal) != 0, w32);
  if (rows) memcpy(out, dst.data(), rows * 32);
  return 0;
}

extern "C" {
// mi355_msm_sparse_create + _apply on the host: create_flags bit 0, the values are plain integers; flags bit 0, z and out are plain integers
unsigned ht_sparse_entries_per_lane(void) { return SPARSE_E; }
unsigned ht_sparse_block_lanes(void) { return SPARSE_LANES; }
int ht_sparse_apply(int field, unsigned tile_log, unsigned create_flags, unsigned flags, uint64_t rows, uint64_t cols, const uint64_t* row_ptr,
                    const uint32_t* col_idx, const uint8_t* values, const uint8_t* z, uint8_t* out) {
  if (tile_log < POLY_TILE_LOG_MIN || tile_log > POLY_TILE_LOG_MAX || (create_flags & ~kSparseNormal) || (flags & ~kSparseNormal) || rows > ((uint64_t)1 << 20) ||
      cols > ((uint64_t)1 << 20) || !row_ptr || row_ptr[rows] > ((uint64_t)1 << 22) || (row_ptr[rows] && (!col_idx || !values)) || (cols && !z) || (rows && !out))
    return -1;
  return POLY_FIELD(t_sparse_apply, tile_log, create_flags, flags, rows, cols, row_ptr, col_idx, values, z, out);
}
}

// ---- multilinear extensions and sumcheck rounds (mle.hpp): the chains of launches the engine runs, every block lane by lane, with the
// limb-bound checker armed ---------------------------------------------------------------------------------------------------------
#include "mle.hpp"

template <class FR>
struct HostMleRun {
  std::vector<Fr> lds;
  HostMleRun() : lds(POLY_MAX_TILE) {}
  void tree(uint32_t lanes) {
    for (uint32_t s = 0; (2u << s) <= lanes; s++)
      for (uint32_t l = 0; l < (lanes >> (s + 1)); l++) mle_tree_level<FR>(lds.data(), lanes, s, l);
  }
  void fix(const MleFix& p) {
    const uint32_t T = 1u << p.tile_log;
    for (uint64_t tile = 0; tile < (p.n >> p.tile_log); tile++) {
      for (uint32_t i = 0; i < T; i++) mle_fix_load<FR>(lds.data(), p, tile << p.tile_log, i);
      for (uint32_t s = 0; s < p.kk; s++)
        for (uint32_t j = 0; j < (T >> (s + 1)); j++) mle_fix_level<FR>(lds.data(), p, s, j);
      for (uint32_t i = 0; i < (T >> p.kk); i++) mle_fix_store<FR>(lds.data(), p, tile, i);
    }
  }
  void eq(const MleEq& p) {
    for (uint64_t b = 0; b < p.n; b++) mle_eq_elem<FR>(p, b);
  }
  template <int D>
  void round(const MleRound& p) {
    const uint32_t lanes = poly_lanes(p.tile_log);
    std::vector<Fr> acc((size_t)lanes * (D + 1));
    for (uint64_t blk = 0; blk < mle_blocks(p.npts, p.tile_log); blk++) {
      for (uint32_t l = 0; l < lanes; l++) {
        Fr a[D + 1];
        mle_round_lane<FR, D>(a, p, blk, l);
        for (int t = 0; t <= D; t++) acc[(size_t)l * (D + 1) + t] = a[t];
      }
      for (int t = 0; t <= D; t++) {
        for (uint32_t l = 0; l < lanes; l++) lds[l] = acc[(size_t)l * (D + 1) + t];
        tree(lanes);
        poly_store_m<FR>(p.part + blk * MLE_EVALS + t, lds[0]);
      }
    }
  }
  void sum(const MleSum& p) {
    const uint32_t lanes = poly_lanes(p.tile_log);
    for (uint64_t blk = 0; blk < mle_blocks(p.n, p.tile_log); blk++)
      for (uint32_t t = 0; t < p.ne; t++) {
        for (uint32_t l = 0; l < lanes; l++) mle_sum_lane<FR>(lds[l], p, blk, l, t);
        tree(lanes);
        poly_store_m<FR>(p.dst + blk * MLE_EVALS + t, lds[0]);
      }
  }
};

template <class FR>
static int t_mle_fix(uint32_t tile_log, unsigned flags, uint32_t nv, uint32_t k, const uint8_t* in, const uint8_t* point, uint8_t* out) {
  const bool normal = (flags & kMleNormal) != 0;
  const size_t n_in = (size_t)1 << nv, n_out = (size_t)1 << (nv - k);
  std::vector<uint32_t> src(n_in * 8), dst(n_out * 8, 0xa5a5a5a5u);
  memcpy(src.data(), in, n_in * 32);
  std::vector<Fr> work(mle_fix_work_elems(nv, k, tile_log) + 2);
  Fr pt[MLE_MAX_VARS];
  for (uint32_t i = 0; i < k; i++) poly_scalar<FR>(pt[i], point + 32 * i, normal);
  HostMleRun<FR> run;
  mle_chain_fix<FR>(run, dst.data(), src.data(), nv, pt, k, normal, tile_log, work.data());
  memcpy(out, dst.data(), n_out * 32);
  return 0;
}

template <class FR>
static int t_mle_eq(unsigned flags, uint32_t k, const uint8_t* point, uint8_t* out) {
  const bool normal = (flags & kMleNormal) != 0;
  const uint32_t lo_log = (k + 1) / 2;
  std::vector<uint32_t> dst(((size_t)8) << k, 0xa5a5a5a5u);
  std::vector<Fr> lo, hi;
  Fr pt[MLE_MAX_VARS], one, cout;
  for (uint32_t i = 0; i < k; i++) poly_scalar<FR>(pt[i], point + 32 * i, normal);
  fr_set<FR>(one, FR::ONE);
  fr_const<FR>(cout, normal ? 3 : 2);
  mle_eq_half<FR>(lo, pt, lo_log, one);
  mle_eq_half<FR>(hi, pt + lo_log, k - lo_log, cout);
  HostMleRun<FR> run;
  mle_chain_eq<FR>(run, dst.data(), lo.data(), hi.data(), k);
  memcpy(out, dst.data(), (size_t)32 << k);
  return 0;
}

template <class FR>
static int t_mle_round(uint32_t tile_log, unsigned flags, uint32_t m, uint32_t nv, const uint8_t* tables, uint32_t n_terms, const uint8_t* coeffs,
                       const uint32_t* nfs, const uint32_t* factors, const uint8_t* r_prev, uint8_t* folded, uint8_t* evals_out) {
  const bool normal = (flags & kMleNormal) != 0, fused = r_prev != nullptr;
  const size_t n_in = (size_t)1 << nv, n_half = n_in / 2;
  std::vector<uint32_t> src((size_t)m * n_in * 8), fold(fused ? (size_t)m * n_half * 8 : 8, 0xa5a5a5a5u);
  memcpy(src.data(), tables, (size_t)m * n_in * 32);
  MleRound p{};
  p.npts = (fused ? n_half : n_in) / 2;
  p.m = m;
  p.n_terms = n_terms;
  p.tile_log = tile_log;
  p.fused = fused ? 1u : 0u;
  fr_const<FR>(p.cin, normal ? 1 : 0);
  fr_const<FR>(p.cout, normal ? 3 : 2);
  uint32_t D = 0;
  for (uint32_t i = 0; i < m; i++) {
    p.src[i] = src.data() + (size_t)i * n_in * 8;
    p.folded[i] = fold.data() + (size_t)i * n_half * 8;
    p.tab[i] = fused ? p.folded[i] : p.src[i];
  }
  for (uint32_t j = 0; j < n_terms; j++) {
    poly_scalar<FR>(p.term[j].c, coeffs + 32 * j, normal);
    p.term[j].nf = nfs[j];
    for (uint32_t q = 0; q < nfs[j]; q++) p.term[j].f[q] = factors[j * MLE_MAX_FACTORS + q];
    if (nfs[j] > D) D = nfs[j];
  }
  if (fused) {
    Fr r;
    poly_scalar<FR>(r, r_prev, normal);
    mle_one_minus<FR>(p.fa, r);
    mle_mul_canon<FR>(p.fa, p.fa, p.cin);
    mle_mul_canon<FR>(p.fb, r, p.cin);
  }
  std::vector<Fr> work(mle_round_work_elems(p.npts, tile_log) + 2);
  HostMleRun<FR> run;
  const Fr* res = mle_chain_round<FR>(run, p, D, work.data());
  for (uint32_t t = 0; t <= D; t++) poly_scalar_out<FR>(evals_out + 32 * t, res[t], normal);
  if (fused) memcpy(folded, fold.data(), (size_t)m * n_half * 32);
  return (int)mle_round_levels(p.npts, tile_log);
}

extern "C" {
// mi355_msm_domain_mle_fix / mle_eq / sumcheck_round on the host; flags bit 0: plain integers.  The tables of a round lie one behind
// the other, the folded ones too; factors holds MLE_MAX_FACTORS indices per term; ht_mle_round returns the launches of the round.
int ht_mle_fix(int field, unsigned tile_log, unsigned flags, unsigned nv, unsigned k, const uint8_t* in, const uint8_t* point, uint8_t* out) {
  if (tile_log < POLY_TILE_LOG_MIN || tile_log > POLY_TILE_LOG_MAX || (flags & ~kMleNormal) || nv > 20 || k > nv || !in || !out || (k && !point)) return -1;
  return POLY_FIELD(t_mle_fix, tile_log, flags, nv, k, in, point, out);
}
int ht_mle_eq(int field, unsigned flags, unsigned k, const uint8_t* point, uint8_t* out) {
  if ((flags & ~kMleNormal) || k > 20 || !out || (k && !point)) return -1;
  return POLY_FIELD(t_mle_eq, flags, k, point, out);
}
int ht_mle_round(int field, unsigned tile_log, unsigned flags, unsigned m, unsigned nv, const uint8_t* tables, unsigned n_terms, const uint8_t* coeffs,
                 const uint32_t* nfs, const uint32_t* factors, const uint8_t* r_prev, uint8_t* folded, uint8_t* evals_out) {
  if (tile_log < POLY_TILE_LOG_MIN || tile_log > POLY_TILE_LOG_MAX || (flags & ~kMleNormal) || m < 1 || m > MLE_MAX_TABLES || nv < 1 || nv > 16 ||
      n_terms < 1 || n_terms > MLE_MAX_TERMS || !tables || !coeffs || !nfs || !factors || !evals_out || (r_prev && (nv < 2 || !folded)))
    return -1;
  for (unsigned j = 0; j < n_terms; j++) {
    if (nfs[j] < 1 || nfs[j] > MLE_MAX_FACTORS) return -1;
    for (unsigned q = 0; q < nfs[j]; q++)
      if (factors[j * MLE_MAX_FACTORS + q] >= m) return -1;
  }
  return POLY_FIELD(t_mle_round, tile_log, flags, m, nv, tables, n_terms, coeffs, nfs, factors, r_prev, folded, evals_out);
}
}

// ---- Poseidon sponges and Merkle trees (poseidon.hpp): the table create derives and the kernel body, lane by lane, with the limb-bound
// checker armed ---------------------------------------------------------------------------------------------------------------------
#include "poseidon.hpp"

template <class FR>
struct HostPosRun {
  void hash(const PosRun& p) {
    if (p.n_out == 0) return;
    std::vector<uint32_t> state((size_t)2 * p.tab.t * FR_NL);
    for (uint64_t i = 0; i < p.n; i++) pos_lane<FR>(PosState<1>{state.data()}, p, i);
  }
  void fill(uint32_t* first, uint64_t count) {
    for (uint64_t i = 1; i < count; i++) memcpy(first + i * 8, first, 32);
  }
};

template <class FR>
static int t_pos_plan(PosPlan& pl, std::vector<uint8_t>& img, PosTab& tab, unsigned create_flags, uint32_t rate, uint32_t alpha, uint32_t rf, uint32_t rp,
                      const uint8_t* ark, const uint8_t* mds) {
  const uint32_t t = rate + 1;
  std::vector<Fr> a((size_t)(rf + rp) * t), m((size_t)t * t);
  for (size_t i = 0; i < a.size(); i++) poly_scalar<FR>(a[i], ark + 32 * i, (create_flags & kPosNormal) != 0);
  for (size_t i = 0; i < m.size(); i++) poly_scalar<FR>(m[i], mds + 32 * i, (create_flags & kPosNormal) != 0);
  char why[256];
  if (!pos_build<FR>(pl, rate, alpha, rf, rp, a.data(), m.data(), why, sizeof why)) return -2;
  pos_table_fill(img, pl);
  tab = pos_table_at(img.data(), pl);
  return 0;
}

template <class FR>
static PosRun t_pos_base(const PosTab& tab, unsigned flags, int sparse) {
  PosRun r{};
  r.tab = tab;
  r.sparse = sparse ? 1u : 0u;
  fr_const<FR>(r.cin, (flags & kPosNormal) ? 1 : 0);
  fr_const<FR>(r.cout, (flags & kPosNormal) ? 3 : 2);
  return r;
}

template <class FR>
static int t_pos_hash(unsigned create_flags, unsigned flags, uint32_t rate, uint32_t alpha, uint32_t rf, uint32_t rp, const uint8_t* ark, const uint8_t* mds,
                      int sparse, uint64_t n, uint32_t in_len, uint32_t n_out, const uint8_t* header, const uint8_t* in, uint8_t* out) {
  PosPlan pl;
  std::vector<uint8_t> img;
  PosTab tab;
  if (int e = t_pos_plan<FR>(pl, img, tab, create_flags, rate, alpha, rf, rp, ark, mds)) return e;
  // buffers of the exact size
  std::vector<uint32_t> src(n * in_len * 8), dst(n * n_out * 8, 0xa5a5a5a5u);
  if (src.size()) memcpy(src.data(), in, src.size() * 4);
  PosRun r = t_pos_base<FR>(tab, flags, sparse);
  r.in = src.data();
  r.out = dst.data();
  r.n = n;
  r.row_stride = in_len;
  r.in_len = in_len;
  r.n_out = n_out;
  r.has_header = header ? 1u : 0u;
  if (header)
    for (uint32_t e = 0; e < rate; e++) poly_scalar<FR>(r.hdr[e], header + 32 * e, (flags & kPosNormal) != 0);
  HostPosRun<FR> run;
  run.hash(r);
  if (dst.size()) memcpy(out, dst.data(), dst.size() * 4);
  return 0;
}

template <class FR>
static int t_pos_merkle(unsigned create_flags, unsigned flags, uint32_t rate, uint32_t alpha, uint32_t rf, uint32_t rp, const uint8_t* ark, const uint8_t* mds,
                        int sparse, uint64_t n_leaves, uint32_t leaf_len, const uint8_t* domain_sep, const uint8_t* leaves, uint8_t* tree_out) {
  PosPlan pl;
  std::vector<uint8_t> img;
  PosTab tab;
  if (int e = t_pos_plan<FR>(pl, img, tab, create_flags, rate, alpha, rf, rp, ark, mds)) return e;
  uint64_t P = 1;
  while (P < n_leaves) P *= 2;
  std::vector<uint32_t> src(n_leaves * leaf_len * 8), dst((2 * P - 1) * 8, 0xa5a5a5a5u), zeros(16, 0);
  if (src.size()) memcpy(src.data(), leaves, src.size() * 4);
  const PosRun base = t_pos_base<FR>(tab, flags, sparse);
  Fr hl[POS_MAX_RATE], hn[POS_MAX_RATE];
  for (uint32_t e = 0; e < POS_MAX_RATE; e++) {
    fr_zero(hl[e]);
    fr_zero(hn[e]);
  }
  uint8_t len[32] = {0};
  poly_scalar<FR>(hl[0], domain_sep, (flags & kPosNormal) != 0);
  hn[0] = hl[0];
  for (int q = 0; q < 4; q++) len[q] = (uint8_t)((leaf_len + 1) >> (8 * q));
  poly_scalar<FR>(hl[1], len, true);
  len[0] = 3;
  len[1] = len[2] = len[3] = 0;
  poly_scalar<FR>(hn[1], len, true);
  HostPosRun<FR> run;
  pos_merkle_chain(run, base, dst.data(), src.data(), n_leaves, leaf_len, hl, hn, zeros.data());
  memcpy(tree_out, dst.data(), dst.size() * 4);
  return 0;
}

template <class FR>
static int t_pos_permute(unsigned create_flags, uint32_t rate, uint32_t alpha, uint32_t rf, uint32_t rp, const uint8_t* ark, const uint8_t* mds, int sparse,
                         const uint8_t* state_in, uint8_t* state_out, uint64_t* info) {
  PosPlan pl;
  std::vector<uint8_t> img;
  PosTab tab;
  if (int e = t_pos_plan<FR>(pl, img, tab, create_flags, rate, alpha, rf, rp, ark, mds)) return e;
  const uint32_t t = rate + 1;
  std::vector<uint32_t> state((size_t)2 * t * FR_NL);
  const PosState<1> st{state.data()};
  for (uint32_t e = 0; e < t; e++) {
    Fr x;
    poly_scalar<FR>(x, state_in + 32 * e, true);
    st.store(e, x);
  }
  const uint32_t cur = pos_permute<FR>(st, tab, sparse != 0, 0);
  for (uint32_t e = 0; e < t; e++) {
    Fr x;
    st.load(x, cur * t + e);
    poly_scalar_out<FR>(state_out + 32 * e, x, true);
  }
  if (info) {
    info[0] = pl.products_d;
    info[1] = pl.products_s;
    info[2] = info[3] = 0;
    for (uint32_t f : pl.red_d) info[2] += (f != 0);
    for (uint32_t f : pl.red_s) info[3] += (f != 0);
  }
  return 0;
}

extern "C" {
// mi355_msm_poseidon_create + _hash / _merkle on the host: create_flags bit 0, ark and mds are plain integers; flags bit 0, the elements
// of the call are.  -2: create refuses the parameters.  ht_poseidon_permute: one permutation of t plain integers; info receives the
// products of the dense and the sparse form and the rounds with a reduction in each.
unsigned ht_poseidon_block_lanes(void) { return POS_LANES; }
static int ht_pos_shape(int field, unsigned create_flags, unsigned rate, unsigned alpha, unsigned rf, unsigned rp, const void* ark, const void* mds) {
  return (field == 0 || field == 1) && !(create_flags & ~kPosNormal) && !pos_check_shape(rate, alpha, rf, rp) && ark && mds;
}
int ht_poseidon_hash(int field, unsigned create_flags, unsigned flags, unsigned rate, unsigned alpha, unsigned rf, unsigned rp, const uint8_t* ark,
                     const uint8_t* mds, int sparse, uint64_t n, unsigned in_len, unsigned n_out, const uint8_t* header, const uint8_t* in, uint8_t* out) {
  if (!ht_pos_shape(field, create_flags, rate, alpha, rf, rp, ark, mds) || (flags & ~kPosNormal) || n > (1u << 16) || in_len > 4096 || n_out > 4096 ||
      (n && in_len && !in) || (n && n_out && !out))
    return -1;
  return POLY_FIELD(t_pos_hash, create_flags, flags, rate, alpha, rf, rp, ark, mds, sparse, n, in_len, n_out, header, in, out);
}
int ht_poseidon_merkle(int field, unsigned create_flags, unsigned flags, unsigned rate, unsigned alpha, unsigned rf, unsigned rp, const uint8_t* ark,
                       const uint8_t* mds, int sparse, uint64_t n_leaves, unsigned leaf_len, const uint8_t* domain_sep, const uint8_t* leaves, uint8_t* tree_out) {
  if (!ht_pos_shape(field, create_flags, rate, alpha, rf, rp, ark, mds) || (flags & ~kPosNormal) || rate < 2 || n_leaves < 1 || n_leaves > (1u << 12) ||
      leaf_len > 4096 || !domain_sep || (leaf_len && !leaves) || !tree_out)
    return -1;
  return POLY_FIELD(t_pos_merkle, create_flags, flags, rate, alpha, rf, rp, ark, mds, sparse, n_leaves, leaf_len, domain_sep, leaves, tree_out);
}
int ht_poseidon_permute(int field, unsigned create_flags, unsigned rate, unsigned alpha, unsigned rf, unsigned rp, const uint8_t* ark, const uint8_t* mds,
                        int sparse, const uint8_t* state_in, uint8_t* state_out, uint64_t* info) {
  if (!ht_pos_shape(field, create_flags, rate, alpha, rf, rp, ark, mds) || !state_in || !state_out) return -1;
  return POLY_FIELD(t_pos_permute, create_flags, rate, alpha, rf, rp, ark, mds, sparse, state_in, state_out, info);
}
}

// ---- pairings (pairing.hpp): the programs create writes and the three stage bodies, lane by lane, with the limb-bound checker armed -----
#include "pairing.hpp"

template <class E>
struct HostPrRun {
  void miller(const PrRun& p, uint64_t items) { for (uint64_t i = 0; i < items; i++) pr_miller_lane<E>(p, i); }
  void product(const PrRun& p, uint64_t lanes) { for (uint64_t i = 0; i < lanes; i++) pr_product_lane<E>(p, i); }
  void final(const PrRun& p, uint64_t groups) { for (uint64_t i = 0; i < groups; i++) pr_final_lane<E>(p, i); }
};

template <class E>
static int t_pr_run(uint8_t* out, const uint8_t* g1, size_t g1_stride, const uint8_t* g2, size_t g2_stride, size_t n, size_t group, unsigned flags, int check) {
  PrGen<E> gm, ga, gf;
  gm.miller();
  ga.accumulate();
  gf.final_exponentiation();
  if (!gm.check() || !ga.check() || !gf.check()) return -3;
  Fe2 consts[PR_CONSTS];
  pr_consts<E>(consts, check || (flags & kPrCanonical));
  const PrPlan pl = pr_plan(n, group);
  std::vector<uint32_t> ws(pr_ws_words(pl), 0xa5a5a5a5u), wsf(pr_wsf_words(pl), 0xa5a5a5a5u);
  std::vector<uint32_t> a((n * g1_stride + 3) / 4), b((n * g2_stride + 3) / 4), o(((n / group) * (check ? 1 : PR_GT_BYTES) + 3) / 4 + 1);
  memcpy(a.data(), g1, n * g1_stride);
  memcpy(b.data(), g2, n * g2_stride);
  PrRun r{};
  r.miller = gm.ops.data(); r.miller_len = (uint32_t)gm.ops.size();
  r.accum = ga.ops.data(); r.accum_len = (uint32_t)ga.ops.size();
  r.fexp = gf.ops.data(); r.fexp_len = (uint32_t)gf.ops.size();
  r.consts = consts;
  r.ws = ws.data(); r.pitch = pr_ws_items(pl);
  r.ws_f = wsf.data(); r.pitch_f = pl.chunk_groups;
  r.g1 = (const uint8_t*)a.data(); r.g1_stride = g1_stride;
  r.g2 = (const uint8_t*)b.data(); r.g2_stride = g2_stride;
  r.group = pl.group; r.run = pl.run; r.parts = pl.parts;
  r.flags = (flags & kPrCanonical) | (check ? (unsigned)kPrCheck : 0u);
  HostPrRun<E> run;
  pr_chain(run, r, pl, (uint8_t*)o.data(), check ? 1 : PR_GT_BYTES);
  memcpy(out, o.data(), (n / group) * (check ? 1 : PR_GT_BYTES));
  return 0;
}

// one tower routine on canonical Gt images: A in PR_F, B in PR_G, the result in PR_ACC
template <class E>
static int t_pr_op(int op, uint8_t* out, const uint8_t* a, const uint8_t* b, unsigned top) {
  using F = typename E::Fld;
  const Modulus<F> md;
  PrGen<E> g;
  const uint16_t A = PR_F, B = PR_G, R = PR_ACC, S = PR_REGION0;
  switch (op) {
    case 0: g.f12_mul(R, A, B); break;
    case 1: g.f12_sqr(R, A); break;
    case 2: g.f12_inv(R, S, A); break;
    case 3: g.f12_mul(R, A, B, 0x0b); break;   // 034: w^0, w^1, w^3
    case 4: g.f12_mul(R, A, B, 0x0d); break;   // 014: w^0, w^2, w^3
    case 5: g.f12_cyclotomic_sqr(R, A); break;
    case 6: g.f12_cyclotomic_exp(R, S, A); break;
    case 7: case 8: case 9: g.f12_frobenius(R, A, op - 6); break;
    case 10: g.f12_conj(R, A); break;
    case 11: g.f12_mul(R, A, B, 0x15); break;  // Fp6: the even coefficients
    case 12: g.f12_sqr(R, A); break;
    case 13: g.f12_copy(R, A); g.f6_inv(R, R + 2, R + 4, R, R + 2, R + 4); break;
    default: return -1;
  }
  if (!g.check()) return -3;
  Fe2 consts[PR_CONSTS];
  pr_consts<E>(consts, true);
  std::vector<uint32_t> wsv((size_t)PR_SLOTS * PR_FE2_WORDS, 0);
  const PrWs ws{wsv.data(), 1, 0};
  auto load = [&](uint16_t base, const uint8_t* img) {
    for (uint32_t t = 0; t < 12; t++) {
      const uint32_t e = t >> 1, slot = 2 * (e % 3) + e / 3;
      uint32_t w[12];
      memcpy(w, img + 48 * t, 48);
      Fe x, pp;
      FpEl<F>::from_plain(x, w, md);
      if (top) {   // the residue plus 2p: the top of class W
        fe_reduce<F>(x);
        fe_set(pp, F::P);
        fe_add(x, x, pp);
        fe_add(x, x, pp);
        fe_normalize(x);
      }
      pr_store_fe(ws, base + slot, t & 1, x);
    }
  };
  load(A, a);
  if (b) load(B, b);
  pr_exec<E>(ws, g.ops.data(), (uint32_t)g.ops.size(), consts, false, md);
  for (uint32_t t = 0; t < 12; t++) {
    const uint32_t e = t >> 1, slot = 2 * (e % 3) + e / 3;
    Fe x;
    pr_load_fe(x, ws, R + slot, t & 1);
    uint32_t w[12];
    FpEl<F>::to_plain(w, x, md);
    memcpy(out + 48 * t, w, 48);
  }
  return 0;
}

template <class E>
static int t_pr_info(uint64_t* v) {
  PrGen<E> gm, ga, gf;
  gm.miller();
  ga.accumulate();
  gf.final_exponentiation();
  v[0] = gm.products - ga.products;   // Fp2 products of one Miller loop (the accumulation into the run's product apart)
  v[1] = gf.products;
  v[2] = ga.products;
  v[3] = gm.ops.size();
  v[4] = gf.ops.size();
  v[5] = PR_SLOTS;
  v[6] = PR_LANES;
  v[7] = PR_MILLER_SLOTS;
  v[8] = ga.ops.size();
  v[9] = PR_MAX_ITEMS;
  return 0;
}

#define PR_FAMILY(fn, ...) (family == 0 ? fn<Fp2El<Bls12_377_Fq, 5>>(__VA_ARGS__) : fn<Fp2El<Bls12_381_Fq, 1>>(__VA_ARGS__))
extern "C" {
// mi355_msm_pairing_run / _check on the host (family 0: BLS12-377, 1: BLS12-381; flags bit 0: canonical images; check: one byte per group);
// ht_pairing_op: one tower routine on canonical Gt images (top: the operands stored at the top of their class);  ht_pairing_info: the
// Fp2 products of a Miller loop, a final exponentiation and a product step, the lengths of these two programs, the slots, the lanes of a
// block, the slots of a Miller lane, the length of the product step and the lanes of a chunk (ten values).
int ht_pairing_run(int family, uint8_t* out, const uint8_t* g1, size_t g1_stride, const uint8_t* g2, size_t g2_stride, size_t n, size_t group, unsigned flags,
                   int check) {
  if ((family != 0 && family != 1) || (flags & ~1u) || group == 0 || n % group || g1_stride < 104 || g2_stride < 200 || (g1_stride & 3) || (g2_stride & 3) ||
      n > (1u << 16) || (n && (!out || !g1 || !g2)))
    return -1;
  if (n == 0) return 0;
  return PR_FAMILY(t_pr_run, out, g1, g1_stride, g2, g2_stride, n, group, flags, check);
}
int ht_pairing_op(int family, int op, uint8_t* out, const uint8_t* a, const uint8_t* b, unsigned top) {
  if ((family != 0 && family != 1) || !out || !a) return -1;
  return PR_FAMILY(t_pr_op, op, out, a, b, top);
}
int ht_pairing_info(int family, uint64_t* v) {
  if ((family != 0 && family != 1) || !v) return -1;
  return PR_FAMILY(t_pr_info, v);
}
}

// ---- transforms of vectors of points (group_fft.hpp) with the limb-bound checker armed ------------------------------------------
// The SAME MSM_HD functions the kernels of kernels_gfft.hip wrap: the index maps, the twiddle exponent, the twiddle and the factor as
// canonical words, the table of a butterfly's B, the walk and the butterfly; records by fb_host_records, the vector between two
// stages and the output by fb_normalize_run, in the order msm_gfft.hpp launches them (one chunk).
#include "group_fft.hpp"

template <class E>
static void gf_host_emit(const std::vector<XyzzDevT<typename E::T>>& res, bool projective, uint8_t* out, size_t out_stride, const typename E::Md& md) {
  pm_host_output<E>(res, projective ? 2u : 0u, out, out_stride, md);
}

template <class E>
static void gf_host_scale(const GfVec& v, size_t count, const GfScale& fs, uint32_t k, uint32_t w, bool projective, uint8_t* dst, size_t dstride,
                          const typename E::Md& md) {
  using El = typename E::T;
  const uint32_t entries = pm_table_entries(w);
  std::vector<XyzzT<El>> x(entries);
  std::vector<AffineDevT<El>> table(entries);
  std::vector<XyzzDevT<El>> res(count);
  for (size_t j = 0; j < count; j++) {
    uint32_t sc[8];
    gf_scale_words<GfFr<E>>(sc, fs, k, (uint32_t)j);
    gf_table<E>(x.data(), 1, v, (uint32_t)j, entries, md);
    fb_host_records<E>(table.data(), x.data(), entries, md);
    pm_windowed_mul<E>(res[j].p, table.data(), 1, sc, w, pm_top_window(pm_bit_length(sc), w), md);
  }
  gf_host_emit<E>(res, projective, dst, dstride, md);
}

template <class C>
static int t_gf_transform(uint32_t k, unsigned kind, const uint8_t* offset, const uint8_t* in, size_t stride, uint32_t in_len, uint32_t w, unsigned flags,
                          uint8_t* out, size_t out_stride) {
  using E = typename C::E;
  using El = typename E::T;
  using FR = GfFr<E>;
  typename E::Md md;
  const size_t n = (size_t)1 << k, half = n / 2, img0 = 8 * E::WORDS + 8;
  const bool inverse = (kind & kNttKindInverse) != 0, coset = (kind & kNttKindCoset) != 0, projective = (flags & kGfProjective) != 0;
  const uint32_t entries = pm_table_entries(w);
  Fr root, g;
  ntt_root<FR>(root, k);
  if (offset) {
    uint32_t ow[8];
    memcpy(ow, offset, 32);
    fr_from_abi<FR>(g, ow, false);
    fr_reduce<FR>(g);
  } else {
    fr_set<FR>(g, FR::GENERATOR);
  }
  if (inverse) {
    fr_inv<FR>(root, root);
    fr_inv<FR>(g, g);
  }
  std::vector<Fr> wlo, whi, glo, ghi;
  t_ntt_two_level<FR>(wlo, whi, root, k);
  t_ntt_two_level<FR>(glo, ghi, g, k);
  const NttTable tw{wlo.data(), whi.data()};
  GfScale fs{};
  fs.g = NttTable{glo.data(), ghi.data()};
  ntt_size_inv<FR>(fs.scale, k);
  fs.has_g = coset;
  fs.has_scale = inverse;
  GfVec src{in, stride, in_len};
  if (k == 0) {
    std::vector<XyzzT<El>> x(1);
    gf_table<E>(x.data(), 1, src, 0, 1, md);
    std::vector<XyzzDevT<El>> res(1);
    res[0].p = x[0];
    gf_host_emit<E>(res, projective, out, out_stride, md);
    return 0;
  }
  std::vector<uint8_t> vec[2] = {std::vector<uint8_t>(n * img0), std::vector<uint8_t>(n * img0)};
  int cur = -1;
  if (coset && !inverse) {
    gf_host_scale<E>(src, in_len, fs, k, w, false, vec[0].data(), img0, md);
    cur = 0;
    src = GfVec{vec[0].data(), img0, in_len};
  }
  std::vector<XyzzT<El>> x(entries);
  std::vector<AffineDevT<El>> table(entries);
  std::vector<XyzzDevT<El>> res(n);
  for (uint32_t s = 0; s < k; s++) {
    const bool to_out = s + 1 == k && !inverse;
    const int nxt = cur == 0 ? 1 : 0;
    for (size_t b = 0; b < half; b++) {
      if (s == 0) {
        gf_butterfly_first<E>(&res[b].p, &res[half + b].p, src, k, (uint32_t)b, md);
        continue;
      }
      uint32_t sc[8];
      gf_twiddle_words<FR>(sc, tw, k, gf_twiddle_exp(k, s, (uint32_t)b));
      gf_table<E>(x.data(), 1, src, gf_index_b(k, s, (uint32_t)b), entries, md);
      fb_host_records<E>(table.data(), x.data(), entries, md);
      gf_butterfly_mul<E>(&res[b].p, &res[half + b].p, src, table.data(), 1, sc, w, pm_top_window(pm_bit_length(sc), w), k, s, (uint32_t)b, md);
    }
    if (to_out) {
      gf_host_emit<E>(res, projective, out, out_stride, md);
    } else {
      gf_host_emit<E>(res, false, vec[nxt].data(), img0, md);
      cur = nxt;
      src = GfVec{vec[cur].data(), img0, (uint32_t)n};
    }
  }
  if (inverse) gf_host_scale<E>(src, n, fs, k, w, projective, out, out_stride, md);
  return 0;
}

template <class FR>
static int t_gf_twiddles(uint32_t k, int inverse, const uint32_t* exps, size_t count, uint8_t* out) {
  Fr root;
  ntt_root<FR>(root, k);
  if (inverse) fr_inv<FR>(root, root);
  std::vector<Fr> lo, hi;
  t_ntt_two_level<FR>(lo, hi, root, k);
  const NttTable tw{lo.data(), hi.data()};
  for (size_t i = 0; i < count; i++) {
    if (exps[i] >> k) return -1;
    uint32_t w[8];
    gf_twiddle_words<FR>(w, tw, k, exps[i]);
    memcpy(out + 32 * i, w, 32);
  }
  return 0;
}

extern "C" {
// butterfly b of stage s of a transform of 2^k points: out = {index of A, index of B, twiddle exponent}
int ht_gf_index(unsigned k, unsigned s, unsigned b, uint32_t* out) {
  if (!out || k < 1 || k > 28 || s >= k || b >= (1u << (k - 1))) return -1;
  out[0] = gf_index_a(k, s, b);
  out[1] = gf_index_b(k, s, b);
  out[2] = gf_twiddle_exp(k, s, b);
  return 0;
}
// root^e of the domain of 2^k points (the inverse root's for inverse != 0) through the two-level tables, as canonical 32-byte integers
int ht_gf_twiddle_words(int field, unsigned k, int inverse, const uint32_t* exps, size_t count, uint8_t* out) {
  if (!exps || !out || k > 20) return -1;
  return field == 0 ? t_gf_twiddles<Bls12_377_Fr29>(k, inverse, exps, count, out) : field == 1 ? t_gf_twiddles<Bls12_381_Fr29>(k, inverse, exps, count, out) : -1;
}
// one call of mi355_msm_fft_points on the host: window size w, flags bit 1 Projective images, offset an arkworks image or NULL
int ht_gf_transform(int curve, unsigned k, unsigned kind, const uint8_t* offset, const uint8_t* in, size_t stride, unsigned in_len, int w, unsigned flags,
                    uint8_t* out, size_t out_stride) {
  if (k > 12 || kind > 3 || (flags & ~kGfProjective) || !out || (in_len && !in) || in_len > (1u << k) || w < 1 || w > (int)PM_MAX_WINDOW || stride % 4 ||
      out_stride % 4 || (offset && !(kind & 2)))
    return -1;
  DISPATCH_C(curve, t_gf_transform, k, kind, offset, in, stride, in_len, (uint32_t)w, flags, out, out_stride)
}
// the refusals of a call from plain values (gf_check_call): returns 0 and an empty message for a call that would run, else -1
int ht_gf_check(int ctx_curve, int ctx_sharded, int ctx_device, int dom_curve, int dom_device, unsigned k, const void* out, size_t out_stride, const void* in,
                size_t in_len, size_t stride, unsigned kind, unsigned flags, int has_offset, int offset_is_zero, size_t work_limit, char* msg, size_t msg_len) {
  if (!msg || msg_len < 1) return -2;
  GfCall c{ctx_curve, ctx_sharded, ctx_device, dom_curve, dom_device, k, out, out_stride, in, in_len, stride, kind, flags, has_offset, offset_is_zero, work_limit};
  char buf[256];
  const char* m = gf_check_call(c, buf, sizeof buf);
  snprintf(msg, msg_len, "%s", m ? m : "");
  return m ? -1 : 0;
}
}

// ---- hash-to-curve (h2c.hpp) with the limb-bound checker armed --------------------------------------------------------------------
// The SAME MSM_HD functions the kernels of kernels_h2c.hip wrap: SHA-256, expand_message_xmd with the reduction, sqrt_ratio, the
// simplified SWU map, the isogeny, the pair sum and the cofactor clearing; output by fb_normalize_run.  group 0: G1, 1: G2.
#include "h2c.hpp"

struct H2cHostDst {
  uint8_t prime[256];
  H2cDst d;
  H2cHostDst(const uint8_t* dst, size_t len) {
    h2c_make_dst(prime, d.prime_len, d.z_pad, dst, len);
    d.prime = prime;
  }
};

template <class E>
static void t_h2c_field(const H2cDst& d, const uint8_t* data, const uint64_t* off, size_t n, uint32_t count, uint8_t* out) {
  const typename E::Md md;
  const uint32_t elems = count * (E::WORDS / 12);
  for (size_t i = 0; i < n; i++)
    h2c_expand<typename E::Fld>((uint32_t*)out + i * elems * 12, data + off[i], (uint32_t)(off[i + 1] - off[i]), elems, d, md);
}

// flags: bit 2 pairs (n even, n / 2 outputs, cleared), bit 3 Projective images; bit 0 set with bit 2 clear: n outputs, each cleared
template <class E>
static void t_h2c_map(const uint8_t* u, size_t n, unsigned flags, uint8_t* out, size_t stride) {
  using El = typename E::T;
  const typename E::Md md;
  std::vector<XyzzDevT<El>> pts(n);
  std::vector<uint8_t> ws(h2c_map_ws_bytes<E>() + h2c_clear_ws_bytes<E>() + 16);
  for (size_t i = 0; i < n; i++) {
    uint32_t w[E::WORDS];
    memcpy(w, u + i * 4 * E::WORDS, 4 * E::WORDS);
    El x;
    E::from_abi(x, w, md);
    h2c_map_at<E>(&pts[i].p, x, ws.data(), 1, md);
  }
  std::vector<XyzzDevT<El>> res;
  if (flags & 4) {
    res.resize(n / 2);
    for (size_t j = 0; j < n / 2; j++) h2c_clear_at<E>(&res[j].p, &pts[2 * j].p, &pts[2 * j + 1].p, ws.data(), 1, md);
  } else {
    res = pts;
    if (flags & 1)
      for (size_t j = 0; j < n; j++) h2c_clear_at<E>(&res[j].p, &pts[j].p, nullptr, ws.data(), 1, md);
  }
  pm_host_output<E>(res, (flags & 8) ? 2u : 0u, out, stride, md);
}

// mode 0: h2c_clear; mode 1: plain double-and-add by the little-endian integer k of nbytes bytes, on Affine images of any curve points
template <class E>
static void t_h2c_clear(int mode, const uint8_t* points, size_t stride, size_t n, const uint8_t* k, size_t nbytes, uint8_t* out, size_t out_stride) {
  using El = typename E::T;
  const typename E::Md md;
  std::vector<XyzzDevT<El>> res(n);
  std::vector<uint8_t> ws(h2c_clear_ws_bytes<E>() + 16);
  for (size_t i = 0; i < n; i++) {
    const uint8_t* img = points + i * stride;
    uint32_t rec[2 * E::WORDS];
    memcpy(rec, img, 8 * E::WORDS);
    XyzzT<El> q;
    if (img[8 * E::WORDS]) {
      xyzz_set_inf<E>(q);
    } else {
      AffineT<El> a;
      pm_load_point<E>(a, rec, md);
      xyzz_from_affine<E>(q, a, false);
    }
    if (mode == 0) {
      h2c_clear_at<E>(&res[i].p, &q, nullptr, ws.data(), 1, md);
    } else {
      XyzzT<El> acc;
      xyzz_set_inf<E>(acc);
      for (int bit = (int)(8 * nbytes) - 1; bit >= 0; bit--) {
        xyzz_dbl<E>(acc, md);
        if ((k[bit >> 3] >> (bit & 7)) & 1) xyzz_add<E>(acc, q, md);
      }
      res[i].p = acc;
    }
  }
  pm_host_output<E>(res, 0, out, out_stride, md);
}

template <class E>
static int t_h2c_sqrt_ratio(const uint8_t* u, const uint8_t* v, uint8_t* y) {
  const typename E::Md md;
  uint32_t w[E::WORDS];
  typename E::T a, b, r;
  memcpy(w, u, 4 * E::WORDS);
  E::from_abi(a, w, md);
  memcpy(w, v, 4 * E::WORDS);
  E::from_abi(b, w, md);
  bool sq;
  if constexpr (E::WORDS == 12) {
    sq = h2c_sqrt_ratio<E>(r, a, b, md);
  } else {
    Fe2 ws[H2C_MAP_SLOTS];
    const H2cMem s{ws, 1};
    s.put(HS_GXN, a);
    s.put(HS_TV6, b);
    sq = h2c_sqrt_ratio_slots<E>(s, md);
    r = s.get(HS_Y);
  }
  E::to_abi(w, r, md);
  memcpy(y, w, 4 * E::WORDS);
  return sq ? 1 : 0;
}

template <class E>
static void t_h2c_iso(const uint8_t* xn, const uint8_t* xd, const uint8_t* y, uint8_t* out, size_t stride) {
  const typename E::Md md;
  uint32_t w[E::WORDS];
  typename E::T a, b, c;
  memcpy(w, xn, 4 * E::WORDS);
  E::from_abi(a, w, md);
  memcpy(w, xd, 4 * E::WORDS);
  E::from_abi(b, w, md);
  memcpy(w, y, 4 * E::WORDS);
  E::from_abi(c, w, md);
  std::vector<XyzzDevT<typename E::T>> res(1);
  if constexpr (E::WORDS == 12) {
    h2c_iso<E>(res[0].p, a, b, c, md);
  } else {
    Fe2 ws[H2C_MAP_SLOTS];
    const H2cMem s{ws, 1};
    s.put(HS_XN, a);
    s.put(HS_XD, b);
    s.put(HS_Y, c);
    h2c_iso_slots<E>(&res[0].p, s, md);
  }
  pm_host_output<E>(res, 0, out, stride, md);
}

#define H2C_GROUP(fn, ...) (group == 0 ? fn<Bls12_381_G1::E>(__VA_ARGS__) : fn<Bls12_381_G2::E>(__VA_ARGS__))
extern "C" {
int ht_h2c_sha256(const uint8_t* data, size_t len, uint8_t* out) {
  if ((len && !data) || !out || len >= (1u << 28)) return -1;
  uint32_t h[8];
  h2c_sha256(h, data, (uint32_t)len);
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)(h[i >> 2] >> (24 - 8 * (i & 3)));
  return 0;
}
// DST_prime (at most 256 bytes) and the state after 64 zero bytes; returns the length of DST_prime
int ht_h2c_dst(const uint8_t* dst, size_t len, uint8_t* prime, uint32_t* z_pad) {
  if (!dst || !len || !prime || !z_pad) return -1;
  H2cHostDst d(dst, len);
  memcpy(prime, d.prime, d.d.prime_len);
  memcpy(z_pad, d.d.z_pad, 32);
  return (int)d.d.prime_len;
}
// the reduction of hash_to_field on a raw 64-byte big-endian string: m = 1 or 2 strings in, m images of 48 bytes out
int ht_h2c_reduce(const uint8_t* in, size_t count, uint8_t* out) {
  if (!in || !out) return -1;
  const Modulus<Bls12_381_Fq> md;
  for (size_t j = 0; j < count; j++) {
    uint32_t hi[8], lo[8], w[12];
    for (int k = 0; k < 8; k++) {
      const uint8_t* a = in + 64 * j + 4 * k;
      hi[k] = ((uint32_t)a[0] << 24) | ((uint32_t)a[1] << 16) | ((uint32_t)a[2] << 8) | a[3];
      lo[k] = ((uint32_t)a[32] << 24) | ((uint32_t)a[33] << 16) | ((uint32_t)a[34] << 8) | a[35];
    }
    h2c_reduce<Bls12_381_Fq>(w, hi, lo, md);
    memcpy(out + 48 * j, w, 48);
  }
  return 0;
}
int ht_h2c_check_offsets(const uint64_t* off, size_t n, size_t data_bytes, char* msg, size_t msg_len) {
  if (!msg || msg_len < 1) return -2;
  const char* m = h2c_check_offsets(off, n, data_bytes);
  snprintf(msg, msg_len, "%s", m ? m : "");
  return m ? -1 : 0;
}
int ht_h2c_field(int group, const uint8_t* dst, size_t dst_len, const uint8_t* data, size_t data_bytes, const uint64_t* off, size_t n, unsigned count,
                 uint8_t* out) {
  if (group < 0 || group > 1 || !dst || !dst_len || count < 1 || count > 2 || (n && !out) || h2c_check_offsets(off, n, data_bytes)) return -1;
  H2cHostDst d(dst, dst_len);
  H2C_GROUP(t_h2c_field, d.d, data, off, n, count, out);
  return 0;
}
int ht_h2c_map(int group, const uint8_t* u, size_t n, unsigned flags, uint8_t* out, size_t stride) {
  if (group < 0 || group > 1 || (n && (!u || !out)) || (flags & ~13u) || ((flags & 4) && (n & 1)) || stride % 4) return -1;
  H2C_GROUP(t_h2c_map, u, n, flags, out, stride);
  return 0;
}
int ht_h2c_clear(int group, int mode, const uint8_t* points, size_t stride, size_t n, const uint8_t* k, size_t nbytes, uint8_t* out, size_t out_stride) {
  if (group < 0 || group > 1 || (n && (!points || !out)) || (mode && !k) || mode < 0 || mode > 1) return -1;
  H2C_GROUP(t_h2c_clear, mode, points, stride, n, k, nbytes, out, out_stride);
  return 0;
}
int ht_h2c_sqrt_ratio(int group, const uint8_t* u, const uint8_t* v, uint8_t* y) {
  if (group < 0 || group > 1 || !u || !v || !y) return -1;
  return H2C_GROUP(t_h2c_sqrt_ratio, u, v, y);
}
int ht_h2c_iso(int group, const uint8_t* xn, const uint8_t* xd, const uint8_t* y, uint8_t* out, size_t stride) {
  if (group < 0 || group > 1 || !xn || !xd || !y || !out) return -1;
  H2C_GROUP(t_h2c_iso, xn, xd, y, out, stride);
  return 0;
}
}

// ---- lookup tables and the logUp sum (lookup.hpp): the build, the probe, the counters as elements, the u32 scan, the expansion and the
// rows of the logUp sum lane by lane in order -- the atomics are plain sequential operations here -- and the chains the engine runs ------
#include "lookup.hpp"

struct HostLookupRun {
  // a tile of the u32 scan in order: what the block's lanes do through LDS
  void scan_up(const LookupScan& p) {
    const uint64_t T = (uint64_t)1 << LOOKUP_SCAN_TILE_LOG;
    for (uint64_t tile = 0; tile * T < p.n; tile++) {
      uint32_t acc = 0;
      for (uint64_t i = 0; i < T; i++) acc += lookup_scan_elem(p, tile * T + i);
      p.totals[tile] = acc;
    }
  }
  void scan_down(const LookupScan& p) {
    const uint64_t T = (uint64_t)1 << LOOKUP_SCAN_TILE_LOG;
    for (uint64_t tile = 0; tile * T < p.n; tile++) {
      uint32_t acc = p.carry ? p.carry[tile] : 0u;
      for (uint64_t i = 0; i < T && tile * T + i < p.n; i++) {
        const uint32_t e = lookup_scan_elem(p, tile * T + i);
        p.dst[tile * T + i] = acc;
        acc += e;
      }
    }
  }
};

// create + count + sorted: every output may be NULL; info = {slots, distinct, max_probe}
template <class FR>
static int t_lookup(unsigned flags, const uint8_t* table, uint64_t n_t, const uint8_t* values, uint64_t n_f, uint8_t* mult_out, uint32_t* index_out,
                    uint64_t* stats, uint8_t* s_out, uint64_t* info) {
  std::vector<uint32_t> raw(n_t * 8), keys(n_t * 8), vals(n_f * 8), count(n_t, 0u), index(n_f);
  memcpy(raw.data(), table, n_t * 32);
  if (n_f) memcpy(vals.data(), values, n_f * 32);
  uint32_t nslots = 2;
  while (nslots < 2 * n_t) nslots <<= 1;
  std::vector<uint32_t> slots(nslots, LOOKUP_EMPTY);
  LookupHead head{};
  head.first = ~0ull;
  const LookupCanon cp{raw.data(), keys.data(), n_t};
  for (uint64_t i = 0; i < n_t; i++) lookup_canon_elem<FR>(cp, i);
  const LookupTab tab{keys.data(), slots.data(), (uint32_t)n_t, nslots - 1};
  const LookupBuild bp{tab, &head};
  for (uint32_t i = 0; i < n_t; i++) {
    uint32_t steps;
    if (lookup_insert(bp, i, steps)) head.distinct++;
    lookup_note_walk(bp, steps);
  }
  if (head.err) return -2;
  const LookupProbe pp{tab, vals.data(), n_f, n_f ? index.data() : nullptr, count.data(), &head, 1u};
  for (uint64_t j = 0; j < n_f; j++) lookup_credit(pp, lookup_find<FR>(pp, j), j, 1u);
  if (head.err) return -2;
  if (info) {
    info[0] = nslots;
    info[1] = head.distinct;
    info[2] = head.max_probe;
  }
  if (stats) {
    stats[0] = head.missing;
    stats[1] = head.missing ? head.first : n_f;
  }
  if (index_out && n_f) memcpy(index_out, index.data(), n_f * 4);
  if (mult_out) {
    std::vector<uint32_t> dst(n_t * 8);
    LookupMult mp{count.data(), dst.data(), (uint32_t)n_t, (flags & kLookupNormal) ? 1u : 0u, Fr{}};
    lookup_image_const<FR>(mp.image);
    for (uint32_t i = 0; i < n_t; i++) lookup_mult_elem<FR>(mp, i);
    memcpy(mult_out, dst.data(), n_t * 32);
  }
  if (s_out && !head.missing) {
    std::vector<uint32_t> off(n_t), levels(lookup_scan_work_words(n_t)), dst((n_t + n_f) * 8);
    HostLookupRun run;
    lookup_scan_chain(run, off.data(), count.data(), n_t, levels.data());
    const LookupExpand ep{keys.data(), off.data(), dst.data(), (uint32_t)n_t, n_t + n_f};
    for (uint64_t g = 0; g < n_t + n_f; g++) lookup_expand_elem(ep, g);
    memcpy(s_out, dst.data(), (n_t + n_f) * 32);
  }
  return 0;
}

template <class FR>
static int t_logup_sum(uint32_t tile_log, unsigned flags, const uint8_t* table, const uint8_t* mult, const uint8_t* values, uint32_t m, uint64_t stride,
                       uint64_t n, const uint8_t* beta, uint8_t* out, uint8_t* total32, uint8_t* helpers) {
  const bool normal = (flags & kLookupNormal) != 0;
  if (n == 0) {
    if (total32) memset(total32, 0, 32);
    return 0;
  }
  const uint64_t span = (m - 1) * stride + n, hn = (uint64_t)(m + 1) * n;
  std::vector<uint32_t> v(span * 8), t(n * 8), mu(n * 8), h(hn * 8), term(n * 8), dst(n * 8);
  memcpy(v.data(), values, span * 32);
  memcpy(t.data(), table, n * 32);
  memcpy(mu.data(), mult, n * 32);
  LogupRows p{};
  p.values = v.data();
  p.table = t.data();
  p.mult = mu.data();
  p.helpers = h.data();
  p.term = term.data();
  p.n = n;
  p.stride = stride;
  p.m = m;
  p.normal = normal ? 1u : 0u;
  poly_scalar<FR>(p.beta, beta, normal);
  for (uint64_t j = 0; j < n; j++) logup_den_row<FR>(p, j);
  std::vector<Fr> iwork(poly_work_elems(hn, tile_log)), work(scan_work_elems(n, tile_log));
  Fr one;
  fr_set<FR>(one, FR::ONE);
  HostPolyRun<FR> inv;
  poly_chain_inverse<FR>(inv, h.data(), h.data(), hn, normal, tile_log, one, iwork.data());
  for (uint64_t j = 0; j < n; j++) logup_term_row<FR>(p, j);
  HostScanRun<FR> run;
  const Fr* res = scan_chain<FR, kScanSum>(run, dst.data(), term.data(), nullptr, n, normal, false, tile_log, work.data());
  if (total32) poly_scalar_out<FR>(total32, *res, normal);
  memcpy(out, dst.data(), n * 32);
  if (helpers) memcpy(helpers, h.data(), hn * 32);
  return 0;
}

extern "C" {
// mi355_msm_lookup_create + _count + _sorted on the host: flags bit 0, plain integers; mult_out (n_t elements), index_out (n_f u32), stats
// (2), s_out (n_t + n_f elements; untouched when a value is missing) and info (slots, distinct, max_probe) may each be NULL
int ht_lookup(int field, unsigned flags, const uint8_t* table, uint64_t n_t, const uint8_t* values, uint64_t n_f, uint8_t* mult_out, uint32_t* index_out,
              uint64_t* stats, uint8_t* s_out, uint64_t* info) {
  if ((flags & ~kLookupNormal) || n_t < 1 || n_t > ((uint64_t)1 << 22) || n_f > ((uint64_t)1 << 22) || !table || (n_f && !values)) return -1;
  return POLY_FIELD(t_lookup, flags, table, n_t, values, n_f, mult_out, index_out, stats, s_out, info);
}
// the hash of one canonical key, for the tests of its mixing
unsigned ht_lookup_hash(const uint8_t* key32) {
  uint32_t w[8];
  memcpy(w, key32, 32);
  return lookup_hash(w);
}
// mi355_msm_domain_logup_sum on the host; total32 and helpers ((m + 1) n elements) may be NULL
int ht_logup_sum(int field, unsigned tile_log, unsigned flags, const uint8_t* table, const uint8_t* mult, const uint8_t* values, unsigned m, uint64_t stride,
                 uint64_t n, const uint8_t* beta, uint8_t* out, uint8_t* total32, uint8_t* helpers) {
  if (tile_log < POLY_TILE_LOG_MIN || tile_log > POLY_TILE_LOG_MAX || (flags & ~kLookupNormal) || m < 1 || m > LOGUP_MAX_COLUMNS || stride < n ||
      n > ((uint64_t)1 << 20) || stride > ((uint64_t)1 << 22) || !beta || (n && (!table || !mult || !values || !out)))
    return -1;
  return POLY_FIELD(t_logup_sum, tile_log, flags, table, mult, values, m, stride, n, beta, out, total32, helpers);
}
}

// ---- compiled expressions (expr.hpp): the compiler, and the interpreter row by row with one lane's slots in a plain array -----------
#include "expr.hpp"

template <class FR>
static int t_expr(unsigned flags, const uint32_t* nodes, uint64_t n_nodes, const uint8_t* consts, uint64_t n_consts, uint64_t n_chal, uint64_t n_cols,
                  const uint8_t* const* cols, const uint64_t* lens, uint64_t len, uint64_t rot_step, const uint8_t* challenges, uint8_t* out, uint64_t* info,
                  char* msg, uint64_t msg_len) {
  const bool normal = (flags & kExprNormal) != 0;
  ExprProgram pr;
  if (!expr_check_dag(nodes, n_nodes, n_consts, n_chal, n_cols, msg, msg_len)) return -1;
  const bool ok = expr_compile(pr, nodes, n_nodes, n_consts, n_chal, n_cols, expr_store_limit<FR>(), msg, msg_len);
  if (info) {
    info[0] = pr.n_nodes;
    info[1] = pr.ninstr();
    info[2] = pr.slots;
    info[3] = pr.products;
    info[4] = pr.reduces;
    info[5] = expr_lds_bytes(pr.slots);
    info[6] = pr.used_cols;
    info[7] = pr.rot0_only;
  }
  if (!ok) return -1;
  if (!out || len == 0) return 0;
  for (uint64_t j = 0; j < n_cols; j++)
    if (lens[j] == 0 || len % lens[j]) return -3;
  std::vector<uint32_t> cw(n_consts * 8 + 1), hw(n_chal * 8 + 1), dst(len * 8), slots((size_t)pr.slots * 8 + 1);
  std::vector<std::vector<uint32_t>> colw(n_cols);
  auto words = [&](uint32_t* w8, const uint8_t* b32) {
    Fr x;
    uint32_t w[8];
    poly_scalar<FR>(x, b32, normal);
    fr_pack(w, x);
    memcpy(w8, w, 32);
  };
  for (uint64_t k = 0; k < n_consts; k++) words(cw.data() + k * 8, consts + k * 32);
  for (uint64_t k = 0; k < n_chal; k++) words(hw.data() + k * 8, challenges + k * 32);
  for (uint64_t j = 0; j < n_cols; j++) {
    colw[j].resize(lens[j] * 8);
    memcpy(colw[j].data(), cols[j], lens[j] * 32);
  }
  std::vector<ExprColRef> refs(pr.refs.size() + 1);
  for (size_t k = 0; k < pr.refs.size(); k++)
    refs[k] = ExprColRef{colw[pr.refs[k].first].data(), (uint32_t)lens[pr.refs[k].first], expr_shift(pr.refs[k].second, rot_step, len)};
  ExprRun p{};
  p.prog = pr.code.data();
  p.refs = refs.data();
  p.consts = cw.data();
  p.chals = hw.data();
  p.out = dst.data();
  p.ninstr = pr.ninstr();
  p.len = (uint32_t)len;
  p.normal = normal ? 1u : 0u;
  const ExprSlots<1> st{slots.data()};
  for (uint64_t i = 0; i < len; i++) expr_row<FR>(st, p, (uint32_t)i);
  memcpy(out, dst.data(), len * 32);
  return 0;
}

extern "C" {
// mi355_msm_expr_create + _run on the host: flags bit 0, plain integers (constants, challenges, columns and output alike).  info (8: nodes,
// instructions, slots, products, reduces, lds_bytes, the columns read, those read at rotation 0 only) may be NULL; out NULL or len 0: the
// compiler alone.  -1 with msg set: what create refuses.
int ht_expr(int field, unsigned flags, const uint32_t* nodes, uint64_t n_nodes, const uint8_t* consts, uint64_t n_consts, uint64_t n_chal, uint64_t n_cols,
            const uint8_t* const* cols, const uint64_t* lens, uint64_t len, uint64_t rot_step, const uint8_t* challenges, uint8_t* out, uint64_t* info,
            char* msg, uint64_t msg_len) {
  if ((flags & ~kExprNormal) || !nodes || !msg || msg_len < 64 || len > ((uint64_t)1 << 22) || (n_consts && !consts)) return -2;
  if (out && len && ((n_cols && (!cols || !lens)) || (n_chal && !challenges))) return -2;
  msg[0] = 0;
  return POLY_FIELD(t_expr, flags, nodes, n_nodes, consts, n_consts, n_chal, n_cols, cols, lens, len, rot_step, challenges, out, info, msg, msg_len);
}
unsigned ht_expr_max_slots(void) { return EXPR_MAX_SLOTS; }
}

// ---- segmented MSM (seg_msm.hpp): the digits, one call walked serially through the kernels' per-element steps, the launch plan ----
#include "seg_msm.hpp"

template <class C>
static int t_sm_segments(const uint8_t* points, size_t stride, const uint8_t* scalars, const uint64_t* offsets, size_t nseg, uint64_t shared_len, uint32_t c,
                         uint32_t tile, unsigned flags, uint8_t* out, size_t out_stride) {
  using E = typename C::E;
  using El = typename E::T;
  typename E::Md md;
  std::vector<XyzzDevT<El>> res(nseg);
  std::vector<uint32_t> sc;
  for (size_t s = 0; s < nseg; s++) {
    uint64_t p0, s0, len;
    sm_segment_span(p0, s0, len, offsets, s, shared_len, 0);   // (the kernel's own statement of where a segment lies)
    if (len == 0) {
      xyzz_set_inf<E>(res[s].p);
      continue;
    }
    sc.resize(8 * len);
    memcpy(sc.data(), scalars + 32 * s0, 32 * len);
    sm_serial_segment<E>(res[s].p, points + p0 * stride, stride, sc.data(), len, c ? c : sm_window_for(len), tile, (flags & 1) != 0, md);
  }
  pm_host_output<E>(res, (flags & 8) ? 2u : 0u, out, out_stride, md);
  return 0;
}

extern "C" {
// the signed digits of one 32-byte scalar for window size c, from the register form and from the memory form: sm_digits(c) values each
int ht_sm_digits(const uint8_t* scalar, int c, int32_t* out, int32_t* out_mem) {
  if (!scalar || !out || !out_mem || c < 1 || c > (int)SM_MAX_WINDOW) return -1;
  uint32_t s[8];
  memcpy(s, scalar, 32);
  const uint32_t nd = sm_digits((uint32_t)c);
  for (uint32_t j = 0; j < nd; j++) {
    out[j] = sm_digit(s, j, (uint32_t)c);
    out_mem[j] = sm_digit_mem(s, j, (uint32_t)c);
  }
  return (int)nd;
}
// mi355_msm_segments on the host, lane by lane: flags bit 0 Fr Montgomery scalars, bit 2 the shared form (offsets NULL, shared_len
// points), bit 3 Projective images; c 0 = by length
int ht_sm_segments(int curve, const uint8_t* points, size_t stride, const uint8_t* scalars, const uint64_t* offsets, size_t nseg, uint64_t shared_len, int c,
                   int tile, unsigned flags, uint8_t* out, size_t out_stride) {
  if ((flags & ~13u) || c < 0 || c > (int)SM_MAX_WINDOW || tile < (int)SM_MIN_TILE || (tile & (tile - 1)) || out_stride % 4 || (nseg && !out)) return -1;
  if (((flags & 4) != 0) != (offsets == nullptr)) return -1;
  DISPATCH_C(curve, t_sm_segments, points, stride, scalars, offsets, nseg, shared_len, (uint32_t)c, (uint32_t)tile, flags, out, out_stride)
}
// the launch plan, flattened: per class 11 values {chunk, s0, s1, c, nwin, tile, nseg, position of its ids in `ids`, wsum_at, the chunk's
// work_bytes, the chunk's wsum_records}; returns the number of classes, -1 for bad arguments or too small arrays, -2 when a segment
// alone exceeds the limit.  summary: {chunks, max_segs, max_wsum_records}
long ht_sm_plan(const uint64_t* offsets, size_t nseg, uint64_t shared_len, int force_c, int tile_opt, size_t max_segs, size_t work_limit, size_t xyzz_bytes,
                size_t el_bytes, uint64_t* classes, size_t max_classes, uint32_t* ids, size_t max_ids, uint64_t* chunk_bounds, size_t max_chunks,
                uint64_t* summary) {
  if (force_c < 0 || force_c > (int)SM_MAX_WINDOW || !classes || !ids || !summary || !chunk_bounds) return -1;
  SmPlan plan;
  sm_plan(plan, offsets, nseg, shared_len, (uint32_t)force_c, (uint32_t)tile_opt, max_segs, work_limit, xyzz_bytes, el_bytes);
  if (!plan.fits) return -2;
  size_t nc = 0, ni = 0;
  if (plan.chunks.size() > max_chunks) return -1;
  for (size_t k = 0; k < plan.chunks.size(); k++) {
    const SmChunk& ch = plan.chunks[k];
    chunk_bounds[3 * k] = ch.s0;
    chunk_bounds[3 * k + 1] = ch.s1;
    chunk_bounds[3 * k + 2] = ch.work_bytes;
    if (ni + ch.ids.size() > max_ids) return -1;
    for (const SmClass& cl : ch.classes) {
      if (nc >= max_classes) return -1;
      const uint64_t row[11] = {k, ch.s0, ch.s1, cl.c, cl.nwin, cl.tile, cl.nseg, ni + cl.ids_at, cl.wsum_at, ch.work_bytes, ch.wsum_records};
      memcpy(classes + 11 * nc++, row, sizeof row);
    }
    if (!ch.ids.empty()) memcpy(ids + ni, ch.ids.data(), 4 * ch.ids.size());
    ni += ch.ids.size();
  }
  summary[0] = plan.chunks.size();
  summary[1] = plan.max_segs;
  summary[2] = plan.max_wsum_records;
  return (long)nc;
}
// the geometry of one class's launch: {slices per block, lanes per block, LDS words, the tile sm_tile_for picks for maxlen}
int ht_sm_geometry(int c, int tile_opt, uint64_t maxlen, int xyzz_words, uint32_t* out) {
  if (c < 1 || c > (int)SM_MAX_WINDOW || !out) return -1;
  out[0] = sm_slices((uint32_t)c);
  out[1] = sm_block_threads((uint32_t)c);
  out[3] = sm_tile_for((uint32_t)c, (uint32_t)tile_opt, maxlen);
  out[2] = sm_lds_words((uint32_t)c, out[3], (uint32_t)xyzz_words);
  return 0;
}
int ht_sm_window_for(uint64_t len) { return (int)sm_window_for(len); }
}

// ---- Entries32 (msm_types.hpp): the sorted entry stream written and read back with the format's own helpers ----------------------
// The writer restates what the last grouping pass does (partition.hpp): a block sees one segment -- the keys [seg_keys[s],
// seg_keys[s + 1]) -- and gives the first entry of every non-empty bin its distance to the previous non-empty bin of the SAME segment,
// an escape for the segment's first bin and for gaps above 30 (every run start when seg_subjobs[s] != 0: a segment cut into
// sub-jobs), and the key of every lane start in run_keys.  The reader is the accumulation's walk, lane by lane.
#include "msm_types.hpp"

extern "C" {
// keys[n] non-decreasing, values[n] = base index | sign << 31; run_keys[n] is written only where the format needs it (the caller
// pre-fills it to see where).  Returns the number of escapes, -1 for bad arguments (unsorted keys, a key below the first segment, K = 0).
long ht_e32_encode(const uint32_t* keys, const uint32_t* values, size_t n, uint32_t K, const uint32_t* seg_keys, const uint8_t* seg_subjobs, size_t nseg,
                   uint32_t* words, uint32_t* run_keys) {
  if (K == 0 || nseg == 0 || !seg_keys || (n && (!keys || !values || !words || !run_keys))) return -1;
  long escapes = 0;
  size_t seg = 0, prev_seg = (size_t)-1;
  for (size_t i = 0; i < n; i++) {
    if (i && keys[i] < keys[i - 1]) return -1;
    if (keys[i] < seg_keys[0]) return -1;
    while (seg + 1 < nseg && seg_keys[seg + 1] <= keys[i]) seg++;
    uint32_t step = 0;
    if (i == 0 || keys[i] != keys[i - 1]) {
      const bool first_of_segment = seg != prev_seg;
      step = e32_step_of_gap(first_of_segment ? 0u : keys[i] - keys[i - 1], first_of_segment || (seg_subjobs && seg_subjobs[seg]));
      prev_seg = seg;
    }
    words[i] = e32_pack(values[i], step);
    if (step == E32_ESCAPE) {
      run_keys[i] = keys[i];
      escapes++;
    }
  }
  // the lane starts, run by run: the multiples of K inside [start of the run, its end)
  for (size_t i = 0; i < n;) {
    size_t j = i;
    while (j < n && keys[j] == keys[i]) j++;
    for (uint64_t q = e32_first_lane_start((uint32_t)i, K); q < j; q += K) run_keys[q] = keys[i];
    i = j;
  }
  return escapes;
}
// the walk of lane t over [t K, (t + 1) K): keys_out[n]; continued[t] = 1 when the lane's first entry continues the bucket of the lane before
int ht_e32_decode(const uint32_t* words, const uint32_t* run_keys, size_t n, uint32_t K, uint32_t* keys_out, uint32_t* values_out, uint8_t* continued) {
  if (K == 0) return -1;
  for (size_t beg = 0, t = 0; beg < n; beg += K, t++) {
    const size_t end = beg + K < n ? beg + K : n;
    uint32_t cur = run_keys[beg];
    if (continued) continued[t] = e32_step(words[beg]) == 0;
    for (size_t i = beg; i < end; i++) {
      if (i > beg) cur = e32_next_key(cur, words[i], run_keys, (uint32_t)i);
      keys_out[i] = cur;
      values_out[i] = (words[i] & 0x80000000u) | e32_index(words[i]);
    }
  }
  return 0;
}
uint32_t ht_e32_run_keys_offset(uint64_t capacity) { return e32_run_keys_offset(capacity); }
int ht_e32_applies(uint64_t idx0, uint64_t n, uint32_t table_levels) { return e32_applies(idx0, n, table_levels) ? 1 : 0; }
}
