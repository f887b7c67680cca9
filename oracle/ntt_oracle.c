/* ntt_oracle.c -- a plain CPU NTT over the scalar fields of BLS12-377 and BLS12-381.  TEST INFRASTRUCTURE ONLY (part of
 * liboracle.so, see msm_oracle.c for who may load it).
 *
 * It is the at-size checker of the radix-2 domains (csrc/fr.hpp, ntt.hpp, msm_ntt.hpp) and shares nothing with them: no header, no
 * table, no constant file.  What it takes as given are four literals per field -- the modulus, the multiplicative generator and
 * the 2-adicity, ARKC bls12_377/src/fields/fr.rs:24-25 and :7, bls12_381/src/fields/fr.rs:4-5 (`#[modulus = ".."]`,
 * `#[generator = ".."]`; s = 47 and 32) -- and everything else is derived at run time: -r^-1 mod 2^64 by Newton steps, R = 2^256
 * and R^2 by doubling, the root of unity of a domain as generator^((r - 1) >> k) (ARK ff/src/fields/mod.rs get_root_of_unity gives
 * the same element, there by squaring the two-adic root), inverses by Fermat.
 *
 * The arithmetic is the opposite of the kernels' wherever a choice exists: four saturated 64-bit limbs and CIOS with R = 2^256
 * (ARK ff/src/fields/models/fp/montgomery_backend.rs, so an arkworks image is the internal form as it stands) against nine
 * 29-bit limbs with R = 2^261 and lazy reduction; canonical after every operation; iterative decimation in time, in place, behind an
 * explicit bit reversal against Stockham passes in natural order; one flat table of n / 2 twiddles built by a running product
 * against a two-level table built by per-entry powers; the offset powers by a running product as well.
 *
 * PARITY PIN: tests/test_ntt_oracle.py holds it byte-equal to the big-integer model of tests/ntt_cases.py at k <= 12 and to Horner
 * evaluations at 2^18.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef unsigned __int128 u128;

typedef struct {
  uint64_t l[4];
} fr_t;

typedef struct {
  fr_t p;       /* modulus r */
  uint64_t inv; /* -r^-1 mod 2^64 */
  fr_t one;     /* R mod r */
  fr_t r2;      /* R^2 mod r */
  uint64_t generator;
  unsigned two_adicity;
} frfield_t;

/* r = 8444461749428370424248824938781546531375899335154063827935233455917409239041 (ARKC bls12_377/src/fields/fr.rs:24) */
static const uint64_t R377[4] = {0x0a11800000000001ull, 0x59aa76fed0000001ull, 0x60b44d1e5c37b001ull, 0x12ab655e9a2ca556ull};
/* r = 52435875175126190479447740508185965837690552500527637822603658699938581184513 (ARKC bls12_381/src/fields/fr.rs:4) */
static const uint64_t R381[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};

enum { KIND_INVERSE = 1, KIND_COSET = 2, FLAG_NORMAL = 1, FLAG_NR = 2, FLAG_RN = 4, MAX_THREADS = 16 };

static int fr_geq(const fr_t* a, const fr_t* b) {
  for (int i = 3; i >= 0; i--)
    if (a->l[i] != b->l[i]) return a->l[i] > b->l[i];
  return 1;
}

static int fr_is_zero(const fr_t* a) { return (a->l[0] | a->l[1] | a->l[2] | a->l[3]) == 0; }

static uint64_t fr_add_raw(fr_t* r, const fr_t* a, const fr_t* b) {
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)a->l[i] + b->l[i];
    r->l[i] = (uint64_t)c;
    c >>= 64;
  }
  return (uint64_t)c;
}

static uint64_t fr_sub_raw(fr_t* r, const fr_t* a, const fr_t* b) {
  uint64_t borrow = 0;
  for (int i = 0; i < 4; i++) {
    u128 d = (u128)a->l[i] - b->l[i] - borrow;
    r->l[i] = (uint64_t)d;
    borrow = (uint64_t)(d >> 64) & 1;
  }
  return borrow;
}

/* canonical operands, canonical result */
static void fr_add(const frfield_t* f, fr_t* r, const fr_t* a, const fr_t* b) {
  fr_t t;
  uint64_t c = fr_add_raw(&t, a, b);
  if (c || fr_geq(&t, &f->p)) fr_sub_raw(&t, &t, &f->p);
  *r = t;
}

static void fr_sub(const frfield_t* f, fr_t* r, const fr_t* a, const fr_t* b) {
  fr_t t;
  if (fr_sub_raw(&t, a, b)) fr_add_raw(&t, &t, &f->p);
  *r = t;
}

/* a b / R mod r, CIOS: one row of the product, then one reduction step, per limb of b; the sum stays below 2r, one subtraction ends it */
static void fr_mul(const frfield_t* f, fr_t* r, const fr_t* a, const fr_t* b) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (u128)a->l[j] * b->l[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * f->inv;
    c = ((u128)m * f->p.l[0] + t[0]) >> 64;
    for (int j = 1; j < 4; j++) {
      c += (u128)m * f->p.l[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  fr_t o;
  memcpy(o.l, t, 32);
  if (t[4] || fr_geq(&o, &f->p)) fr_sub_raw(&o, &o, &f->p);
  *r = o;
}

/* base^e for a 256-bit exponent (little-endian limbs) */
static void fr_pow(const frfield_t* f, fr_t* r, const fr_t* base, const fr_t* e) {
  fr_t acc = f->one;
  for (int i = 255; i >= 0; i--) {
    fr_mul(f, &acc, &acc, &acc);
    if ((e->l[i >> 6] >> (i & 63)) & 1) fr_mul(f, &acc, &acc, base);
  }
  *r = acc;
}

/* a^(r - 2) */
static void fr_inverse(const frfield_t* f, fr_t* r, const fr_t* a) {
  fr_t e = f->p;
  e.l[0] -= 2; /* r is odd and its low limb is above 2 */
  fr_pow(f, r, a, &e);
}

/* a small integer in Montgomery form */
static void fr_from_u64(const frfield_t* f, fr_t* r, uint64_t v) {
  fr_t t = {{v, 0, 0, 0}};
  fr_mul(f, r, &t, &f->r2);
}

static void field_init(frfield_t* f, int field) {
  memcpy(f->p.l, field ? R381 : R377, 32);
  f->generator = field ? 7 : 22;      /* ARKC bls12_381/src/fields/fr.rs:5, bls12_377/src/fields/fr.rs:25 */
  f->two_adicity = field ? 32 : 47;   /* 2^32 | r - 1 (BLS12-381), 2^47 | r - 1 (BLS12-377, fr.rs:7) */
  uint64_t x = 1;                     /* Newton: x <- x (2 - p x) doubles the correct low bits */
  for (int i = 0; i < 6; i++) x *= 2 - f->p.l[0] * x;
  f->inv = (uint64_t)0 - x;
  fr_t a = {{1, 0, 0, 0}};            /* 2^256 and 2^512 mod r by doubling */
  for (int i = 0; i < 512; i++) {
    fr_add(f, &a, &a, &a);
    if (i == 255) f->one = a;
  }
  f->r2 = a;
}

/* 32 bytes, any 256-bit value, to the Montgomery form of the residue it stands for */
static void fr_load(const frfield_t* f, fr_t* r, const uint8_t* src, int normal) {
  fr_t x;
  for (int i = 0; i < 4; i++) {
    uint64_t w = 0;
    for (int b = 7; b >= 0; b--) w = (w << 8) | src[8 * i + b];
    x.l[i] = w;
  }
  while (fr_geq(&x, &f->p)) fr_sub_raw(&x, &x, &f->p); /* 2^256 / r < 14 */
  if (normal) fr_mul(f, &x, &x, &f->r2);
  *r = x;
}

static void fr_store(const frfield_t* f, uint8_t* dst, const fr_t* a, int normal) {
  fr_t x = *a;
  if (normal) {
    const fr_t plain_one = {{1, 0, 0, 0}};
    fr_mul(f, &x, &x, &plain_one);
  }
  for (int i = 0; i < 4; i++)
    for (int b = 0; b < 8; b++) dst[8 * i + b] = (uint8_t)(x.l[i] >> (8 * b));
}

static size_t bit_reverse(size_t x, unsigned bits) {
  size_t r = 0;
  for (unsigned b = 0; b < bits; b++) r |= ((x >> b) & 1) << (bits - 1 - b);
  return r;
}

static void permute_bit_reversed(fr_t* a, unsigned k) {
  const size_t n = (size_t)1 << k;
  for (size_t i = 0; i < n; i++) {
    const size_t j = bit_reverse(i, k);
    if (i < j) {
      fr_t t = a[i];
      a[i] = a[j];
      a[j] = t;
    }
  }
}

typedef struct {
  const frfield_t* f;
  fr_t* a;
  const fr_t* tw;
  size_t half, step, lo, hi;
} level_job_t;

/* butterflies lo .. hi of one level: butterfly b is pair (i, i + half) of block b / half, i = b mod half, twiddle w^(i n / (2 half)) */
static void* level_worker(void* arg) {
  const level_job_t* j = (const level_job_t*)arg;
  for (size_t b = j->lo; b < j->hi; b++) {
    const size_t blk = b / j->half, i = b % j->half;
    fr_t *u = &j->a[blk * 2 * j->half + i], *v = u + j->half, t;
    fr_mul(j->f, &t, v, &j->tw[i * j->step]);
    fr_sub(j->f, v, u, &t);
    fr_add(j->f, u, u, &t);
  }
  return NULL;
}

/* a[i] <- sum_j a[j] w^(i j), natural order in and out; tw[i] = w^i for i < n / 2 */
static void ntt_in_place(const frfield_t* f, fr_t* a, const fr_t* tw, unsigned k, int threads) {
  const size_t n = (size_t)1 << k, total = n / 2;
  permute_bit_reversed(a, k);
  if ((size_t)threads > total / 1024 + 1) threads = (int)(total / 1024 + 1);
  for (size_t half = 1; half < n; half *= 2) {
    pthread_t th[MAX_THREADS];
    level_job_t job[MAX_THREADS];
    int running[MAX_THREADS];
    for (int t = 0; t < threads; t++) {
      job[t] = (level_job_t){f, a, tw, half, n / (2 * half), total * (size_t)t / (size_t)threads, total * (size_t)(t + 1) / (size_t)threads};
      /* the caller's thread takes the last share, and any share no thread could be started for */
      running[t] = t + 1 < threads && pthread_create(&th[t], NULL, level_worker, &job[t]) == 0;
      if (!running[t]) level_worker(&job[t]);
    }
    for (int t = 0; t < threads; t++)
      if (running[t]) pthread_join(th[t], NULL);
  }
}

/* One call of mi355_msm_domain_transform on one vector.  field: 0 BLS12-377 Fr, 1 BLS12-381 Fr.  kind: 0 forward, 1 inverse, 2 coset
 * forward, 3 coset inverse.  flags: bit 0 normal-form elements (else arkworks images), bit 1 bit-reversed output (forward kinds),
 * bit 2 bit-reversed input (inverse kinds).  offset32: the coset offset in the form of the call, NULL for the generator.  in: in_len
 * elements of 32 bytes, any 256-bit value, zero-extended to 2^k.  out: 2^k canonical elements.  Returns 0, or -1 on bad arguments. */
int oracle_ntt(int field, unsigned k, unsigned kind, unsigned flags, const uint8_t* offset32, const uint8_t* in, size_t in_len, uint8_t* out, int threads) {
  if (field < 0 || field > 1 || kind > 3 || (flags & ~7u) || !out || (in_len && !in)) return -1;
  if ((flags & FLAG_NR) && (kind & KIND_INVERSE)) return -1;
  if ((flags & FLAG_RN) && !(kind & KIND_INVERSE)) return -1;
  if (offset32 && !(kind & KIND_COSET)) return -1;
  frfield_t f;
  field_init(&f, field);
  if (k > f.two_adicity || k > 40) return -1;
  const size_t n = (size_t)1 << k;
  if (in_len > n) return -1;
  const int normal = (flags & FLAG_NORMAL) != 0;
  if (threads < 1) threads = 1;
  if (threads > MAX_THREADS) threads = MAX_THREADS;

  /* omega = generator^((r - 1) >> k), inverted for the inverse kinds */
  fr_t gen, omega, e = f.p;
  fr_from_u64(&f, &gen, f.generator);
  e.l[0] -= 1;
  for (unsigned i = 0; i < k; i++)
    for (int q = 0; q < 4; q++) e.l[q] = (e.l[q] >> 1) | (q < 3 ? e.l[q + 1] << 63 : 0);
  fr_pow(&f, &omega, &gen, &e);
  if (kind & KIND_INVERSE) fr_inverse(&f, &omega, &omega);

  fr_t offset = gen;
  if (kind & KIND_COSET) {
    if (offset32) fr_load(&f, &offset, offset32, normal);
    if (fr_is_zero(&offset)) return -1;
    if (kind & KIND_INVERSE) fr_inverse(&f, &offset, &offset);
  }

  fr_t* a = (fr_t*)malloc(n * sizeof(fr_t));
  fr_t* tw = (fr_t*)malloc((n / 2 + 1) * sizeof(fr_t));
  if (!a || !tw) {
    free(a);
    free(tw);
    return -1;
  }
  tw[0] = f.one;
  for (size_t i = 1; i < n / 2; i++) fr_mul(&f, &tw[i], &tw[i - 1], &omega);

  /* the stored vector, zero-extended; a bit-reversed input is put in natural order first */
  for (size_t i = 0; i < n; i++) {
    if (i < in_len)
      fr_load(&f, &a[i], in + 32 * i, normal);
    else
      memset(&a[i], 0, sizeof(fr_t));
  }
  if (flags & FLAG_RN) permute_bit_reversed(a, k);
  if (kind == KIND_COSET) { /* coset forward: x[j] g^j */
    fr_t pw = f.one;
    for (size_t j = 0; j < n; j++) {
      fr_mul(&f, &a[j], &a[j], &pw);
      fr_mul(&f, &pw, &pw, &offset);
    }
  }
  ntt_in_place(&f, a, tw, k, threads);
  if (kind & KIND_INVERSE) { /* 1 / n, and g^-j over a coset */
    fr_t size, scale, pw;
    fr_from_u64(&f, &size, (uint64_t)n);
    fr_inverse(&f, &scale, &size);
    pw = scale;
    for (size_t j = 0; j < n; j++) {
      if (kind & KIND_COSET) {
        fr_mul(&f, &a[j], &a[j], &pw);
        fr_mul(&f, &pw, &pw, &offset);
      } else {
        fr_mul(&f, &a[j], &a[j], &scale);
      }
    }
  }
  if (flags & FLAG_NR) permute_bit_reversed(a, k);
  for (size_t i = 0; i < n; i++) fr_store(&f, out + 32 * i, &a[i], normal);
  free(a);
  free(tw);
  return 0;
}
