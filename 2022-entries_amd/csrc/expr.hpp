// expr.hpp -- custom-gate expressions over columns of Fr with rotations: the compiler from a DAG to a straight-line program, and the
// interpreter that runs the program for one row, on the arithmetic of fr.hpp.  One kernel per field serves every program.
//
// Reference behaviour: none to compare against (the reference has no Plonkish prover; halo2 calls this step evaluate_h).  The contract
// is stated on integers: out[i] = the DAG evaluated modulo r with COL(j, rot) = cols[j][((i + rot * rot_step) mod len) mod lens[j]].
//
// The DAG.  Nodes of three u32 (op, a, b) in topological order, the last one the result: COL (a: column, b: the rotation as a signed
// 32-bit value), CONST (a: index into the constants of create), CHAL (a: index into the challenges of a run), ADD, SUB, MUL (a, b:
// earlier nodes), NEG, SQR (a).  Nodes the result does not depend on cost nothing.
//
// The program (expr_compile).  Instructions of three u32: w0 = op | dst << 8 | m << 16, w1 and w2 = the operands, kind << 28 | index.
// An operand is a slot, the accumulator (the value of the most recent instruction without a slot: a node whose only use is the next
// instruction never touches LDS), a column reference (column, rotation), a constant or a challenge.  Leaves are never kept: a column
// operand is loaded where it is used and pays its conversion there.  The order of evaluation is a post-order walk from the result that
// takes the operand with the larger Sethi-Ullman label first; a linear scan then hands out the lowest free slot and frees a slot with
// the last use of its node.  S = the number of slots in use at once, at most EXPR_MAX_SLOTS.
//
// The stored form and the bounds.  A slot, the accumulator and every loaded operand is a 256-bit integer (8 words) that stands for
// value / R mod r, R = 2^261, as fr.hpp's "stored as 256 bits".  The compiler carries for every node an upper bound B (value <= B r)
// and keeps every stored value below 2^256, i.e. B <= LIM = 2^256 / r (13.7 for BLS12-377, 2.208 for BLS12-381) -- which is tighter
// than what fr_mul asks of its operands (B_a B_b <= 2^261 / r = 32 LIM), so a product never needs a reduction of its own:
//   leaf            a constant or a challenge is canonical, a column is brought below r after its conversion:    B = 1
//   MUL, SQR        unpack, one fr_mul, pack:                                              B = 1 + B_a B_b / (32 LIM)
//   ADD             a + b on 256-bit integers:                                             B = B_a + B_b
//   SUB, NEG        a + m r - b with m = ceil(B_b) (NEG: a = 0):                             B = B_a + m
// Where B would pass LIM the compiler first reduces an operand in place: RED, one conditional subtraction of r (B -> max(1, B - 1)),
// while B <= 3, else MUL1, a product by one (B -> 1 + B / (32 LIM)); the larger operand first, the subtrahend of a SUB before
// the minuend.  Both count in "reduces", MUL1 also in "products".  The host build runs every instruction under MSM_CHECK: no carry out
// of an ADD, no borrow out of a SUB, every fr_mul column and result.
//
// The interpreter (expr_row).  One lane per row; the slots live lane-interleaved (word q of slot s of lane l at (s * 8 + q) * L + l, L
// lanes per block on the device, 1 on the host), so no lane reads another's and no barrier is needed.  The loop over the instructions
// and the loop over the two operands are rolled; program counter, op and operand numbers are wave-uniform, and only the column reads
// are indexed by the lane.  The code holds three products: the conversion of a column, the product of MUL / SQR / MUL1, the
// conversion of the result.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "fr.hpp"

namespace msm {

constexpr unsigned kExprNormal = 1u, kExprDevice = 2u;        // the flags of a call: plain integers; device pointers
constexpr uint32_t EXPR_LANES = 64;                           // lanes per block: one wave
constexpr uint32_t EXPR_MAX_NODES = 65535, EXPR_MAX_CONSTS = 4096, EXPR_MAX_CHALS = 64, EXPR_MAX_COLS = 64, EXPR_MAX_ROT = 1u << 15;
constexpr uint32_t EXPR_MAX_LEN_LOG = 30;
// 32 slots are 64 KiB of LDS for a block of one wave: two waves per CU of 160 KiB.  With one wave per CU three of the four SIMDs idle,
// and splitting the sum over an output column costs less than that.
constexpr uint32_t EXPR_MAX_SLOTS = 32;

enum : uint32_t { EXPR_COL = 0, EXPR_CONST = 1, EXPR_CHAL = 2, EXPR_ADD = 3, EXPR_SUB = 4, EXPR_MUL = 5, EXPR_NEG = 6, EXPR_SQR = 7 };
// instructions: x = a + b, a + m r - b, a b, a a, a - [a >= r] r, a 1, a
enum : uint32_t { EXPR_I_ADD = 0, EXPR_I_SUB = 1, EXPR_I_MUL = 2, EXPR_I_SQR = 3, EXPR_I_RED = 4, EXPR_I_MUL1 = 5, EXPR_I_MOV = 6 };
// operand kinds; a missing operand reads as zero
enum : uint32_t { EXPR_K_NONE = 0, EXPR_K_SLOT = 1, EXPR_K_ACC = 2, EXPR_K_COL = 3, EXPR_K_CONST = 4, EXPR_K_CHAL = 5 };
constexpr uint32_t EXPR_NO_DST = 0xff;

MSM_HD uint32_t expr_lds_bytes(uint32_t slots) { return slots * 8 * 4 * EXPR_LANES; }

// a column reference of one run: where the column lies, its length and (rot * rot_step) mod len
struct ExprColRef {
  const uint32_t* base;
  uint32_t len, shift;
};

struct ExprRun {
  const uint32_t* prog;        // 3 words per instruction
  const ExprColRef* refs;
  const uint32_t* consts;      // 8 words each: canonical, times R
  const uint32_t* chals;       // the same, of this run
  uint32_t* out;
  uint32_t ninstr, len, normal;
};

// the slots of one lane: L = EXPR_LANES in LDS, 1 on the host
template <uint32_t L>
struct ExprSlots {
  uint32_t* base;
  MSM_HD void load(uint32_t (&w)[8], uint32_t slot) const {
#pragma unroll
    for (int q = 0; q < 8; q++) w[q] = base[(slot * 8 + q) * L];
  }
  MSM_HD void store(uint32_t slot, const uint32_t (&w)[8]) const {
#pragma unroll
    for (int q = 0; q < 8; q++) base[(slot * 8 + q) * L] = w[q];
  }
};

// x = a + m r - b on 256-bit integers; the compiler keeps b <= m r and the result below 2^256
template <class FR>
MSM_HD void expr_sub_words(uint32_t (&x)[8], const uint32_t (&a)[8], const uint32_t (&b)[8], uint32_t m) {
  int64_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    c += (int64_t)((uint64_t)FR::P32[j] * m) + (int64_t)a[j] - (int64_t)b[j];
    x[j] = (uint32_t)c;
    c >>= 32;
  }
  MSM_CHECK(c == 0);
}

MSM_HD void expr_add_words(uint32_t (&x)[8], const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    c += (uint64_t)a[j] + b[j];
    x[j] = (uint32_t)c;
    c >>= 32;
  }
  MSM_CHECK(c == 0);
}

// row i of a run
template <class FR, class ST>
MSM_HD void expr_row(const ST& st, const ExprRun& p, uint32_t i) {
  uint32_t acc[8];
#pragma unroll
  for (int q = 0; q < 8; q++) acc[q] = 0;
#pragma unroll 1
  for (uint32_t pc = 0; pc < p.ninstr; pc++) {
    const uint32_t w0 = p.prog[3 * pc], w1 = p.prog[3 * pc + 1], w2 = p.prog[3 * pc + 2];
    const uint32_t op = w0 & 0xff, dst = (w0 >> 8) & 0xff, m = w0 >> 16;
    uint32_t a[8], b[8];
#pragma unroll 1
    for (uint32_t k = 0; k < 2; k++) {
      const uint32_t ref = k ? w2 : w1, kind = ref >> 28, idx = ref & 0x0fffffffu;
      uint32_t t[8];
      if (kind == EXPR_K_SLOT) {
        st.load(t, idx);
      } else if (kind == EXPR_K_COL) {
        const ExprColRef c = p.refs[idx];
        uint32_t row = i + c.shift;                // both below len <= 2^30
        if (row >= p.len) row -= p.len;
        if (c.len != p.len) row %= c.len;
        const uint32_t* src = c.base + (uint64_t)row * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = src[q];
        Fr x;
        fr_from_abi<FR>(x, t, p.normal != 0);
        fr_pack(t, x);
        fr_canon<FR>(t);
      } else if (kind == EXPR_K_CONST || kind == EXPR_K_CHAL) {
        const uint32_t* src = (kind == EXPR_K_CONST ? p.consts : p.chals) + idx * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = src[q];
      } else {
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = kind == EXPR_K_ACC ? acc[q] : 0u;
      }
#pragma unroll
      for (int q = 0; q < 8; q++) {
        if (k == 0) a[q] = t[q]; else b[q] = t[q];
      }
    }
    uint32_t x[8];
    if (op == EXPR_I_MUL || op == EXPR_I_SQR || op == EXPR_I_MUL1) {
      Fr fa, fb;
      fr_unpack(fa, a);
      if (op == EXPR_I_MUL) fr_unpack(fb, b); else if (op == EXPR_I_SQR) fb = fa; else fr_set<FR>(fb, FR::ONE);
      fr_mul<FR>(fa, fa, fb);
      fr_pack(x, fa);
    } else if (op == EXPR_I_ADD) {
      expr_add_words(x, a, b);
    } else if (op == EXPR_I_SUB) {
      expr_sub_words<FR>(x, a, b, m);
    } else {
#pragma unroll
      for (int q = 0; q < 8; q++) x[q] = a[q];
      if (op == EXPR_I_RED) fr_canon<FR>(x);
    }
    if (dst != EXPR_NO_DST) {
      st.store(dst, x);
    } else {
#pragma unroll
      for (int q = 0; q < 8; q++) acc[q] = x[q];
    }
  }
  Fr f;
  uint32_t w[8];
  fr_unpack(f, acc);
  fr_to_abi<FR>(w, f, p.normal != 0);
  uint32_t* dst = p.out + (uint64_t)i * 8;
#pragma unroll
  for (int q = 0; q < 8; q++) dst[q] = w[q];
}

// ---- the compiler (host) ---------------------------------------------------------------------------------------------------------------

struct ExprProgram {
  std::vector<uint32_t> code;                             // 3 words per instruction
  std::vector<std::pair<uint32_t, int32_t>> refs;         // the distinct (column, rotation) pairs, in the order of their first use
  uint32_t n_nodes = 0, n_consts = 0, n_chal = 0, n_cols = 0, slots = 0;
  uint64_t products = 0, reduces = 0;                     // per row: conversions, MUL, SQR and MUL1; RED and MUL1
  uint64_t rot0_only = 0, used_cols = 0;                  // bit j: column j is read, and at rotation 0 only
  uint32_t ninstr() const { return (uint32_t)(code.size() / 3); }
};

// 2^256 / r, rounded down a little: the most a stored value may reach in units of r
template <class FR>
double expr_store_limit() { return 4294967296.0 / ((double)FR::P32[7] + 1.0); }

// the limits of create, in the order of the header: false with a message
inline bool expr_check_dag(const uint32_t* nodes, size_t n_nodes, size_t n_consts, size_t n_chal, size_t n_cols, char* msg, size_t msg_len) {
  if (n_nodes < 1) return snprintf(msg, msg_len, "an expression has at least one node"), false;
  if (n_nodes > EXPR_MAX_NODES) return snprintf(msg, msg_len, "%zu nodes exceed %u", n_nodes, EXPR_MAX_NODES), false;
  if (n_consts > EXPR_MAX_CONSTS) return snprintf(msg, msg_len, "%zu constants exceed %u", n_consts, EXPR_MAX_CONSTS), false;
  if (n_chal > EXPR_MAX_CHALS) return snprintf(msg, msg_len, "%zu challenges exceed %u", n_chal, EXPR_MAX_CHALS), false;
  if (n_cols > EXPR_MAX_COLS) return snprintf(msg, msg_len, "%zu columns exceed %u", n_cols, EXPR_MAX_COLS), false;
  for (size_t i = 0; i < n_nodes; i++) {
    const uint32_t op = nodes[3 * i], a = nodes[3 * i + 1], b = nodes[3 * i + 2];
    if (op > EXPR_SQR) return snprintf(msg, msg_len, "node %zu: unknown op %u", i, op), false;
    if (op == EXPR_COL) {
      const int64_t rot = (int32_t)b;
      if (a >= n_cols) return snprintf(msg, msg_len, "node %zu: column %u of %zu", i, a, n_cols), false;
      if (rot > (int64_t)EXPR_MAX_ROT || rot < -(int64_t)EXPR_MAX_ROT) return snprintf(msg, msg_len, "node %zu: rotation %lld outside +-2^15", i, (long long)rot), false;
    } else if (op == EXPR_CONST) {
      if (a >= n_consts) return snprintf(msg, msg_len, "node %zu: constant %u of %zu", i, a, n_consts), false;
    } else if (op == EXPR_CHAL) {
      if (a >= n_chal) return snprintf(msg, msg_len, "node %zu: challenge %u of %zu", i, a, n_chal), false;
    } else {
      const bool two = op == EXPR_ADD || op == EXPR_SUB || op == EXPR_MUL;
      if (a >= i || (two && b >= i)) return snprintf(msg, msg_len, "node %zu: an operand is not an earlier node (the nodes come in topological order)", i), false;
    }
  }
  return true;
}

// the DAG (already judged by expr_check_dag) to a program; K = 32 lim.  False with a message when the slots do not suffice.
inline bool expr_compile(ExprProgram& pr, const uint32_t* nodes, size_t n_nodes, size_t n_consts, size_t n_chal, size_t n_cols, double lim, char* msg,
                         size_t msg_len) {
  const double K = 32 * lim;
  const uint32_t N = (uint32_t)n_nodes, root = N - 1;
  auto op_of = [&](uint32_t n) { return nodes[3 * n]; };
  auto leaf = [&](uint32_t n) { return op_of(n) <= EXPR_CHAL; };
  auto arity = [&](uint32_t n) { return leaf(n) ? 0u : (op_of(n) == EXPR_NEG || op_of(n) == EXPR_SQR) ? 1u : 2u; };
  auto child = [&](uint32_t n, uint32_t k) { return nodes[3 * n + 1 + k]; };
  pr = ExprProgram();
  pr.n_nodes = N;
  pr.n_consts = (uint32_t)n_consts;
  pr.n_chal = (uint32_t)n_chal;
  pr.n_cols = (uint32_t)n_cols;
  // what the result depends on, and how often each node is used by such nodes
  std::vector<uint8_t> live(N, 0);
  std::vector<uint32_t> uses(N, 0), label(N, 0);
  live[root] = 1;
  for (uint32_t n = N; n-- > 0;) {
    if (!live[n]) continue;
    for (uint32_t k = 0; k < arity(n); k++) {
      live[child(n, k)] = 1;
      uses[child(n, k)]++;
    }
  }
  // Sethi-Ullman labels: a leaf takes no slot
  for (uint32_t n = 0; n < N; n++) {
    if (!live[n] || leaf(n)) continue;
    uint32_t l[2] = {0, 0};
    for (uint32_t k = 0; k < arity(n); k++) l[k] = leaf(child(n, k)) ? 0 : label[child(n, k)];
    label[n] = l[0] == l[1] ? l[0] + 1 : (l[0] > l[1] ? l[0] : l[1]);
    if (label[n] < 1) label[n] = 1;
  }
  // the order: post-order from the result, the heavier operand first, every node once
  std::vector<uint32_t> order;
  {
    std::vector<uint8_t> done(N, 0);
    std::vector<std::pair<uint32_t, uint32_t>> stack;   // (node, operands already visited)
    if (!leaf(root)) stack.push_back({root, 0});
    while (!stack.empty()) {
      const uint32_t n = stack.back().first, at = stack.back().second;
      if (done[n]) {
        stack.pop_back();
        continue;
      }
      const uint32_t ar = arity(n);
      if (at < ar) {
        stack.back().second++;
        uint32_t k = at;
        if (ar == 2 && label[child(n, 1)] > label[child(n, 0)]) k = 1 - at;
        const uint32_t c = child(n, k);
        if (!leaf(c) && !done[c]) stack.push_back({c, 0});
      } else {
        done[n] = 1;
        order.push_back(n);
        stack.pop_back();
      }
    }
  }
  // the linear scan
  std::vector<double> bound(N, 1.0);
  std::vector<int32_t> slot(N, -1);        // -1: no slot (a leaf, not yet evaluated, or in the accumulator)
  std::vector<uint32_t> left = uses;
  std::vector<uint8_t> free_slot(256, 1);
  std::map<std::pair<uint32_t, int32_t>, uint32_t> ref_at;
  uint32_t in_use = 0, most = 0;
  uint64_t rotated = 0;
  auto emit = [&](uint32_t op, uint32_t dst, uint32_t m, uint32_t a, uint32_t b) {
    pr.code.push_back(op | dst << 8 | m << 16);
    pr.code.push_back(a);
    pr.code.push_back(b);
  };
  auto operand = [&](uint32_t c) -> uint32_t {
    const uint32_t o = op_of(c);
    if (o == EXPR_COL) {
      const std::pair<uint32_t, int32_t> key{nodes[3 * c + 1], (int32_t)nodes[3 * c + 2]};
      auto it = ref_at.find(key);
      if (it == ref_at.end()) {
        it = ref_at.insert({key, (uint32_t)pr.refs.size()}).first;
        pr.refs.push_back(key);
        pr.used_cols |= 1ull << key.first;
        if (key.second != 0) rotated |= 1ull << key.first;
      }
      pr.products++;
      return EXPR_K_COL << 28 | it->second;
    }
    if (o == EXPR_CONST) return EXPR_K_CONST << 28 | nodes[3 * c + 1];
    if (o == EXPR_CHAL) return EXPR_K_CHAL << 28 | nodes[3 * c + 1];
    return slot[c] >= 0 ? EXPR_K_SLOT << 28 | (uint32_t)slot[c] : EXPR_K_ACC << 28;
  };
  // one step of reduction of the interior node c, where it lies
  auto reduce = [&](uint32_t c) {
    const uint32_t where = slot[c] >= 0 ? EXPR_K_SLOT << 28 | (uint32_t)slot[c] : EXPR_K_ACC << 28;
    const uint32_t dst = slot[c] >= 0 ? (uint32_t)slot[c] : EXPR_NO_DST;
    if (bound[c] <= 3) {
      emit(EXPR_I_RED, dst, 0, where, 0);
      bound[c] = bound[c] - 1 > 1 ? bound[c] - 1 : 1;
    } else {
      emit(EXPR_I_MUL1, dst, 0, where, 0);
      bound[c] = 1 + bound[c] / K;
      pr.products++;
    }
    pr.reduces++;
  };
  auto reducible = [&](uint32_t c) { return !leaf(c) && bound[c] > 1; };
  for (size_t at = 0; at < order.size(); at++) {
    const uint32_t n = order[at], o = op_of(n), ar = arity(n);
    const uint32_t ca = child(n, 0), cb = ar == 2 ? child(n, 1) : ca;
    double res = 0;
    uint32_t m = 0;
    for (;;) {
      const double ba = bound[ca], bb = bound[cb];
      bool fits;
      if (o == EXPR_ADD) {
        res = ba + bb;
        fits = res <= lim;
      } else if (o == EXPR_SUB || o == EXPR_NEG) {
        m = (uint32_t)std::ceil(bb);
        res = (o == EXPR_SUB ? ba : 0) + m;
        fits = res <= lim;
      } else {
        res = 1 + ba * bb / K;
        fits = ba * bb <= 0.9 * K;
      }
      if (fits) break;
      uint32_t pick;
      if (o == EXPR_SUB) pick = reducible(cb) ? cb : ca;
      else if (o == EXPR_NEG) pick = cb;
      else pick = (reducible(ca) && (ba >= bb || !reducible(cb))) ? ca : cb;
      if (!reducible(pick)) return snprintf(msg, msg_len, "node %u: the bounds cannot be kept (internal error)", n), false;
      reduce(pick);
    }
    uint32_t wa = 0, wb = 0;
    if (o == EXPR_NEG) {
      wb = operand(ca);
    } else {
      wa = operand(ca);
      if (ar == 2) wb = operand(cb);
    }
    for (uint32_t k = 0; k < ar; k++) {
      const uint32_t c = child(n, k);
      if (leaf(c)) continue;
      if (--left[c] == 0 && slot[c] >= 0) {
        free_slot[slot[c]] = 1;
        slot[c] = -1;
        in_use--;
      }
    }
    // the result: the accumulator when its only use is the next instruction (or it is the result of the program), else the lowest free slot
    uint32_t dst = EXPR_NO_DST;
    const bool next_takes = at + 1 < order.size() && uses[n] == 1 && (child(order[at + 1], 0) == n || (arity(order[at + 1]) == 2 && child(order[at + 1], 1) == n));
    if (n != root && !next_takes) {
      uint32_t s = 0;
      while (!free_slot[s]) s++;
      if (s >= EXPR_NO_DST) return snprintf(msg, msg_len, "the program needs more than %u slots", EXPR_NO_DST), false;
      free_slot[s] = 0;
      slot[n] = (int32_t)s;
      dst = s;
      in_use++;
      if (in_use > most) most = in_use;
    }
    const uint32_t iop = o == EXPR_ADD ? EXPR_I_ADD : (o == EXPR_SUB || o == EXPR_NEG) ? EXPR_I_SUB : o == EXPR_MUL ? EXPR_I_MUL : EXPR_I_SQR;
    if (iop == EXPR_I_MUL || iop == EXPR_I_SQR) pr.products++;
    emit(iop, dst, iop == EXPR_I_SUB ? m : 0, wa, wb);
    bound[n] = res;
  }
  if (leaf(root)) emit(EXPR_I_MOV, EXPR_NO_DST, 0, operand(root), 0);
  pr.products++;   // the conversion of the result
  pr.slots = most;
  pr.rot0_only = pr.used_cols & ~rotated;
  if (most > EXPR_MAX_SLOTS)
    return snprintf(msg, msg_len, "the program needs S = %u slots, the kernel's limit is %u: split the sum over an output column", most, EXPR_MAX_SLOTS), false;
  return true;
}

// (rot * rot_step) mod len in [0, len), for len >= 1
inline uint32_t expr_shift(int32_t rot, uint64_t rot_step, uint64_t len) {
  const uint64_t step = rot_step % len, r = (uint64_t)(rot < 0 ? -(int64_t)rot : rot) * step % len;
  return (uint32_t)(rot < 0 && r ? len - r : r);
}

#if defined(__HIPCC__)
template <class FR>
__global__ void __launch_bounds__(EXPR_LANES) k_expr_rows(ExprRun p) {
  extern __shared__ uint32_t expr_lds[];
  const uint64_t i = (uint64_t)blockIdx.x * EXPR_LANES + threadIdx.x;
  if (i >= p.len) return;
  const ExprSlots<EXPR_LANES> st{expr_lds + threadIdx.x};
  expr_row<FR>(st, p, (uint32_t)i);
}
#endif

}  // namespace msm
