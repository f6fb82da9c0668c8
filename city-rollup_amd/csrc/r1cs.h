// Kernels of the device-resident R1CS (host side: r1cs.inc): A w, B w, C w as sparse matrix-vector products over the
// BLS12-381 scalar field, and the satisfaction check a o b = c. DESIGN.md section 4.6.
//
// No domain conversions: the witness and the outputs are canonical values split into 28-bit limbs in registers, the
// coefficient table is in Montgomery form (converted once at create), so fr_mul(c R, w) = c w is already canonical; a row
// accumulates with fr_add / fr_sub and is stored as it stands.
//
// A term is 8 bytes: the wire, and a tag = class | payload << 3. The payload is the index into the coefficient table
// (general terms) or the one-limb constant itself (small terms). A row's terms are sorted by class at create, so a lane
// walks its row in phases (all additions, all subtractions, ...) and the lanes of a wave are in the same phase together.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls12_381_fr.h"

namespace r1cs {

using blsfr::Fr;
using blsfr::LB;
using blsfr::LM;
using blsfr::NL;

enum : uint32_t { CLS_ADD = 0, CLS_SUB = 1, CLS_SMALL = 2, CLS_NEG_SMALL = 3, CLS_GENERAL = 4, N_CLS = 5 };
constexpr int TAG_BITS = 3;
constexpr uint32_t TAG_MASK = (1u << TAG_BITS) - 1;
constexpr uint32_t MAX_COEFFS = 1u << (32 - TAG_BITS);
constexpr uint32_t SMALL_LIMIT = 1u << LB;      // a small constant is one limb: 2 <= c < 2^28
constexpr size_t LONG_ROW_THRESHOLD = 128;      // a row of more terms takes a workgroup (k_eval_long), any other a lane
constexpr unsigned THREADS = 256;
constexpr size_t NO_ROW = ~(size_t)0;

struct Term { uint32_t col, tag; };
static_assert(sizeof(Term) == 8, "a term is one 8-byte load");

struct Matrix {
  const uint64_t *row_ptr;  // n_constraints + 1
  const Term *terms;
};
struct System {
  Matrix m[3];
  const Fr *coeffs;  // Montgomery form
  size_t n, n_pad;   // constraints, 2^log_domain
};

// ---- canonical 8 x 32-bit words <-> ten 28-bit limbs, no arithmetic -----------------------------------------------------
GL_HD Fr split_words(const uint32_t w[8]) {
  Fr r;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const int bit = LB * i, word = bit >> 5, sh = bit & 31;
    uint64_t v = word < 8 ? w[word] : 0;
    if (word + 1 < 8) v |= (uint64_t)w[word + 1] << 32;
    r.l[i] = (uint32_t)(v >> sh) & LM;
  }
  return r;
}
GL_HD void join_words(const Fr &a, uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const int bit = LB * i, word = bit >> 5, sh = bit & 31;
    const uint64_t v = (uint64_t)a.l[i] << sh;
    if (word < 8) w[word] |= (uint32_t)v;
    if (word + 1 < 8) w[word + 1] |= (uint32_t)(v >> 32);
  }
}
// an element of a canonical array (32 bytes, 32-byte aligned): two 16-byte loads / stores
__device__ __forceinline__ Fr load_canonical(const uint32_t *base, size_t i) {
  const uint4 *p = (const uint4 *)(base + 8 * i);
  const uint4 lo = p[0], hi = p[1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return split_words(w);
}
__device__ __forceinline__ void store_canonical(uint32_t *base, size_t i, const Fr &a) {
  uint32_t w[8];
  join_words(a, w);
  uint4 *p = (uint4 *)(base + 8 * i);
  p[0] = make_uint4(w[0], w[1], w[2], w[3]);
  p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// ---- a one-limb constant times a canonical value: 10 + 10 products instead of fr_mul's 200 ------------------------------
// t = c w < 2^28 r has 11 limbs. The quotient q = floor(t / r) is estimated from the bits above 2^224:
//   T1 = floor(t / 2^224) < 2^59,  R1 = floor(r / 2^224) (31 bits),  q' = floor(T1 / (R1 + 1)).
// q' <= q because T1 / (R1 + 1) < t / r. And t / r - q' < (T1 + 1) / R1 - T1 / (R1 + 1) + 1 = (T1 + R1 + 1) / (R1 (R1 + 1)) + 1
// < 2^59 / 2^61 + 1 < 2, so t - q' r < 3 r: two conditional subtractions finish it. q' <= q < 2^28 is one limb.
constexpr uint64_t SMALL_R1 = (uint64_t)BLS_FR_P[8] | ((uint64_t)BLS_FR_P[9] << LB);
static_assert(SMALL_R1 >> 30 == 1, "R1 = floor(r / 2^224) has 31 bits: R1^2 > 2^60 bounds the estimate's error below 1");
GL_HD Fr mul_small(const Fr &w, uint32_t c) {
  uint32_t t[NL + 1];
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    acc += (uint64_t)w.l[i] * c;  // < 2^56 + 2^28
    t[i] = (uint32_t)acc & LM;
    acc >>= LB;
  }
  t[NL] = (uint32_t)acc;  // < 2^28
  const uint64_t t1 = (uint64_t)t[8] | ((uint64_t)t[9] << LB) | ((uint64_t)t[10] << (2 * LB));
  const uint32_t q = (uint32_t)(t1 / (SMALL_R1 + 1));
  Fr r;
  uint64_t sub = 0;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    sub += (uint64_t)q * BLS_FR_P[i];
    const uint32_t d = t[i] - ((uint32_t)sub & LM) - br;
    r.l[i] = d & LM;
    br = d >> 31;
    sub >>= LB;
  }
  // the eleventh limb of t - q' r is zero (t - q' r < 3 r < 2^280): nothing is left to carry
  blsfr::fr_cond_sub(r);
  blsfr::fr_cond_sub(r);
  return r;
}

// one term into the running sum of a row
GL_HD Fr apply_class(const Fr &acc, uint32_t cls, uint32_t payload, const Fr *coeffs, const Fr &w) {
  switch (cls) {
    case CLS_ADD: return blsfr::fr_add(acc, w);
    case CLS_SUB: return blsfr::fr_sub(acc, w);
    case CLS_SMALL: return blsfr::fr_add(acc, mul_small(w, payload));
    case CLS_NEG_SMALL: return blsfr::fr_sub(acc, mul_small(w, payload));
    default: return blsfr::fr_add(acc, blsfr::fr_mul(coeffs[payload], w));
  }
}
__device__ __forceinline__ Fr apply_term(const Fr &acc, const Term t, const uint32_t *witness, const Fr *coeffs) {
  return apply_class(acc, t.tag & TAG_MASK, t.tag >> TAG_BITS, coeffs, load_canonical(witness, t.col));
}

// the class of a coefficient (4 x u64, host) and, for the one-limb classes, the constant
enum : uint32_t { CLS_ZERO = 100, CLS_NOT_CANONICAL = 101 };
inline uint32_t classify(const uint64_t c[4], uint32_t *small) {
  *small = 0;
  if (!blsfr::fr_is_canonical((const uint32_t *)c)) return CLS_NOT_CANONICAL;
  uint64_t neg[4];  // r - c
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    const uint64_t ri = (uint64_t)BLS_FR_P32[2 * i] | ((uint64_t)BLS_FR_P32[2 * i + 1] << 32);
    const uint64_t d = ri - c[i], e = d - br;
    br = (ri < c[i]) || (d < br);
    neg[i] = e;
  }
  const bool one_word = !(c[1] | c[2] | c[3]), neg_one_word = !(neg[1] | neg[2] | neg[3]);
  if (one_word && c[0] == 0) return CLS_ZERO;
  if (one_word && c[0] == 1) return CLS_ADD;
  if (neg_one_word && neg[0] == 1) return CLS_SUB;
  if (one_word && c[0] < SMALL_LIMIT) { *small = (uint32_t)c[0]; return CLS_SMALL; }
  if (neg_one_word && neg[0] < SMALL_LIMIT) { *small = (uint32_t)neg[0]; return CLS_NEG_SMALL; }
  return CLS_GENERAL;
}

// A row evaluated by one lane, in phases by class. The loop of a phase ends at the first term of a later class.
__device__ __forceinline__ Fr eval_row_lane(const Matrix &M, size_t beg, size_t end, const uint32_t *witness, const Fr *coeffs) {
  Fr acc = blsfr::fr_zero();
  size_t t = beg;
  Term cur = t < end ? M.terms[t] : Term{0, N_CLS};
#define R1CS_PHASE(CLS, EXPR)                                     \
  while ((cur.tag & TAG_MASK) == (CLS)) {                         \
    const Fr w = load_canonical(witness, cur.col);                \
    const uint32_t payload = cur.tag >> TAG_BITS;                 \
    (void)payload;                                                \
    acc = (EXPR);                                                 \
    t++;                                                          \
    cur = t < end ? M.terms[t] : Term{0, N_CLS};                  \
  }
  R1CS_PHASE(CLS_ADD, blsfr::fr_add(acc, w))
  R1CS_PHASE(CLS_SUB, blsfr::fr_sub(acc, w))
  R1CS_PHASE(CLS_SMALL, blsfr::fr_add(acc, mul_small(w, payload)))
  R1CS_PHASE(CLS_NEG_SMALL, blsfr::fr_sub(acc, mul_small(w, payload)))
  R1CS_PHASE(CLS_GENERAL, blsfr::fr_add(acc, blsfr::fr_mul(coeffs[payload], w)))
#undef R1CS_PHASE
  return acc;
}

// ---- short rows: a lane per row, grid.y = the matrix. Rows from n_constraints up to the domain size are written as zero;
// long rows are left to k_eval_long.
struct Outputs { uint32_t *p[3]; };
__global__ __launch_bounds__(THREADS) void k_eval_short(System S, const uint32_t *witness, Outputs out) {
  const size_t j = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (j >= S.n_pad) return;
  const Matrix &M = S.m[blockIdx.y];
  uint32_t *dst = out.p[blockIdx.y];
  if (j >= S.n) { store_canonical(dst, j, blsfr::fr_zero()); return; }
  const size_t beg = M.row_ptr[j], end = M.row_ptr[j + 1];
  if (end - beg > LONG_ROW_THRESHOLD) return;
  store_canonical(dst, j, eval_row_lane(M, beg, end, witness, S.coeffs));
}

// ---- long rows: a workgroup per row. long_rows[i] = matrix << 28 | row, ascending. The value goes to the row's place in the
// matrix's output array, or (out.p[matrix] == NULL: the check) to long_vals[i].
__global__ __launch_bounds__(THREADS) void k_eval_long(System S, const uint32_t *witness, const uint32_t *long_rows, Outputs out,
                                                       uint32_t *long_vals) {
  __shared__ Fr part[THREADS];
  const uint32_t key = long_rows[blockIdx.x];
  const uint32_t mat = key >> 28;
  const size_t j = key & ((1u << 28) - 1);
  const Matrix &M = S.m[mat];
  const size_t beg = M.row_ptr[j], end = M.row_ptr[j + 1];
  Fr acc = blsfr::fr_zero();
  for (size_t t = beg + threadIdx.x; t < end; t += THREADS) acc = apply_term(acc, M.terms[t], witness, S.coeffs);
  part[threadIdx.x] = acc;
  __syncthreads();
  for (unsigned half = THREADS / 2; half > 0; half >>= 1) {  // cross-lane tree of fr_add
    if (threadIdx.x < half) part[threadIdx.x] = blsfr::fr_add(part[threadIdx.x], part[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (out.p[mat]) store_canonical(out.p[mat], j, part[0]);
    else store_canonical(long_vals, blockIdx.x, part[0]);
  }
}

// ---- the check: rows j < n with a_j b_j != c_j counted, the lowest reported. counters[0] = count, counters[1] = lowest
// (initialised to ~0). FUSED: the three rows are evaluated here (long rows come from long_vals, found by binary search in
// long_rows); otherwise they are read from evaluated arrays.
__device__ __forceinline__ Fr row_value(const System &S, uint32_t mat, size_t j, const uint32_t *witness, const uint32_t *long_rows,
                                        uint32_t n_long, const uint32_t *long_vals) {
  const Matrix &M = S.m[mat];
  const size_t beg = M.row_ptr[j], end = M.row_ptr[j + 1];
  if (end - beg <= LONG_ROW_THRESHOLD) return eval_row_lane(M, beg, end, witness, S.coeffs);
  const uint32_t key = (mat << 28) | (uint32_t)j;
  uint32_t lo = 0, hi = n_long;  // the key is in the list: every long row was put there at create
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (long_rows[mid] <= key) lo = mid;
    else hi = mid;
  }
  return load_canonical(long_vals, lo);
}
template <bool FUSED>
__global__ __launch_bounds__(THREADS) void k_check(System S, const uint32_t *witness, const uint32_t *long_rows, uint32_t n_long,
                                                   const uint32_t *long_vals, const uint32_t *a_ev, const uint32_t *b_ev,
                                                   const uint32_t *c_ev, unsigned long long *counters) {
  const size_t j = (size_t)blockIdx.x * THREADS + threadIdx.x;
  bool bad = false;
  if (j < S.n) {
    Fr a, b, c;
    if (FUSED) {
      a = row_value(S, 0, j, witness, long_rows, n_long, long_vals);
      b = row_value(S, 1, j, witness, long_rows, n_long, long_vals);
      c = row_value(S, 2, j, witness, long_rows, n_long, long_vals);
    } else {
      a = load_canonical(a_ev, j);
      b = load_canonical(b_ev, j);
      c = load_canonical(c_ev, j);
    }
    // a b / R against c / R: both fully reduced, so equal exactly when a b = c (mod r)
    Fr one = blsfr::fr_zero();
    one.l[0] = 1;
    const Fr lhs = blsfr::fr_mul(a, b), rhs = blsfr::fr_mul(c, one);
    for (int i = 0; i < NL; i++) bad = bad || lhs.l[i] != rhs.l[i];
  }
  const unsigned long long mask = __ballot(bad);
  if (mask == 0) return;
  const unsigned lane = threadIdx.x & 63;
  if (lane == (unsigned)__ffsll((long long)mask) - 1) {  // the lowest violating lane of the wave holds the wave's lowest row
    atomicAdd(&counters[0], (unsigned long long)__popcll(mask));
    atomicMin(&counters[1], (unsigned long long)j);
  }
}

}  // namespace r1cs
