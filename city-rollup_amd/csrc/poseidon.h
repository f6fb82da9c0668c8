// Poseidon-Goldilocks permutation (width 12, rate 8, x^7, 4 + 22 + 4 rounds) for gfx950.
//
// Replaces plonky2's `PoseidonHash` / `PoseidonPermutation` (un-vendored dependency of the
// reference; call sites: city_crypto/src/hash/traits/hasher.rs:77-159 and every Merkle tree /
// challenger use inside `CircuitData::prove`).
//
// One lane owns one 12-element state (24 VGPRs): no cross-lane traffic, integer and fp64 VALU only, bound by instruction
// issue. What shapes the code (measured on MI355X, profiles/r01_ubench_valu.txt, r02_ubench_poseidon.txt):
//   * a 64-bit modular multiplication is 11 instructions (gl.h: `mul_wide_cy`, `reduce128_lazy`, `fold_top` — three pieces in `asm`);
//   * the MDS layer (circulant, entries <= 41, + diag 8) uses NO integer multiplies at all: the length-12 cyclic
//     convolution is evaluated per limb plane through the CRT split
//         x^12-1 = (x^6-1)(x^6+1),  x^6-1 = (x^3-1)(x^3+1)
//     whose transformed kernels are all +-powers of two ([16,16,32], [-1,-8,2], [2,-4,16,1,-1,-1]): ~90 operations per plane
//     instead of 288 multiply-adds per state — on two 32-bit limb planes in DOUBLE PRECISION (exact: everything stays below
//     2^53; `mds_layer_d`), which beat the three 22-bit integer planes of `mds_limb` by 15 % on the whole permutation;
//   * state is carried lazily (any u64 congruent to the value); the next round's constant is
//     folded into the recombination, and only the final output is canonicalised;
//   * the 22 partial rounds never leave the transformed domain of that CRT split (see `permute_until`), and keep their limb planes in
//     units of 2^32, where the carry of a normalisation is one rounding instruction (`renorm32_d`: 6 operations per component, not 8).
#pragma once
#include "gl.h"
#include "poseidon_tables.h"

namespace poseidon {

constexpr int W = 12;
constexpr int RATE = 8;
constexpr int HALF_FULL = 4;
constexpr int PARTIAL = 22;
constexpr int ROUNDS = 2 * HALF_FULL + PARTIAL;
static_assert(RATE % 2 == 0 && W % 2 == 0, "the S-boxes of a round go in pairs (sbox_lazy2)");

// device copy of the round constants (uniform index -> scalar loads)
__constant__ uint64_t d_RC[ROUNDS * W];

GL_HD uint64_t rc(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return d_RC[i];
#else
  return POSEIDON_RC[i];
#endif
}
// Constants of the double-precision layers (`recombine_d`): each constant c, minus the bit pattern of 1.5 * 2^52 at both limb
// positions, as the two doubles 1.5 * 2^52 + lo32 and 1.5 * 2^52 + hi32 — added to a limb they convert it to an integer AND
// add the constant in one operation. RCD = the round constants (+ one entry for "no constant"); DDK / DDLAST = the partial-round constants pushed
// forward through the MDS (gen_tables.plane_constants: one scalar per partial round on element 0, one vector after the last).
// Hosts upload all three; only the forms kept for the A/B read them (POSEIDON_RECOMBINE_V1, POSEIDON_PARTIAL_V1): the default build
// takes the tables of `recombine_s` below.
struct Magic { double m0, m1; };
__constant__ uint64_t d_RCD[2 * (ROUNDS * W + 1)];
__constant__ uint64_t d_DDK[2 * PARTIAL];
__constant__ uint64_t d_DDLAST[2 * W];
// The partial rounds keep their planes in units of 2^32 (`renorm32_d`): a limb l arrives as l 2^-32 and is converted by 1.5 * 2^20, whose
// mantissa is the one of 1.5 * 2^52 under another exponent field; POSEIDON_DOMD32_* are the same constants with that difference taken out.
// DDK_HOST / DDLAST_HOST: what the form compiled here reads, and what a host uploads into d_DDK / d_DDLAST.
#if defined(POSEIDON_RENORM_MAGIC)  // planes in units of 1 and the two-operation carry (rounds 2-4 of the build): kept for the A/B
constexpr bool UNITS32 = false;
static const uint64_t (&DDK_HOST)[2 * PARTIAL] = POSEIDON_DOMD_K;
static const uint64_t (&DDLAST_HOST)[2 * W] = POSEIDON_DOMD_LAST;
#else
constexpr bool UNITS32 = true;
static const uint64_t (&DDK_HOST)[2 * PARTIAL] = POSEIDON_DOMD32_K;
static const uint64_t (&DDLAST_HOST)[2 * W] = POSEIDON_DOMD32_LAST;
#endif
GL_HD Magic rcd(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return {__builtin_bit_cast(double, d_RCD[2 * i]), __builtin_bit_cast(double, d_RCD[2 * i + 1])};
#else
  return {__builtin_bit_cast(double, POSEIDON_RCD[2 * i]), __builtin_bit_cast(double, POSEIDON_RCD[2 * i + 1])};
#endif
}
GL_HD Magic domd_k(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return {__builtin_bit_cast(double, d_DDK[2 * i]), __builtin_bit_cast(double, d_DDK[2 * i + 1])};
#else
  return {__builtin_bit_cast(double, DDK_HOST[2 * i]), __builtin_bit_cast(double, DDK_HOST[2 * i + 1])};
#endif
}
GL_HD Magic domd_last(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return {__builtin_bit_cast(double, d_DDLAST[2 * i]), __builtin_bit_cast(double, d_DDLAST[2 * i + 1])};
#else
  return {__builtin_bit_cast(double, DDLAST_HOST[2 * i]), __builtin_bit_cast(double, DDLAST_HOST[2 * i + 1])};
#endif
}
// The constants of `recombine_s` (below `recombine_d`): the same three families with T0 * (2^32 - 1) put back for the literal T0 that
// the recombination takes off its top word (gen_tables.top0_literals). They are compile-time tables of the header, read in place (a
// uniform index: scalar loads) — no host uploads them. POSEIDON_RECOMBINE_V1: `recombine_d` and its tables everywhere, kept for the A/B.
#if defined(POSEIDON_RECOMBINE_V1)
constexpr bool SMALL_TOP = false;
#else
constexpr bool SMALL_TOP = true;
#endif
constexpr uint32_t TOP0_PLANES = UNITS32 ? POSEIDON_TOP0_PARTIAL32 : POSEIDON_TOP0_PARTIAL;
GL_HD Magic rcs(int i) { return {__builtin_bit_cast(double, POSEIDON_RCS[2 * i]), __builtin_bit_cast(double, POSEIDON_RCS[2 * i + 1])}; }
GL_HD Magic doms_k(int i) {
  const uint64_t(&t)[2 * PARTIAL] = UNITS32 ? POSEIDON_DOMS32_K : POSEIDON_DOMS_K;
  return {__builtin_bit_cast(double, t[2 * i]), __builtin_bit_cast(double, t[2 * i + 1])};
}
GL_HD Magic doms_last(int i) {
  const uint64_t(&t)[2 * W] = UNITS32 ? POSEIDON_DOMS32_LAST : POSEIDON_DOMS_LAST;
  return {__builtin_bit_cast(double, t[2 * i]), __builtin_bit_cast(double, t[2 * i + 1])};
}
// ---- what a caller keeps of a permutation, and what it knows of its input --------------------------------------------------
// `hash_no_pad` is an overwrite-mode sponge: the rate words 0..7 of every permutation but a leaf's last are overwritten by the
// next chunk, and of the last one (and of a tree node's only one) words 0..3 are the digest. `permute_until<OUT, ZERO_CAP>`:
// OUT says which outputs are live — the last layer leaves the transformed domain, recombines and canonicalises only those, and
// clears the others — and ZERO_CAP that the capacity words 8..11 of the input are known to be zero (every tree node, the first
// permutation of a leaf): their first round is then four table constants (POSEIDON_CAP0_SBOX = (0 + rc[8 + i])^7) and what `s`
// holds there is not read. Both are compile-time: with the form in registers the leaf hash spilled 30-50 registers where it
// spills 6, so a sponge loop has one call per form it needs (merkle.h k_leaf_hash_cols).
enum : int {
  OUT_ALL = 0,       // all twelve, canonical
  OUT_CAPACITY = 1,  // words 8..11, lazy (any u64 congruent to the value: what the next permutation's `add_const_lazy` takes)
  OUT_DIGEST = 2     // words 0..3, canonical
};
// ---- lazy field helpers: inputs/outputs are arbitrary u64 congruent to the value ----------
using gl::fold_top;
using gl::mul_lazy;
using gl::mul_lazy2;
// x^7 = x^3 x^4: x^3 and x^4 are one pair of products (`gl::mul_lazy2`), so an S-box is three products deep, not four
GL_HD uint64_t sbox_lazy(uint64_t x) {
  const uint64_t x2 = mul_lazy(x, x);
  uint64_t x3, x4;
  mul_lazy2(x, x2, x2, x2, x3, x4);
  return mul_lazy(x3, x4);
}
// two S-boxes, every product of one paired with the same product of the other: what a round does to several words
GL_HD void sbox_lazy2(uint64_t &x, uint64_t &y) {
  uint64_t x2, y2, x3, y3, x4, y4;
  mul_lazy2(x, x, y, y, x2, y2);
  mul_lazy2(x, x2, y, y2, x3, y3);
  mul_lazy2(x2, x2, y2, y2, x4, y4);
  mul_lazy2(x3, x4, y3, y4, x, y);
}
// The S-box of the partial rounds (`partial_rounds`), one product after the other: there the two limb planes of the state are live
// (48 registers) and the pair's second set of temporaries is what does not fit — with `sbox_lazy` the leaf hash (96 registers) spills
// 7 registers where it spills 6 and k_level grows from 96 registers to 98, a resident wave less.
GL_HD uint64_t sbox_lazy_chain(uint64_t x) {
  const uint64_t x2 = mul_lazy(x, x), x4 = mul_lazy(x2, x2), x3 = mul_lazy(x, x2);
  return mul_lazy(x3, x4);
}
GL_HD uint64_t add_const_lazy(uint64_t a, uint64_t c) {  // c canonical
  uint64_t s = a + c;
  if (s < a) {  // wrapped: 2^64 == EPS
    s += gl::EPS;
    if (s < gl::EPS) s += gl::EPS;  // (cannot happen for c < p, kept for safety)
  }
  return s;
}

// ---- MDS layer on one 22-bit limb plane, arithmetic mod 2^32 (exact: true results < 2^31) ----
// y[r] = sum_i C[i] * s[(i+r) % 12] + 8*s[0]*[r==0],  C = {17,15,41,16,2,28,13,13,39,18,34,20}
// as T^-1' . K . T: T = two butterfly levels (`dom_enter`), K = three small component-wise products (`dom_mul`),
// T^-1' = the butterflies back (`dom_leave`). Index layout of a transformed plane: [0..2] = aa, [3..5] = ab, [6..11] = b.
GL_HD void dom_enter(const uint32_t (&s)[W], uint32_t (&u)[W]) {
  uint32_t a[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    a[i] = s[i] + s[i + 6];
    u[6 + i] = s[i] - s[i + 6];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    u[i] = a[i] + a[i + 3];
    u[3 + i] = a[i] - a[i + 3];
  }
}
GL_HD void dom_mul(const uint32_t (&u)[W], uint32_t (&o)[W]) {
  typedef uint32_t T;
  // cyclic-3 part: aa (*) [16,16,32]
  const T T16 = (u[0] + u[1] + u[2]) << 4;
  o[0] = T16 + (u[2] << 4);
  o[1] = T16 + (u[0] << 4);
  o[2] = T16 + (u[1] << 4);
  // negacyclic-3 part: ab (*) [-1,-8,2]
  o[3] = (u[5] << 3) - u[3] - (u[4] << 1);
  o[4] = (T)0 - (u[3] << 3) - u[4] - (u[5] << 1);
  o[5] = (u[3] << 1) - (u[4] << 3) - u[5];
  // negacyclic-6 part: b (*) N mod (x^6+1), N = [2,-4,16,1,-1,-1]:  v[k] = sum_{i+j=k} b[i]N[j] - sum_{i+j=k+6} b[i]N[j]
  const T *b = &u[6];
  T nb[6];
#pragma unroll
  for (int i = 0; i < 6; i++) nb[i] = (T)0 - b[i];
  o[6] = (b[0] << 1) + b[1] + b[2] + nb[3] + (nb[4] << 4) + (b[5] << 2);
  o[7] = (nb[0] << 2) + (b[1] << 1) + b[2] + b[3] + nb[4] + (nb[5] << 4);
  o[8] = (b[0] << 4) + (nb[1] << 2) + (b[2] << 1) + b[3] + b[4] + nb[5];
  o[9] = b[0] + (b[1] << 4) + (nb[2] << 2) + (b[3] << 1) + b[4] + b[5];
  o[10] = nb[0] + b[1] + (b[2] << 4) + (nb[3] << 2) + (b[4] << 1) + b[5];
  o[11] = nb[0] + nb[1] + b[2] + (b[3] << 4) + (nb[4] << 2) + (b[5] << 1);
}
GL_HD void dom_leave(const uint32_t (&o)[W], uint32_t (&y)[W]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const uint32_t p = o[i] + o[3 + i], q = o[i] - o[3 + i];
    y[i] = p + o[6 + i];
    y[i + 6] = p - o[6 + i];
    y[i + 3] = q + o[9 + i];
    y[i + 9] = q - o[9 + i];
  }
}
GL_HD void mds_limb(const uint32_t (&s)[W], uint32_t (&y)[W]) {
  uint32_t u[W], o[W];
  dom_enter(s, u);
  dom_mul(u, o);
  dom_leave(o, y);
  y[0] += s[0] << 3;
}

// y = y0 + 2^22 y1 + 2^44 y2 + c  (y* < 2^32, c < 2^64)  ->  lazy u64
GL_HD uint64_t recombine(uint32_t y0, uint32_t y1, uint32_t y2, uint64_t c) {
  const gl::u128 acc = (gl::u128)c + y0 + ((uint64_t)y1 << 22) + ((gl::u128)y2 << 44);  // < 2^77: plain carry chains
  return fold_top((uint64_t)acc, (uint32_t)(acc >> 64));
}
GL_HD void split3(uint64_t v, uint32_t &a, uint32_t &b, uint32_t &c) {
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  a = lo & 0x3FFFFFu;
  b = ((lo >> 22) | (hi << 10)) & 0x3FFFFFu;
  c = hi >> 12;
}

// s <- MDS * s + next_rc   (next_rc_base < 0: no constant)
GL_HD void mds_layer(uint64_t (&s)[W], int next_rc_base) {
  uint32_t l0[W], l1[W], l2[W];
#pragma unroll
  for (int i = 0; i < W; i++) split3(s[i], l0[i], l1[i], l2[i]);
  uint32_t y0[W], y1[W], y2[W];
  mds_limb(l0, y0);
  mds_limb(l1, y1);
  mds_limb(l2, y2);
#pragma unroll
  for (int i = 0; i < W; i++)
    s[i] = recombine(y0[i], y1[i], y2[i], next_rc_base >= 0 ? rc(next_rc_base + i) : 0);
}

// Textbook round structure: 30 x (constants, S-box, MDS); state lazy, canonical on exit. Kept as the plain
// statement of the permutation (tests compare `permute` with it); the kernels use `permute` below.
GL_HD void permute_textbook(uint64_t (&s)[W]) {
#pragma unroll
  for (int i = 0; i < W; i++) s[i] = add_const_lazy(s[i], rc(i));
#pragma unroll 1
  for (int r = 0; r < HALF_FULL; r++) {
#pragma unroll
    for (int i = 0; i < W; i++) s[i] = sbox_lazy(s[i]);
    mds_layer(s, (r + 1) * W);
  }
#pragma unroll 1
  for (int r = HALF_FULL; r < HALF_FULL + PARTIAL; r++) {
    s[0] = sbox_lazy(s[0]);
    mds_layer(s, (r + 1) * W);
  }
#pragma unroll 1
  for (int r = HALF_FULL + PARTIAL; r < ROUNDS; r++) {
#pragma unroll
    for (int i = 0; i < W; i++) s[i] = sbox_lazy(s[i]);
    mds_layer(s, r + 1 < ROUNDS ? (r + 1) * W : -1);
  }
#pragma unroll
  for (int i = 0; i < W; i++) s[i] = gl::canon(s[i]);
}

// ---- the linear layers on TWO 32-bit limb planes in double precision -------------------------------------------------
// v_fma_f64 issues at the rate of the integer VOP3 forms (4.3 cycles per wave64, profiles/r01_ubench_valu.txt) and a double
// holds 53 bits exactly: a 32-bit limb has room for TWO layers of growth (2 x 8 bits) plus two fractional bits, so the MDS
// needs two planes instead of the three 22-bit integer planes of `mds_limb`, the products by +-2^k are single fused
// multiply-adds with the sign in the constant, and a carry normalisation is needed every second layer only. All arithmetic
// is exact (integers and quarter-integers below 2^53; multiplications by powers of two): no rounding ever happens, the
// result is bit-identical to the integer formulation (`permute_textbook` keeps that one; tests compare the two).
//
// Partial rounds in the transformed domain of the circulant. Only element 0 meets an S-box in a partial round; the other
// eleven go from one MDS straight into the next, and they need no round constants at all — those are pushed forward through
// the MDS offline. Between two layers T . T^-1' is only a scaling: if o = (E, F, v) are the products of one layer, the next
// layer's transformed input is T(y) = (4E, 4F, 2v). So the state never leaves the domain for all 22 rounds:
//   * the state is kept as W = (E, F, v), the products of the last layer, i.e. the transformed state divided by (4, 4, 2) —
//     the scaling T . T^-1' = diag(4, 4, 2) goes into the constants of the next layer's products (64, 64, 128 / 4, 32, 8 /
//     4, 8, 32, 2, 2, 2), and replacing element 0 by its S-box output adds (new - z) / 4 to aa0 and ab0 and (new - z) / 2 to b0:
//     exact quarter-integers;
//   * limb -> integer is (limb + 1.5 * 2^52), whose mantissa holds limb + 2^51 (the offsets are taken out of the constant
//     offline); carry extraction is (x + 1.5 * 2^84) - 1.5 * 2^84, the multiple of 2^32 nearest to x (balanced remainders);
//   * inside `partial_rounds` both planes are kept in UNITS OF 2^32, a limb l as l 2^-32: the carry is then rint(x), one
//     instruction, and limb -> integer is (x + 1.5 * 2^20), the same mantissa under another exponent (`renorm32_d`).
// Magnitudes in the units of the partial rounds, 2^32 (tests/test_hostsim.py replays them in units of 1, tests/test_renorm_units.py
// checks the normalisation in these): a normalised limb is within 2^-1 + 2^-12 of zero; a layer multiplies by at most 256 (aa),
// 44 (ab), 50 (b); element 0 is E0 + F0 + v0 < 350 x the layer's input; a limb entering the normalisation is below 2^17.3 and
// two layers after one every limb is below 2^16.6, with two fractional bits that now sit at 2^-33 and 2^-34 (2^-1, 2^-2 in units
// of 1) — 51 of the 53 bits — and the limb -> integer conversion is good to 2^19. Nothing grows: the scaling moves every
// exponent by -32 and no mantissa, the largest span between the top bit of a limb and its last fractional bit is 2^16.6 .. 2^-34,
// the 51 bits it was in units of 1 (2^48.6 .. 2^-2), and the smallest non-zero magnitude, 2^-34, is far from the subnormals.
// Index layout of a plane as before: [0..2] = aa, [3..5] = ab, [6..11] = b. SCALED: the input is W; else the transformed state.
#if defined(__FAST_MATH__) || defined(__FINITE_MATH_ONLY__) && __FINITE_MATH_ONLY__
#error "poseidon.h: the double-precision layers rely on IEEE semantics ((x + M) - M is a rounding, not x, and rint rounds to nearest, ties to even — the carry of renorm32_d): do not build with -ffast-math"
#endif
// OUT32: the products leave in units of 2^32 (every constant times 2^-32: only the exponents change) — the entry into `partial_rounds`
template <bool SCALED, bool OUT32 = false>
GL_HD void dom_mul_d(const double (&u)[W], double (&o)[W]) {
  constexpr double U = OUT32 ? 0x1p-32 : 1.0;
  constexpr double A = (SCALED ? 64.0 : 16.0) * U;
  const double t = (u[0] + u[1] + u[2]) * A;
  o[0] = __builtin_fma(u[2], A, t);
  o[1] = __builtin_fma(u[0], A, t);
  o[2] = __builtin_fma(u[1], A, t);
  constexpr double B1 = (SCALED ? 4.0 : 1.0) * U, B2 = (SCALED ? 8.0 : 2.0) * U, B8 = (SCALED ? 32.0 : 8.0) * U;
  o[3] = __builtin_fma(u[5], B8, __builtin_fma(u[3], -B1, u[4] * -B2));
  o[4] = __builtin_fma(u[3], -B8, __builtin_fma(u[4], -B1, u[5] * -B2));
  o[5] = __builtin_fma(u[3], B2, __builtin_fma(u[4], -B8, u[5] * -B1));
  constexpr double S = (SCALED ? 2.0 : 1.0) * U;
  constexpr double c[6][6] = {{2, 1, 1, -1, -16, 4},  {-4, 2, 1, 1, -1, -16}, {16, -4, 2, 1, 1, -1},
                              {1, 16, -4, 2, 1, 1},   {-1, 1, 16, -4, 2, 1},  {-1, -1, 1, 16, -4, 2}};
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double acc = u[6] * (S * c[k][0]);
#pragma unroll
    for (int i = 1; i < 6; i++) acc = __builtin_fma(u[6 + i], S * c[k][i], acc);
    o[6 + k] = acc;
  }
}
GL_HD void dom_enter_d(const double (&s)[W], double (&u)[W]) {
  double a[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    a[i] = s[i] + s[i + 6];
    u[6 + i] = s[i] - s[i + 6];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    u[i] = a[i] + a[i + 3];
    u[3 + i] = a[i] - a[i + 3];
  }
}
GL_HD void dom_leave_d(const double (&o)[W], double (&y)[W]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double p = o[i] + o[3 + i], q = o[i] - o[3 + i];
    y[i] = p + o[6 + i];
    y[i + 6] = p - o[6 + i];
    y[i + 3] = q + o[9 + i];
    y[i + 9] = q - o[9 + i];
  }
}
// value l + 2^32 h: both limbs to within 2^31 (+ the folded top) of zero, same value mod p
GL_HD void renorm_d(double &l, double &h) {
  constexpr double MAGIC = 0x1.8p84, INV = 0x1p-32;  // (x + MAGIC) - MAGIC: x rounded to a multiple of 2^32
  const double c = (l + MAGIC) - MAGIC;
  l -= c;
  h = __builtin_fma(c, INV, h);
  const double t = (h + MAGIC) - MAGIC;       // t / 2^32 units of 2^64 == 2^32 - 1:  h <- h - t + t / 2^32,  l <- l - t / 2^32
  h = __builtin_fma(t, -(1.0 - INV), h);      // one rounding of an exactly representable result (t (1 - 2^-32) is an integer < 2^51)
  l = __builtin_fma(t, -INV, l);
}
// The same on planes kept in units of 2^32 (L = l 2^-32, H = h 2^-32, exact: only the exponents differ): the multiple of 2^32 nearest
// to l is rint(L), ONE instruction (v_rndne_f64) where (x + MAGIC) - MAGIC is two — 6 operations per component instead of 8. Same
// carries, ties included (both round to nearest-even), so the same limbs as `renorm_d`, scaled.
GL_HD void renorm32_d(double &l, double &h) {
  constexpr double INV = 0x1p-32;
  const double c = __builtin_rint(l);
  l -= c;
  h = __builtin_fma(c, INV, h);
  const double t = __builtin_rint(h);
  h = __builtin_fma(t, -(1.0 - INV), h);
  l = __builtin_fma(t, -INV, l);
}
// the form the partial rounds are compiled with
GL_HD void renorm_planes_d(double &l, double &h) {
  if (UNITS32) renorm32_d(l, h); else renorm_d(l, h);
}
// integer limbs |l|, |h| < 2^51 - 2^32 -> lazy u64 congruent to l + 2^32 h + c, for the constant c that `m` encodes. The bit
// pattern of l + m.m0 is B + l + lo32(c') and that of h + m.m1 is B + h + hi32(c'), B = 0x433 * 2^52 + 2^51 being the pattern
// of 1.5 * 2^52 (exponent field included: nothing is masked) and c' = c - B (1 + 2^32): the two patterns are added as
// integers at their limb positions, and what overflows 2^64 (up to 2^31) is folded like any top word.
GL_HD uint64_t recombine_d(double l, double h, Magic m) {
  const uint64_t a0 = __builtin_bit_cast(uint64_t, l + m.m0), a1 = __builtin_bit_cast(uint64_t, h + m.m1);
  uint32_t w1;
  const uint32_t carry = __builtin_add_overflow(gl::hi32(a0), gl::lo32(a1), &w1);
  return fold_top(gl::pack(gl::lo32(a0), w1), gl::hi32(a1) + carry);
}
// The same with a SMALL top word, and the rare wrap of its fold left to the caller. In `recombine_d` the top word hi32(a1) + carry is
// Bhi + floor(x1 / 2^32) + carry with Bhi = B >> 32 (0x43380000; 0x41380000 for planes in units of 2^32) and x1 = h + hi32(c'): about
// 2^30 whatever the data, so `fold_top` wraps 2^64 every fourth time and pays a select and an add on every call. Here the literal
// T0 = Bhi - margin is taken off the top word as it is formed (two instructions as before), and the constants `m` come from the tables
// that have T0 2^64 == T0 (2^32 - 1) put back (POSEIDON_RCS / DOMS*_K / DOMS*_LAST with POSEIDON_TOP0_FULL / _PARTIAL / _PARTIAL32).
//   * top >= 0 for every reachable (l, h), negative limbs included. The bit pattern of 1.5 * 2^52 + x is the integer B + x for
//     -2^51 <= x < 2^51: the mantissa field holds 2^51 + x >= 0, the exponent field does not move. So a1 = B + x1 with the low word of B
//     zero, hi32(a1) = Bhi + floor(x1 / 2^32) (floor towards -infinity), and top = margin + floor(x1 / 2^32) + carry. A NEGATIVE h only
//     lowers that floor, to no less than -2^19 (h >= -2^51, hi32(c') >= 0), which the margin 2^19 of the partial rounds covers; in a
//     full-round layer h >= 0 and the margin is 0. The sign of l does not enter: hi32(a0) = Bhi + floor(x0 / 2^32) is added to lo32(a1)
//     mod 2^32 and its carry counted, so lo + 2^64 (hi32(a1) + carry) is a0 + 2^32 a1 exactly, whatever the signs.
//   * top <= 2^20: floor(x1 / 2^32) <= 2^19 - 1 for h < 2^51 - 2^32, plus the carry, plus the margin (gen_tables.top0_margin asserts it).
//   * one wrap suffices: lo + top (2^32 - 1) < 2^64 + 2^52, so a wrapped sum is below 2^52 and + EPS does not wrap it (gl::fold_top_open).
// The result is the one of `recombine_d` on the same value up to a multiple of p: another lazy representative of the same residue.
// `wrap` must go to gl::fold_repair with the result whenever it is non-zero (`repair_s`); a caller ORs several and tests once.
template <uint32_t T0>
GL_HD uint64_t recombine_s(double l, double h, Magic m, uint64_t &wrap) {
  const uint64_t a0 = __builtin_bit_cast(uint64_t, l + m.m0), a1 = __builtin_bit_cast(uint64_t, h + m.m1);
  // middle and top word in one 64-bit sum, d = a1 + hi32(a0) (no wrap: a1 < 2^63): hi32(d) is hi32(a1) + carry. As a multiply-add by 1
  // it is one instruction that leaves VCC alone, and the literal then rides a plain 32-bit add — an add with carry-in cannot take a
  // literal on gfx9 (one constant-bus read), and a register that holds it is one the leaf hash does not have.
#if GL_DEVICE_ASM
  uint64_t d, unused;
  asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=&v"(d), "=&s"(unused) : "v"(gl::hi32(a0)), "v"(a1));
#else
  const uint64_t d = a1 + gl::hi32(a0);
#endif
  return gl::fold_top_open(gl::pack(gl::lo32(a0), gl::lo32(d)), gl::hi32(d) - T0, wrap);
}
// A test build counts the repairs per site (0: a full-round layer, 1: one partial round, 2: the exit of the partial rounds).
#if !defined(POSEIDON_WRAP_PROBE)
#define POSEIDON_WRAP_PROBE(site) ((void)0)
#endif
// the rare path of N recombinations, behind ONE test of the union of their wraps (wave-uniform on the device: SGPR pairs)
template <int N>
GL_HD void repair_s(uint64_t *r, const uint64_t (&wrap)[N], int site) {
  uint64_t any = wrap[0];
#pragma unroll
  for (int i = 1; i < N; i++) any |= wrap[i];
  if (__builtin_expect(any != 0, 0)) {
    POSEIDON_WRAP_PROBE(site);
#pragma unroll
    for (int i = 0; i < N; i++) r[i] = gl::fold_repair(r[i], wrap[i]);
  }
}
// the N recombinations of a layer or an exit: all wraps ORed, one test (`c(i)`: the constant of word i; smaller groups: DESIGN.md §4.1 (8))
template <uint32_t T0, int N, typename Const>
GL_HD void recombine_all_s(const double (&yl)[N], const double (&yh)[N], Const c, uint64_t *r, int site) {
  uint64_t wrap[N];
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = recombine_s<T0>(yl[i], yh[i], c(i), wrap[i]);
  repair_s(r, wrap, site);
}

// the butterflies back for the live words only: y[0..3] = words 0..3 (digest) or words 8..11 (capacity)
GL_HD void dom_leave_digest_d(const double (&o)[W], double (&y)[4]) {
#pragma unroll
  for (int i = 0; i < 3; i++) y[i] = (o[i] + o[3 + i]) + o[6 + i];
  y[3] = (o[0] - o[3]) + o[9];
}
GL_HD void dom_leave_capacity_d(const double (&o)[W], double (&y)[4]) {
  y[0] = (o[2] + o[5]) - o[8];
#pragma unroll
  for (int i = 0; i < 3; i++) y[1 + i] = (o[i] - o[3 + i]) - o[9 + i];
}

// s <- MDS * s + next_rc on two double-precision limb planes (next_rc_base < 0: no constant)
GL_HD void mds_layer_d(uint64_t (&s)[W], int next_rc_base) {
  double ll[W], lh[W], u[W], o[W], yl[W], yh[W];
#pragma unroll
  for (int i = 0; i < W; i++) {
    ll[i] = (double)(uint32_t)s[i];
    lh[i] = (double)(uint32_t)(s[i] >> 32);
  }
  dom_enter_d(ll, u);
  dom_mul_d<false>(u, o);
  dom_leave_d(o, yl);
  yl[0] = __builtin_fma(ll[0], 8.0, yl[0]);
  dom_enter_d(lh, u);
  dom_mul_d<false>(u, o);
  dom_leave_d(o, yh);
  yh[0] = __builtin_fma(lh[0], 8.0, yh[0]);
  if (SMALL_TOP) {
    recombine_all_s<POSEIDON_TOP0_FULL>(yl, yh, [&](int i) { return rcs(next_rc_base >= 0 ? next_rc_base + i : ROUNDS * W); }, s, 0);
  } else {
#pragma unroll
    for (int i = 0; i < W; i++) s[i] = recombine_d(yl[i], yh[i], rcd(next_rc_base >= 0 ? next_rc_base + i : ROUNDS * W));
  }
}
// The permutation's LAST layer (no constant follows it) for a form that keeps four words: only those leave the domain and are
// recombined (the products nobody reads go with them). The dead words are cleared.
template <bool DIGEST>
GL_HD void mds_last_layer_d(uint64_t (&s)[W]) {
  double ll[W], lh[W], u[W], o[W], yl[4], yh[4];
#pragma unroll
  for (int i = 0; i < W; i++) {
    ll[i] = (double)(uint32_t)s[i];
    lh[i] = (double)(uint32_t)(s[i] >> 32);
  }
  dom_enter_d(ll, u);
  dom_mul_d<false>(u, o);
  if (DIGEST) {
    dom_leave_digest_d(o, yl);
    yl[0] = __builtin_fma(ll[0], 8.0, yl[0]);
  } else {
    dom_leave_capacity_d(o, yl);
  }
  dom_enter_d(lh, u);
  dom_mul_d<false>(u, o);
  if (DIGEST) {
    dom_leave_digest_d(o, yh);
    yh[0] = __builtin_fma(lh[0], 8.0, yh[0]);
  } else {
    dom_leave_capacity_d(o, yh);
  }
  uint64_t r[4];
  if (SMALL_TOP) {
    const Magic none = rcs(ROUNDS * W);
    recombine_all_s<POSEIDON_TOP0_FULL>(yl, yh, [&](int) { return none; }, r, 0);
  } else {
    const Magic none = rcd(ROUNDS * W);
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = recombine_d(yl[i], yh[i], none);
  }
#pragma unroll
  for (int i = 0; i < W; i++) s[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (DIGEST) s[i] = gl::canon(r[i]);
    else s[RATE + i] = r[i];
  }
}
// ---- the scaled layer two deep (partial_rounds): constants derived from dom_mul_d<true> at compile time ------------------------
template <int N> struct DomMat { double a[N][N]; };
template <int N> constexpr DomMat<N> dom_mat_sq(const DomMat<N> &m) {
  DomMat<N> r{};
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) {
      double acc = 0;
      for (int k = 0; k < N; k++) acc += m.a[i][k] * m.a[k][j];
      r.a[i][j] = acc;
    }
  return r;
}
// the blocks of the scaled layer K as matrices (rows: products, columns: inputs): aa = 64 (J + P), P: row i takes column (i + 2) % 3
constexpr DomMat<3> DOM_K_AB = {{{-4, -8, 32}, {-32, -4, -8}, {8, -32, -4}}};
constexpr DomMat<6> DOM_K_B = {{{4, 2, 2, -2, -32, 8}, {-8, 4, 2, 2, -2, -32}, {32, -8, 4, 2, 2, -2},
                                {2, 32, -8, 4, 2, 2}, {-2, 2, 32, -8, 4, 2}, {-2, -2, 2, 32, -8, 4}}};
constexpr DomMat<3> DOM_K_AB2 = dom_mat_sq(DOM_K_AB);
constexpr DomMat<6> DOM_K_B2 = dom_mat_sq(DOM_K_B);
// l K: element 0 of the NEXT layer read off this layer's inputs (rows 0, 3, 6 of K). The aa and ab parts are apart from the b part,
// which `partial_rounds` takes in another basis (`dom_next_z_b`, `dom_mul2_b` below): one copy of their constants.
GL_HD double dom_next_z_a(const double (&u)[W]) {
  constexpr double CZ[6] = {64, 64, 128, -4, -8, 32};
  double acc = u[0] * CZ[0];
#pragma unroll
  for (int k = 1; k < 6; k++) acc = __builtin_fma(u[k], CZ[k], acc);
  return acc;
}
GL_HD double dom_next_z(const double (&u)[W]) {
  double acc = dom_next_z_a(u);
#pragma unroll
  for (int k = 0; k < 6; k++) acc = __builtin_fma(u[6 + k], DOM_K_B.a[0][k], acc);
  return acc;
}
// o = K^2 u + d K t   (K t = columns 0 of the blocks of K over (4, 4, 2): a change d of element 0, one layer on)
GL_HD void dom_mul2_a(const double (&u)[W], double d, double (&o)[W]) {
  constexpr double KT[6] = {16, 32, 16, -1, -8, 2};
  // aa: (64 (J + P))^2 = 4096 (5 J + P^2), P^2: row i takes column (i + 1) % 3
  const double t = (u[0] + u[1] + u[2]) * 20480.0;
  o[0] = __builtin_fma(u[1], 4096.0, __builtin_fma(d, KT[0], t));
  o[1] = __builtin_fma(u[2], 4096.0, __builtin_fma(d, KT[1], t));
  o[2] = __builtin_fma(u[0], 4096.0, __builtin_fma(d, KT[2], t));
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double acc = d * KT[3 + k];
#pragma unroll
    for (int j = 0; j < 3; j++) acc = __builtin_fma(u[3 + j], DOM_K_AB2.a[k][j], acc);
    o[3 + k] = acc;
  }
}
GL_HD void dom_mul2_d(const double (&u)[W], double d, double (&o)[W]) {
  dom_mul2_a(u, d, o);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double acc = d * (DOM_K_B.a[k][0] / 2);
#pragma unroll
    for (int j = 0; j < 6; j++) acc = __builtin_fma(u[6 + j], DOM_K_B2.a[k][j], acc);
    o[6 + k] = acc;
  }
}

// ---- the b block in a basis where it is block-triangular (partial_rounds) ------------------------------------------------------------
// The b block is multiplication by a fixed polynomial in Z[x] / (x^6 + 1), and x^6 + 1 = (x^2 + 1)(x^4 - x^2 + 1). Reduction mod
// x^4 - x^2 + 1 (x^4 -> x^2 - 1, x^5 -> x^3 - x) is a ring map, so the four coordinates B = (u0 - u4, u1 - u5, u2 + u4, u3 + u5) of
// u mod (x^4 - x^2 + 1) are mapped among themselves. In the basis (B0, B1, B2, B3, u4, u5) = T u the layer is T K T^-1: integer
// entries (T and T^-1 are), rows 0..3 with a zero 4 x 2 corner — 28 non-zeros where the dense square has 36, and one more zero in
// K t. The planes stay in that basis from the entry of `partial_rounds` to its exit (`dom_b_to_tri`, `dom_b_from_tri`: four additions
// per plane each); the carry normalisation acts per component and commutes with any integer basis change up to multiples of p. What
// the rounds need in that basis: element 0 reads v0 = B0 + u4, so l = e0 + e3 + e6 + e10; a change of element 0 is d / 2 on v0, and
// T e0 = e0: it still lands on index 6 alone. Magnitudes: the absolute row sums of (T K T^-1)^2 are at most 3 420 and those of l K
// there 52 where the dense ones are 50, against 65 536 and 256 for the aa block, which stays the bound of every plane; B2 and B3 are
// sums of two old components, one more bit, only between the entry's products and the first normalisation and again at the exit,
// where u2 = B2 - u4 and u3 = B3 - u5 are differences of two b components (each below 2^-4 of an aa component).
// POSEIDON_BBLOCK_DENSE: the dense block in the old basis, kept for the A/B.
#if defined(POSEIDON_BBLOCK_DENSE)
constexpr bool B_TRI = false;
#else
constexpr bool B_TRI = true;
#endif
template <int N> constexpr DomMat<N> dom_mat_mul(const DomMat<N> &x, const DomMat<N> &y) {
  DomMat<N> r{};
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) {
      double acc = 0;
      for (int k = 0; k < N; k++) acc += x.a[i][k] * y.a[k][j];
      r.a[i][j] = acc;
    }
  return r;
}
template <int N> constexpr bool dom_mat_is_identity(const DomMat<N> &m) {
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++)
      if (m.a[i][j] != (i == j ? 1.0 : 0.0)) return false;
  return true;
}
constexpr DomMat<6> DOM_B_T = {{{1, 0, 0, 0, -1, 0}, {0, 1, 0, 0, 0, -1}, {0, 0, 1, 0, 1, 0}, {0, 0, 0, 1, 0, 1}, {0, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 0, 1}}};
constexpr DomMat<6> DOM_B_TINV = {{{1, 0, 0, 0, 1, 0}, {0, 1, 0, 0, 0, 1}, {0, 0, 1, 0, -1, 0}, {0, 0, 0, 1, 0, -1}, {0, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 0, 1}}};
static_assert(dom_mat_is_identity(dom_mat_mul(DOM_B_T, DOM_B_TINV)), "T^-1 is the inverse of T");
constexpr DomMat<6> DOM_K_BT = dom_mat_mul(dom_mat_mul(DOM_B_T, DOM_K_B), DOM_B_TINV);
constexpr DomMat<6> DOM_K_BT2 = dom_mat_sq(DOM_K_BT);
template <int N> constexpr bool dom_corner_is_zero(const DomMat<N> &m, int rows, int from) {
  for (int i = 0; i < rows; i++)
    for (int j = from; j < N; j++)
      if (m.a[i][j] != 0.0) return false;
  return true;
}
static_assert(dom_corner_is_zero(DOM_K_BT, 4, 4) && dom_corner_is_zero(DOM_K_BT2, 4, 4), "rows B0..B3 do not read u4, u5");
// what the rounds read of the b block in the basis they run in: the squared block, the b part of l K (row v0 = B0 + u4 of K) and the
// b part of K t (column v0 of K over 2: T e0 = e0)
struct DomVec6 { double a[6]; };
constexpr DomVec6 dom_b_next_z(bool tri) {
  DomVec6 r{};
  for (int j = 0; j < 6; j++) r.a[j] = tri ? DOM_K_BT.a[0][j] + DOM_K_BT.a[4][j] : DOM_K_B.a[0][j];
  return r;
}
constexpr DomVec6 dom_b_kt(bool tri) {
  DomVec6 r{};
  for (int i = 0; i < 6; i++) r.a[i] = (tri ? DOM_K_BT.a[i][0] : DOM_K_B.a[i][0]) / 2;
  return r;
}
constexpr DomMat<6> DOM_B2 = B_TRI ? DOM_K_BT2 : DOM_K_B2;
constexpr DomVec6 DOM_B_CZ = dom_b_next_z(B_TRI), DOM_B_KT = dom_b_kt(B_TRI);
// products in the old basis -> the basis of the rounds, and back (indices 6..11 of a plane)
GL_HD void dom_b_to_tri(double (&o)[W]) {
  o[6] -= o[10], o[7] -= o[11], o[8] += o[10], o[9] += o[11];
}
GL_HD void dom_b_from_tri(double (&o)[W]) {
  o[6] += o[10], o[7] += o[11], o[8] -= o[10], o[9] -= o[11];
}
// element 0 read off the products (l W), `dom_next_z` and `dom_mul2_d` with the b block in the basis of the rounds. A zero entry
// costs nothing: after unrolling, which terms exist is known at compile time (the dense form issues what `dom_mul2_d` issues).
GL_HD double dom_read_z(const double (&w)[W]) {
  const double z = w[0] + w[3] + w[6];
  return B_TRI ? z + w[10] : z;
}
GL_HD double dom_next_z_b(const double (&u)[W]) {
  double acc = dom_next_z_a(u);
#pragma unroll
  for (int k = 0; k < 6; k++) acc = __builtin_fma(u[6 + k], DOM_B_CZ.a[k], acc);
  return acc;
}
GL_HD void dom_mul2_b(const double (&u)[W], double d, double (&o)[W]) {
  dom_mul2_a(u, d, o);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double acc = 0;
    bool first = true;
    if (DOM_B_KT.a[k] != 0.0) acc = d * DOM_B_KT.a[k], first = false;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      if (DOM_B2.a[k][j] == 0.0) continue;
      acc = first ? u[6 + j] * DOM_B2.a[k][j] : __builtin_fma(u[6 + j], DOM_B2.a[k][j], acc);
      first = false;
    }
    o[6 + k] = acc;
  }
}

// The 22 partial rounds with the MDS layers on either side of them. s in: the S-box OUTPUTS of the last full round before
// them (round 3); s out: the state entering the S-boxes of the first full round after them (round 26), constants included.
// `input(i, x)` sees the S-box input x (lazy u64) of partial round i on element 0 and returns what goes into the S-box — x
// itself for the permutation; the PoseidonGate constrains x against a wire and continues with the wire. `stop` as below.
template <typename Input, typename Stop>
GL_HD bool partial_rounds(uint64_t (&s)[W], Input input, Stop stop) {
  // straight into the domain (no constants: all pushed forward)
  double wl[W], wh[W], ol[W], oh[W];
  double nl, nh;  // limbs of the latest S-box output on element 0
  {
    double ll[W], lh[W];
#pragma unroll
    for (int k = 0; k < W; k++) {
      ll[k] = (double)(uint32_t)s[k];
      lh[k] = (double)(uint32_t)(s[k] >> 32);
    }
    nl = ll[0], nh = lh[0];
    dom_enter_d(ll, wl);
    dom_enter_d(lh, wh);
    dom_mul_d<false, UNITS32>(wl, ol);
    dom_mul_d<false, UNITS32>(wh, oh);
  }
  // From here to the exit the planes are in units of 2^32 (UNITS32; U = 1 restores units of 1). Every operation multiplies by a
  // compile-time constant or adds two planes, so the unit costs nothing: only where a limb of an S-box output (nl, nh: units of 1)
  // meets a plane does its factor carry U, and the recombination gets the constants of that unit (`doms_k` / `doms_last`; `recombine_d`: DDK_HOST / DDLAST_HOST).
  constexpr double U = UNITS32 ? 0x1p-32 : 1.0;
  // TWO partial rounds per trip, with ONE application of the layer squared. Let W = (E, F, v) be the products at the top of round r,
  // K the scaled layer (dom_mul_d<true>), t = (1/4, 0, 0 | 1/4, 0, 0 | 1/2, 0, ...) what a change of element 0 is in the domain and
  // l = e_0 + e_3 + e_6 the functional that reads element 0 off the products. Round r: z = l W, S-box, W' = W + (new - z) t. Round r + 1
  // needs only ELEMENT 0 of the next layer — z' = l K W' = <CZ, W'>, twelve multiply-adds instead of the 51 operations of the whole
  // layer — and then W'' = K (K W' + (new' - z') t) = K^2 W' + (new' - z') K t: the squared layer costs what one layer costs (its
  // blocks are dense already: 6 + 9 + 36), so a trip is 12 + 51 + 12 operations per plane where two layers were 102. K^2 grows a limb
  // by at most 2^16 (aa: 4096 (5 J + P^2), rows sum to 2^16), which is the two layers of growth a limb was normalised for anyway:
  // one renorm per trip as before, now in front of the squared layer. Magnitudes (tests/test_hostsim.py replays them): W at the top of
  // a trip is below 2^47.3 with no fractional bits, z below 2^48.9.
#if defined(POSEIDON_PARTIAL_V1)  // one layer per round (rounds 2-3 of the build): kept for the A/B in tools/ubench_poseidon_variants.hip
  // one partial round: read element 0 off the products (a), S-box it, put it back (W = (E, F, v) + (new - z) / (4, 4, 2) on
  // aa0, ab0, b0, in place), optionally normalise, next products (a -> b). Two rounds per trip, ping-pong, so nothing is copied.
  auto round = [&](int i, double (&al)[W], double (&ah)[W], double (&bl)[W], double (&bh)[W], bool normalise) {
    const double zl = al[0] + al[3] + al[6], zh = ah[0] + ah[3] + ah[6];
    // element 0 of the state: E0 + F0 + v0 + the diagonal 8 of the MDS on the previous S-box output
    const uint64_t x = sbox_lazy_chain(input(i, recombine_d(__builtin_fma(nl, 8.0 * U, zl), __builtin_fma(nh, 8.0 * U, zh), domd_k(i))));
    nl = (double)(uint32_t)x;
    nh = (double)(uint32_t)(x >> 32);
    const double dl = __builtin_fma(nl, U, -zl), dh = __builtin_fma(nh, U, -zh);
    al[0] = __builtin_fma(dl, 0.25, al[0]), ah[0] = __builtin_fma(dh, 0.25, ah[0]);
    al[3] = __builtin_fma(dl, 0.25, al[3]), ah[3] = __builtin_fma(dh, 0.25, ah[3]);
    al[6] = __builtin_fma(dl, 0.5, al[6]), ah[6] = __builtin_fma(dh, 0.5, ah[6]);
    if (normalise) {
#pragma unroll
      for (int k = 0; k < W; k++) renorm_planes_d(al[k], ah[k]);
    }
    dom_mul_d<true>(al, bl);
    dom_mul_d<true>(ah, bh);
  };
  static_assert(PARTIAL % 2 == 0, "two rounds per trip");
#pragma unroll 1
  for (int i = 0; i < PARTIAL; i += 2) {
    if ((i & 3) == 0 && stop()) return false;
    round(i, ol, oh, wl, wh, false);
    round(i + 1, wl, wh, ol, oh, true);  // a limb holds two layers of growth: normalise every second round
  }
  // leave the domain: natural limbs, + what is pending of the constants
  double yl[W], yh[W];
  dom_leave_d(ol, yl);
  dom_leave_d(oh, yh);
  yl[0] = __builtin_fma(nl, 8.0 * U, yl[0]), yh[0] = __builtin_fma(nh, 8.0 * U, yh[0]);
#pragma unroll
  for (int k = 0; k < W; k++) s[k] = recombine_d(yl[k], yh[k], domd_last(k));
#else
  // The b block of both planes lives in the basis (B0..B3, u4, u5) from here to the exit (B_TRI; see `dom_b_to_tri`).
  if (B_TRI) dom_b_to_tri(ol), dom_b_to_tri(oh);
  // element 0 of a round from its limbs: `recombine_s` with its own test of the rare wrap (SMALL_TOP), else `recombine_d`
  auto element0 = [&](int i, double l, double h) -> uint64_t {
    if (!SMALL_TOP) return recombine_d(l, h, domd_k(i));
    uint64_t r[1], wrap[1];
    r[0] = recombine_s<TOP0_PLANES>(l, h, doms_k(i), wrap[0]);
    repair_s(r, wrap, 1);
    return r[0];
  };
  auto trip = [&](int i, double (&al)[W], double (&ah)[W], double (&bl)[W], double (&bh)[W]) {
    // round i: element 0 = E0 + F0 + v0 + the diagonal 8 of the MDS on the previous S-box output
    {
      const double zl = dom_read_z(al), zh = dom_read_z(ah);
      const uint64_t x = sbox_lazy_chain(input(i, element0(i, __builtin_fma(nl, 8.0 * U, zl), __builtin_fma(nh, 8.0 * U, zh))));
      nl = (double)(uint32_t)x;
      nh = (double)(uint32_t)(x >> 32);
      const double dl = __builtin_fma(nl, U, -zl), dh = __builtin_fma(nh, U, -zh);
      al[0] = __builtin_fma(dl, 0.25, al[0]), ah[0] = __builtin_fma(dh, 0.25, ah[0]);
      al[3] = __builtin_fma(dl, 0.25, al[3]), ah[3] = __builtin_fma(dh, 0.25, ah[3]);
      al[6] = __builtin_fma(dl, 0.5, al[6]), ah[6] = __builtin_fma(dh, 0.5, ah[6]);
    }
#pragma unroll
    for (int k = 0; k < W; k++) renorm_planes_d(al[k], ah[k]);
    // round i + 1: element 0 one layer ahead, then the squared layer with the change of element 0 carried one layer on (a -> b)
    const double zl = dom_next_z_b(al), zh = dom_next_z_b(ah);
    const uint64_t x = sbox_lazy_chain(input(i + 1, element0(i + 1, __builtin_fma(nl, 8.0 * U, zl), __builtin_fma(nh, 8.0 * U, zh))));
    nl = (double)(uint32_t)x;
    nh = (double)(uint32_t)(x >> 32);
    dom_mul2_b(al, __builtin_fma(nl, U, -zl), bl);
#if defined(__HIP_DEVICE_COMPILE__) && !defined(POSEIDON_INTERLEAVE_PLANES)  // the macro: A/B in tools/ubench_leaf_residency.hip
    __builtin_amdgcn_sched_barrier(0);  // one plane after the other: interleaved, the four arrays are live at once and the leaf hash (96 registers) spills
#endif
    dom_mul2_b(ah, __builtin_fma(nh, U, -zh), bh);
  };
  static_assert(PARTIAL % 4 == 2, "five double trips (ping-pong, nothing is copied) and a last single one");
#pragma unroll 1
  for (int i = 0; i + 4 <= PARTIAL; i += 4) {
    if (stop()) return false;
    trip(i, ol, oh, wl, wh);
    trip(i + 2, wl, wh, ol, oh);
  }
  trip(PARTIAL - 2, ol, oh, wl, wh);
  // leave the domain: natural limbs, + what is pending of the constants
  double yl[W], yh[W];
  if (B_TRI) dom_b_from_tri(wl), dom_b_from_tri(wh);
  dom_leave_d(wl, yl);
  dom_leave_d(wh, yh);
  yl[0] = __builtin_fma(nl, 8.0 * U, yl[0]), yh[0] = __builtin_fma(nh, 8.0 * U, yh[0]);
  if (SMALL_TOP) {
    recombine_all_s<TOP0_PLANES>(yl, yh, [&](int k) { return doms_last(k); }, s, 2);
  } else {
#pragma unroll
    for (int k = 0; k < W; k++) s[k] = recombine_d(yl[k], yh[k], domd_last(k));
  }
#endif
  return true;
}
struct SameInput {
  GL_HD uint64_t operator()(int, uint64_t x) const { return x; }
};

// `stop` is polled between rounds (every full round, every fourth partial round); when it answers true the permutation is
// abandoned and false returned. It must answer the same for every lane of a wave. The proof-of-work search uses it to drop
// candidates that can no longer be the smallest witness.
template <int OUT = OUT_ALL, bool ZERO_CAP = false, typename Stop>
GL_HD bool permute_until(uint64_t (&s)[W], Stop stop) {
  static_assert(OUT == OUT_ALL || OUT == OUT_CAPACITY || OUT == OUT_DIGEST, "unknown output form");
#pragma unroll
  for (int i = 0; i < RATE; i++) s[i] = add_const_lazy(s[i], rc(i));
#pragma unroll
  for (int i = RATE; i < W; i++) s[i] = ZERO_CAP ? POSEIDON_CAP0_SBOX[i - RATE] : add_const_lazy(s[i], rc(i));  // round 0 of a zero word: done offline
#pragma unroll 1
  for (int r = 0; r < HALF_FULL - 1; r++) {
    if (stop()) return false;
#pragma unroll
    for (int i = 0; i < RATE; i += 2) sbox_lazy2(s[i], s[i + 1]);
    if (r > 0 || !ZERO_CAP) {
#pragma unroll
      for (int i = RATE; i < W; i += 2) sbox_lazy2(s[i], s[i + 1]);
    }
    mds_layer_d(s, (r + 1) * W);
  }
#pragma unroll
  for (int k = 0; k < W; k += 2) sbox_lazy2(s[k], s[k + 1]);  // the last full round before the partial rounds
  if (!partial_rounds(s, SameInput(), stop)) return false;
  // a form that drops outputs has its last round apart from the loop (its layer is another one); OUT_ALL keeps the loop whole
  constexpr int LOOPED = OUT == OUT_ALL ? ROUNDS : ROUNDS - 1;
#pragma unroll 1
  for (int r = HALF_FULL + PARTIAL; r < LOOPED; r++) {
    if (stop()) return false;
#pragma unroll
    for (int i = 0; i < W; i += 2) sbox_lazy2(s[i], s[i + 1]);
    mds_layer_d(s, r + 1 < ROUNDS ? (r + 1) * W : -1);
  }
  if (OUT == OUT_ALL) {
#pragma unroll
    for (int i = 0; i < W; i++) s[i] = gl::canon(s[i]);
  } else {
    if (stop()) return false;
#pragma unroll
    for (int i = 0; i < W; i += 2) sbox_lazy2(s[i], s[i + 1]);
    mds_last_layer_d<OUT == OUT_DIGEST>(s);
  }
  return true;
}

struct NeverStop {
  GL_HD bool operator()() const { return false; }
};
GL_HD void permute(uint64_t (&s)[W]) { permute_until(s, NeverStop()); }
// the only permutation of a tree node (two_to_one): zero capacity in, digest out
GL_HD void permute_node(uint64_t (&s)[W]) { permute_until<OUT_DIGEST, true>(s, NeverStop()); }
// of a sponge chain: a permutation whose rate words the next chunk overwrites whole; the last one
GL_HD void permute_absorb(uint64_t (&s)[W]) { permute_until<OUT_CAPACITY, false>(s, NeverStop()); }
GL_HD void permute_squeeze(uint64_t (&s)[W]) { permute_until<OUT_DIGEST, false>(s, NeverStop()); }
// What HOST code hashes with (the transcript of a small batch, the verifier, public-input hashes): the integer round structure.
// On an x86 core it takes 1.8 us per permutation; `permute`, whose double-precision layers are shaped for the GPU's issue
// rates, takes 5.7 us there. Same function, bit for bit (tests compare the two over 600 M chained permutations).
inline void permute_host(uint64_t (&s)[W]) { permute_textbook(s); }

}  // namespace poseidon
