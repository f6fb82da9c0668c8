// Goldilocks field arithmetic for gfx950 device code (and host code: every function is
// __host__ __device__ so the C++ host side of the prover uses the same definitions).
//
// p = 2^64 - 2^32 + 1. Elements are canonical u64 in [0, p) at every kernel boundary
// (the wire format of plonky2's GoldilocksField); inside a kernel
// values may be carried "lazily" as any u64 congruent to the value.
//
// CDNA4 has no 64x64->128 multiply: the product is built from v_mad_u64_u32 and the
// reduction uses 2^64 == 2^32-1 and 2^96 == -1 (mod p).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GL_HD __host__ __device__ __forceinline__
// device code takes the hand-scheduled `asm` forms below; GL_PORTABLE (experiments: tools/ubench_leaf_latency.hip) builds the
// portable C forms for the device too
#if defined(__HIP_DEVICE_COMPILE__) && !defined(GL_PORTABLE)
#define GL_DEVICE_ASM 1
#else
#define GL_DEVICE_ASM 0
#endif

namespace gl {

constexpr uint64_t P = 0xFFFFFFFF00000001ULL;
constexpr uint64_t EPS = 0xFFFFFFFFULL;  // 2^64 mod p

// x - p == x + EPS (mod 2^64): one 64-bit compare, one select, one 64-bit add (v_lshl_add_u64) on gfx950
GL_HD uint64_t canon(uint64_t x) { return x + (x >= P ? EPS : 0); }

GL_HD uint32_t lo32(uint64_t x) { return (uint32_t)x; }
GL_HD uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
GL_HD uint64_t pack(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// The helpers below are phrased through unsigned __int128 so that LLVM legalises them into plain
// v_sub_co/v_subb_co (v_add_co/v_addc_co) carry chains: 5 instructions per modular subtraction,
// 7 per addition, no 64-bit compares/selects.
typedef unsigned __int128 u128;

// a, b canonical -> canonical.  a - b, plus p when it borrowed (p == -EPS mod 2^64)
GL_HD uint64_t sub(uint64_t a, uint64_t b) {
  u128 d = (u128)a - b;
  uint64_t borrowed = (uint64_t)(d >> 64);  // 0 or all ones
  return (uint64_t)d - (borrowed & EPS);
}
GL_HD uint64_t neg(uint64_t a) { return a ? P - a : 0; }
// a, b canonical -> canonical, five instructions on gfx950 (one v_lshl_add_u64, two 64-bit compares, a select, one more add; as
// a - (p - b) through carry chains it was seven). s = a + b mod 2^64. If it wrapped, the true sum is s + 2^64 == s + EPS, which
// cannot wrap again (s <= 2p - 2 - 2^64) and is below p; if it did not wrap but s >= p, then s - p == s + EPS (mod 2^64): both
// repairs add EPS.
GL_HD uint64_t add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s + (((s < a) | (s >= P)) ? EPS : 0);
}

// lazy add: a any u64, b any u64 -> u64 congruent to a+b (not canonical)
GL_HD uint64_t add_lazy(uint64_t a, uint64_t b) {
  uint64_t s = a + b;
  if (s < a) {          // wrapped: + 2^64 == + EPS
    s += EPS;
    if (s < EPS) s += EPS;
  }
  return s;
}

// A modular multiplication is 11 VALU instructions on gfx950: 4 v_mad_u64_u32 for the product (+ 2 moves), 2 for the borrow
// chain `lo - w3`, one more multiply-add for `+ w2 (2^32 - 1)` (+ select, 64-bit add). Three pieces are written as `asm`
// because carry-outs are out of the compiler's reach (it zero-extends, adds and compares instead: 19 instructions; the
// permutation measures 2.06 -> 2.48 -> 2.62 G/s with them, tools/ubench_poseidon_variants.hip).
//
// The carry-out `cy` of the third multiply-add (`mul_wide_cy`) has weight 2^96 == -1: it is a unit to subtract, and it never
// becomes a VGPR. It stays in the SGPR pair the multiply-add wrote and enters the borrow chain of the reduction as the
// carry-in of its first subtract (`reduce128_lazy(lo, hi', cy)`), where hi' is the high half WITHOUT that carry. What makes
// this sound, with a = a1 2^32 + a0, b likewise, r = a1 b0 + p01 mod 2^64 and hi' = a1 b1 + hi32(r):
//   1. hi' cannot carry: a1 b1 + hi32(r) <= (2^32 - 1)^2 + 2^32 - 1 = 2^64 - 2^32. The true high half is hi = hi' + cy 2^32.
//   2. hi32(hi') + cy <= 2^32 - 1: adding cy 2^32 to hi' does not touch its low word, so hi32(hi') + cy = hi32(hi), and
//      hi <= 2^64 - 2 because a b <= (2^64 - 1)^2. `mul_add_lazy` adds the carry of lo + c to hi' first: a b + c <=
//      (2^64 - 1) 2^64 keeps hi + 1 <= 2^64 - 1, so hi' + 1 cannot carry either and hi32(hi' + 1) + cy = hi32(hi + 1) <=
//      2^32 - 1. The chain therefore subtracts exactly the old w3 = hi32(hi), and borrows for exactly the same operands
//      (lo < w3) as the two-argument form.
//   3. the repaired t0 cannot underflow: a borrow means lo < w3 <= 2^32 - 1, so t0 = lo - w3 + 2^64 >= 2^64 - 2^32 + 1 > EPS.
//   4. the fold cannot wrap twice: t0 + w2 (2^32 - 1) < 2^65 - 2^33, so after one wrap (+ EPS) it is below 2^64 - 2^33.
//
// The `s_nop 1` are the two wait states gfx950 needs between a VALU write of an SGPR and a VALU read of it; the compiler's
// hazard recogniser does not look inside `asm`, so every statement that reads such an SGPR (`cy` comes from ANOTHER
// statement) carries its own wait states in front of the read. tests/test_gpu_parity.py drives `cp_field_mul` through every
// carry / borrow corner on the device, tests/test_gpu_product_chain.py every class of (cy, borrow, fold wrap).

// lo + top * (2^32 - 1) as a lazy u64 (top * 2^64 == top * (2^32 - 1))
GL_HD uint64_t fold_top(uint64_t lo, uint32_t top) {
#if GL_DEVICE_ASM
  // one multiply-add; its carry-out (one wrap of 2^64 == + EPS) selects the repair. The repaired sum cannot wrap again:
  // lo + top (2^32 - 1) < 2^65 - 2^33, so after one wrap it is below 2^64 - 2^33.
  uint64_t r, cy;
  uint32_t m;
  asm("v_mad_u64_u32 %0, %1, %3, -1, %4\n\ts_nop 1\n\tv_cndmask_b32 %2, 0, -1, %1" : "=&v"(r), "=&s"(cy), "=v"(m) : "v"(top), "v"(lo));
  return r + m;
#else
  const u128 s = (u128)lo + (((uint64_t)top << 32) - top);
  return (uint64_t)s + ((0 - (uint64_t)(s >> 64)) & EPS);
#endif
}

// The same fold for a caller that knows its top word SMALL (top <= 2^20: poseidon.h `recombine_s`), in two halves. The sum wraps 2^64
// only when the 64 - 20 - 32 = 12 high bits of `lo` are all ones, so the repair is taken out of the stream: `fold_top_open` is the
// multiply-add alone — it returns the sum mod 2^64 and leaves the wrap in `wrap` (device: the SGPR pair the instruction wrote its
// carry-out to, one bit per lane; host: 0 or 1) — and the caller ORs the wraps of as many folds as it likes on the scalar side, tests
// the union once and, behind that wave-uniform branch, hands every sum and its own wrap to `fold_repair` (+ EPS where the bit is
// set, nothing where it is not). One wrap suffices: lo + top (2^32 - 1) < 2^64 + 2^52, so a wrapped sum is below 2^52 and + EPS
// cannot wrap it again. fold_repair(fold_top_open(lo, top, w), w) == fold_top(lo, top), bit for bit.
GL_HD uint64_t fold_top_open(uint64_t lo, uint32_t top, uint64_t &wrap) {
#if GL_DEVICE_ASM
  uint64_t r;
  asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=&v"(r), "=&s"(wrap) : "v"(top), "v"(lo));
  return r;
#else
  const u128 s = (u128)lo + (((uint64_t)top << 32) - top);
  wrap = (uint64_t)(s >> 64);
  return (uint64_t)s;
#endif
}
GL_HD uint64_t fold_repair(uint64_t r, uint64_t wrap) {
#if GL_DEVICE_ASM
  // `wrap` was written by a VALU instruction of another statement: the two wait states in front of the read (see above)
  uint32_t m;
  asm volatile("s_nop 1\n\tv_cndmask_b32 %0, 0, -1, %1" : "=v"(m) : "s"(wrap));
  return r + m;
#else
  return r + ((0 - wrap) & EPS);
#endif
}

// 128-bit (hi:lo) -> lazy u64 (any representative):  lo - hi_hi + hi_lo*(2^32-1),
// every wrap of 2^64 repaid by -+EPS
GL_HD uint64_t reduce128_lazy(uint64_t lo, uint64_t hi) {
  const uint32_t w2 = lo32(hi), w3 = hi32(hi);
#if GL_DEVICE_ASM
  // lo - w3 borrows only when lo < w3 < 2^32 (a 2^-32 event for a product): the repair (- EPS for the 2^64 that was lent)
  // sits behind a wave-uniform branch instead of costing three instructions on every multiplication
  uint32_t tl, th, m;
  uint64_t bm;
  asm("v_sub_co_u32_e64 %0, %2, %3, %4\n\ts_nop 1\n\tv_subbrev_co_u32_e64 %1, %2, 0, %5, %2"
      : "=&v"(tl), "=&v"(th), "=&s"(bm)
      : "v"(lo32(lo)), "v"(w3), "v"(hi32(lo)));
  uint64_t t0 = pack(tl, th);
  if (__builtin_expect(bm != 0, 0)) {
    asm volatile("v_cndmask_b32 %0, 0, -1, %1" : "=v"(m) : "s"(bm));
    t0 -= m;
  }
#else
  const u128 t = (u128)lo - w3;
  const uint64_t t0 = (uint64_t)t - ((uint64_t)(t >> 64) & EPS);
#endif
  return fold_top(t0, w2);
}
GL_HD uint64_t reduce128(uint64_t lo, uint64_t hi) { return canon(reduce128_lazy(lo, hi)); }

// 64x64 -> 128 as exactly four 32x32+64 multiply-adds (v_mad_u64_u32): the true 128-bit value, for callers that go on adding
// to it (poseidon_coop.h's dot product); a modular product takes `mul_wide_cy` below
GL_HD void mul_wide(uint64_t a, uint64_t b, uint64_t &lo, uint64_t &hi) {
  const uint32_t a0 = lo32(a), a1 = hi32(a), b0 = lo32(b), b1 = hi32(b);
  const uint64_t p00 = (uint64_t)a0 * b0;
  const uint64_t p01 = (uint64_t)a0 * b1 + (p00 >> 32);  // < 2^64
#if GL_DEVICE_ASM
  // the third multiply-add takes the whole second one as its addend; its carry-out replaces two zero-extending moves
  // and a 64-bit addition
  uint64_t r, cr;
  uint32_t cbit;
  asm("v_mad_u64_u32 %0, %1, %3, %4, %5\n\ts_nop 1\n\tv_cndmask_b32 %2, 0, 1, %1"
      : "=&v"(r), "=&s"(cr), "=&v"(cbit)
      : "v"(a1), "v"(b0), "v"(p01));
  lo = pack(lo32(p00), lo32(r));
  hi = (uint64_t)a1 * b1 + pack(hi32(r), cbit);
#else
  (void)p01;
  const u128 p = (u128)a * b;  // the host has the instruction
  lo = (uint64_t)p;
  hi = (uint64_t)(p >> 64);
#endif
}

// The carry-aware pair (see the comment above `fold_top`). `carry_t` is the carry-out of the product's third multiply-add:
// on the device the SGPR pair that instruction wrote (one bit per lane), only ever handed from `mul_wide_cy` to
// `reduce128_lazy`; in the portable form `hi` is the true high half and the carry is 0.
typedef uint64_t carry_t;

// a * b = lo + (hi + cy 2^32) 2^64
GL_HD void mul_wide_cy(uint64_t a, uint64_t b, uint64_t &lo, uint64_t &hi, carry_t &cy) {
#if GL_DEVICE_ASM
  const uint32_t a0 = lo32(a), a1 = hi32(a), b0 = lo32(b), b1 = hi32(b);
  const uint64_t p00 = (uint64_t)a0 * b0;
  const uint64_t p01 = (uint64_t)a0 * b1 + (p00 >> 32);  // < 2^64
  uint64_t r;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=&v"(r), "=&s"(cy) : "v"(a1), "v"(b0), "v"(p01));
  lo = pack(lo32(p00), lo32(r));
  hi = (uint64_t)a1 * b1 + (uint64_t)hi32(r);  // (1): no carry
#else
  mul_wide(a, b, lo, hi);
  cy = 0;
#endif
}

// (lo, hi', cy) -> lazy u64: lo - (hi32(hi') + cy) + lo32(hi') (2^32 - 1), every wrap of 2^64 repaid by -+EPS
GL_HD uint64_t reduce128_lazy(uint64_t lo, uint64_t hi, carry_t cy) {
#if GL_DEVICE_ASM
  // `cy` is the carry-in of the low-word subtract (2); the rare borrow (lo < w3) keeps its wave-uniform branch (3)
  uint32_t tl, th, m;
  uint64_t bm;
  asm("s_nop 1\n\tv_subb_co_u32_e64 %0, %2, %3, %4, %6\n\ts_nop 1\n\tv_subbrev_co_u32_e64 %1, %2, 0, %5, %2"
      : "=&v"(tl), "=&v"(th), "=&s"(bm)
      : "v"(lo32(lo)), "v"(hi32(hi)), "v"(hi32(lo)), "s"(cy));
  uint64_t t0 = pack(tl, th);
  if (__builtin_expect(bm != 0, 0)) {
    asm volatile("v_cndmask_b32 %0, 0, -1, %1" : "=v"(m) : "s"(bm));
    t0 -= m;
  }
  return fold_top(t0, lo32(hi));
#else
  (void)cy;
  return reduce128_lazy(lo, hi);
#endif
}
GL_HD uint64_t reduce128(uint64_t lo, uint64_t hi, carry_t cy) { return canon(reduce128_lazy(lo, hi, cy)); }

// a*b as a lazy u64; a, b may be lazy themselves
GL_HD uint64_t mul_lazy(uint64_t a, uint64_t b) {
  uint64_t lo, hi;
  carry_t cy;
  mul_wide_cy(a, b, lo, hi, cy);
  return reduce128_lazy(lo, hi, cy);
}
// Two independent products in one go: r0 == a0 b0, r1 == a1 b1, any u64 in, lazy u64 out; each is the arithmetic of `mul_lazy`, bit
// for bit. What the pair buys is scheduling, not instructions (2 x 11 VALU as before). A lone `mul_lazy` is three basic blocks (its
// rare-borrow branch) and carries three `s_nop 1` in front of dependent instructions, so one wave's own stream — a SIMD that holds one
// or two waves — stalls on every product. Here the two chains are issued alternately, so that each VALU write of an SGPR (cy, the
// low-word borrow, the 64-bit borrow, the fold's carry-out) has its sibling's instruction as the first of the two wait states gfx950
// needs before a VALU reads that SGPR (counted as LLVM's hazard recogniser counts: one per intervening instruction), and an `s_nop 0`
// where a second one is missing; the two borrow masks are ORed on the scalar side and tested ONCE, and both chains are repaired behind
// that single rare, wave-uniform branch (`v_cndmask` on a zero mask selects 0: the chain that did not borrow is left as it is, notes
// (1)-(4) above `fold_top` hold per chain). Per pair: one branch instead of two, 4 wait states of `s_nop` instead of 12.
GL_HD void mul_lazy2(uint64_t a0, uint64_t b0, uint64_t a1, uint64_t b1, uint64_t &r0, uint64_t &r1) {
#if GL_DEVICE_ASM
  const uint32_t al = lo32(a0), ah = hi32(a0), bl = lo32(b0), bh = hi32(b0);
  const uint32_t cl = lo32(a1), ch = hi32(a1), dl = lo32(b1), dh = hi32(b1);
  const uint64_t p00 = (uint64_t)al * bl, q00 = (uint64_t)cl * dl;
  const uint64_t p01 = (uint64_t)al * bh + (p00 >> 32), q01 = (uint64_t)cl * dh + (q00 >> 32);  // < 2^64
  // the third multiply-adds; their carry-outs stay in SGPR pairs (`mul_wide_cy`)
  uint64_t rA, rB;
  carry_t cyA, cyB;
  asm("v_mad_u64_u32 %0, %1, %4, %5, %6\n\tv_mad_u64_u32 %2, %3, %7, %8, %9"
      : "=&v"(rA), "=&s"(cyA), "=&v"(rB), "=&s"(cyB)
      : "v"(ah), "v"(bl), "v"(p01), "v"(ch), "v"(dl), "v"(q01));
  const uint64_t loA = pack(lo32(p00), lo32(rA)), loB = pack(lo32(q00), lo32(rB));
  const uint64_t hiA = (uint64_t)ah * bh + (uint64_t)hi32(rA), hiB = (uint64_t)ch * dh + (uint64_t)hi32(rB);  // (1): no carry
  // the borrow chains lo - (hi32(hi') + cy). Wait states:
  //   cyA, cyB come from the statement above, out of the recogniser's sight: the `s_nop 1` in front pads both reads in full;
  //   low-word borrow of A (%4): written by the 1st subtract, read by the 3rd: the 2nd subtract (chain B) + `s_nop 0`;
  //   low-word borrow of B (%5): written by the 2nd subtract, read by the 4th: `s_nop 0` + the 3rd subtract (chain A);
  //   the 64-bit borrows are read next by `s_or_b64` (SALU: no wait states) and, behind the branch, by the repair below.
  uint32_t tlA, thA, tlB, thB;
  uint64_t bA, bB, bm;
  asm("s_nop 1\n\t"
      "v_subb_co_u32_e64 %0, %4, %7, %8, %10\n\t"
      "v_subb_co_u32_e64 %2, %5, %11, %12, %14\n\t"
      "s_nop 0\n\t"
      "v_subbrev_co_u32_e64 %1, %4, 0, %9, %4\n\t"
      "v_subbrev_co_u32_e64 %3, %5, 0, %13, %5\n\t"
      "s_or_b64 %6, %4, %5"
      : "=&v"(tlA), "=&v"(thA), "=&v"(tlB), "=&v"(thB), "=&s"(bA), "=&s"(bB), "=&s"(bm)
      : "v"(lo32(loA)), "v"(hi32(hiA)), "v"(hi32(loA)), "s"(cyA), "v"(lo32(loB)), "v"(hi32(hiB)), "v"(hi32(loB)), "s"(cyB)
      : "scc");
  uint64_t tA = pack(tlA, thA), tB = pack(tlB, thB);
  if (__builtin_expect(bm != 0, 0)) {  // (3): a 2^-32 event per product; a chain whose mask is zero subtracts 0
    uint32_t nA, nB;
    // bA, bB were written in another statement: the whole pad in front (the compare and the branch between count, but are not in sight)
    asm volatile("s_nop 1\n\tv_cndmask_b32 %0, 0, -1, %2\n\tv_cndmask_b32 %1, 0, -1, %3" : "=&v"(nA), "=v"(nB) : "s"(bA), "s"(bB));
    tA -= nA;
    tB -= nB;
  }
  // the folds t0 + w2 (2^32 - 1) (`fold_top`). Wait states of the carry-outs:
  //   A (%1): written by the 1st multiply-add, read by the 1st select: the 2nd multiply-add (chain B) + `s_nop 0`;
  //   B (%4): written by the 2nd multiply-add, read by the 2nd select: `s_nop 0` + the 1st select (chain A).
  // The repair + (2^32 - 1) of chain A is the 64-bit add of `fold_top` (its mask, zero-extended, shares the kernel's one zero register);
  // chain B's mask would need a second zero register and a move per pair, so its repair is one more multiply-add, bit (0 / 1) times
  // 2^32 - 1 plus the sum: the same value, and the pair stays at 22 instructions.
  uint64_t fA, fB, cA, cB, cD;
  uint32_t mA, nB;
  asm("v_mad_u64_u32 %0, %1, %8, -1, %9\n\t"
      "v_mad_u64_u32 %3, %4, %10, -1, %11\n\t"
      "s_nop 0\n\t"
      "v_cndmask_b32 %2, 0, -1, %1\n\t"
      "v_cndmask_b32 %5, 0, 1, %4\n\t"
      "v_mad_u64_u32 %6, %7, %5, -1, %3"
      : "=&v"(fA), "=&s"(cA), "=&v"(mA), "=&v"(fB), "=&s"(cB), "=&v"(nB), "=&v"(r1), "=&s"(cD)
      : "v"(lo32(hiA)), "v"(tA), "v"(lo32(hiB)), "v"(tB));
  r0 = fA + mA;  // (4): neither can wrap again
#else
  r0 = mul_lazy(a0, b0);
  r1 = mul_lazy(a1, b1);
#endif
}
// Two independent 128-bit values in one go: r0 == lo0 + hi0 2^64, r1 == lo1 + hi1 2^64, each the lazy word of the two-operand
// `reduce128_lazy`, bit for bit. It is the reduction of `mul_lazy2` without the carry-ins, for callers whose 128-bit values are no
// products (ntt16.h's shifts): the two borrow chains alternate, so that each low-word borrow has its sibling's subtract as the first of its
// two wait states and an `s_nop 0` as the second; the 64-bit borrow masks are ORed on the scalar side and tested ONCE, both chains are
// repaired behind that single wave-uniform branch, and the folds run against each other exactly as in `mul_lazy2`. Per pair: one branch
// instead of two, 2 wait states of `s_nop` (2 more behind the rare branch) instead of 8.
GL_HD void reduce128_lazy2(uint64_t lo0, uint64_t hi0, uint64_t lo1, uint64_t hi1, uint64_t &r0, uint64_t &r1) {
#if GL_DEVICE_ASM
  // the borrow chains lo - hi32(hi). Wait states:
  //   low-word borrow of A (%4): written by the 1st subtract, read by the 3rd: the 2nd subtract (chain B) + `s_nop 0`;
  //   low-word borrow of B (%5): written by the 2nd subtract, read by the 4th: `s_nop 0` + the 3rd subtract (chain A);
  //   the 64-bit borrows are read next by `s_or_b64` (SALU: no wait states) and, behind the branch, by the repair below.
  uint32_t tlA, thA, tlB, thB;
  uint64_t bA, bB, bm;
  asm("v_sub_co_u32_e64 %0, %4, %7, %8\n\t"
      "v_sub_co_u32_e64 %2, %5, %10, %11\n\t"
      "s_nop 0\n\t"
      "v_subbrev_co_u32_e64 %1, %4, 0, %9, %4\n\t"
      "v_subbrev_co_u32_e64 %3, %5, 0, %12, %5\n\t"
      "s_or_b64 %6, %4, %5"
      : "=&v"(tlA), "=&v"(thA), "=&v"(tlB), "=&v"(thB), "=&s"(bA), "=&s"(bB), "=&s"(bm)
      : "v"(lo32(lo0)), "v"(hi32(hi0)), "v"(hi32(lo0)), "v"(lo32(lo1)), "v"(hi32(hi1)), "v"(hi32(lo1))
      : "scc");
  uint64_t tA = pack(tlA, thA), tB = pack(tlB, thB);
  if (__builtin_expect(bm != 0, 0)) {  // lo < hi32(hi) in either chain; a chain whose mask is zero subtracts 0
    uint32_t nA, nB;
    // bA, bB were written in another statement: the whole pad in front
    asm volatile("s_nop 1\n\tv_cndmask_b32 %0, 0, -1, %2\n\tv_cndmask_b32 %1, 0, -1, %3" : "=&v"(nA), "=v"(nB) : "s"(bA), "s"(bB));
    tA -= nA;
    tB -= nB;
  }
  // the folds t0 + w2 (2^32 - 1), as in `mul_lazy2`: chain A's repair is the 64-bit add of `fold_top`, chain B's one more multiply-add,
  // bit (0 / 1) times 2^32 - 1 plus the sum — the same value. Wait states of the carry-outs:
  //   A (%1): written by the 1st multiply-add, read by the 1st select: the 2nd multiply-add (chain B) + `s_nop 0`;
  //   B (%4): written by the 2nd multiply-add, read by the 2nd select: `s_nop 0` + the 1st select (chain A).
  uint64_t fA, fB, cA, cB, cD;
  uint32_t mA, nB;
  asm("v_mad_u64_u32 %0, %1, %8, -1, %9\n\t"
      "v_mad_u64_u32 %3, %4, %10, -1, %11\n\t"
      "s_nop 0\n\t"
      "v_cndmask_b32 %2, 0, -1, %1\n\t"
      "v_cndmask_b32 %5, 0, 1, %4\n\t"
      "v_mad_u64_u32 %6, %7, %5, -1, %3"
      : "=&v"(fA), "=&s"(cA), "=&v"(mA), "=&v"(fB), "=&s"(cB), "=&v"(nB), "=&v"(r1), "=&s"(cD)
      : "v"(lo32(hi0)), "v"(tA), "v"(lo32(hi1)), "v"(tB));
  r0 = fA + mA;  // neither can wrap again (note (4) above `fold_top`)
#else
  r0 = reduce128_lazy(lo0, hi0);
  r1 = reduce128_lazy(lo1, hi1);
#endif
}
// the canonical forms of the two pairs
GL_HD void reduce128_2(uint64_t lo0, uint64_t hi0, uint64_t lo1, uint64_t hi1, uint64_t &r0, uint64_t &r1) {
  uint64_t t0, t1;
  reduce128_lazy2(lo0, hi0, lo1, hi1, t0, t1);
  r0 = canon(t0);
  r1 = canon(t1);
}
GL_HD void mul2(uint64_t a0, uint64_t b0, uint64_t a1, uint64_t b1, uint64_t &r0, uint64_t &r1) {
  uint64_t t0, t1;
  mul_lazy2(a0, b0, a1, b1, t0, t1);
  r0 = canon(t0);
  r1 = canon(t1);
}
GL_HD uint64_t mul(uint64_t a, uint64_t b) {
  uint64_t lo, hi;
  carry_t cy;
  mul_wide_cy(a, b, lo, hi, cy);
  return reduce128(lo, hi, cy);
}
GL_HD uint64_t sqr(uint64_t a) { return mul(a, a); }
// a*b + c as a lazy u64 (any representative < 2^64 of the class); a, b, c may be lazy themselves
GL_HD uint64_t mul_add_lazy(uint64_t a, uint64_t b, uint64_t c) {
  uint64_t lo, hi;
  carry_t cy;
  mul_wide_cy(a, b, lo, hi, cy);
  lo += c;
  hi += lo < c;  // (2): a*b + c <= (2^64-1) 2^64 keeps the true high half <= 2^64-1, and hi' below it
  return reduce128_lazy(lo, hi, cy);
}

GL_HD uint64_t pow7(uint64_t x) {
  uint64_t x2 = sqr(x), x4 = sqr(x2), x3 = mul(x, x2);
  return mul(x3, x4);
}

GL_HD uint64_t pow(uint64_t b, uint64_t e) {
  uint64_t r = 1;
  while (e) {
    if (e & 1) r = mul(r, b);
    b = sqr(b);
    e >>= 1;
  }
  return r;
}
GL_HD uint64_t inv(uint64_t a) { return pow(a, P - 2); }

// quadratic extension F_p[X]/(X^2 - 7)
struct Ext {
  uint64_t a, b;
};
GL_HD Ext ext_add(Ext x, Ext y) { return {add(x.a, y.a), add(x.b, y.b)}; }
GL_HD Ext ext_sub(Ext x, Ext y) { return {sub(x.a, y.a), sub(x.b, y.b)}; }
GL_HD Ext ext_mul(Ext x, Ext y) {
  uint64_t bb = mul(x.b, y.b);
  return {add(mul(x.a, y.a), mul(bb, 7)), add(mul(x.a, y.b), mul(x.b, y.a))};
}
GL_HD Ext ext_scale(Ext x, uint64_t s) { return {mul(x.a, s), mul(x.b, s)}; }

}  // namespace gl
