// Square roots in F_p and F_p^2 of BLS12-381 and the decoding of a compressed point around them.
// __host__ __device__ throughout, like pairing.h: the kernels of pairing.hip, the host functions of groth16_pack.inc and
// tests/sqrtsim run this very text.
//
// p = 3 mod 4, so everything here hangs on ONE exponentiation, w = a^((p - 3) / 4):
//   t = w a = a^((p + 1) / 4) and t^2 = a^((p - 1) / 2) a = +-a: t is a root of a where a is a residue, of -a where it is not,
//   and w t = a^((p - 1) / 2) = +-1 tells which, so 1 / t = +-w comes with it.
// The exponent is a compile-time constant, the same in every lane: a fixed 2-bit window (a, a^2, a^3: three entries of 14
// registers) costs no divergence - 380 squarings and 143 products for the 379 bits.
//
// F_p^2 = F_p[u] / (u^2 + 1) goes through the norm: for a = c0 + c1 u with c1 != 0, a root x0 + x1 u has
//   x0^2 - x1^2 = c0, 2 x0 x1 = c1, so (x0^2 + x1^2)^2 = c0^2 + c1^2 =: n, and a has a root exactly where n is a residue of F_p.
// With s^2 = n, d = (c0 + s) / 2 and d' = (c0 - s) / 2 = d - s: d d' = -c1^2 / 4 is a non-residue (-1 is one), so exactly one of
// d, d' is a residue, x0^2. The exponentiation of d gives t with t^2 = +-d and 1 / t:
//   d a residue:     x0 = t,            x1 = c1 / (2 t)
//   d a non-residue: x0 = c1 / (2 t),   x1 = t         (t^2 = -d, and (c1 / (2 t))^2 = c1^2 / (-4 d) = d')
// Two exponentiations in F_p and a handful of products, against two exponentiations in F_p^2 (three products each step) of
// the textbook algorithm. c1 = 0 needs one: a root of c0 is (t, 0) where c0 is a residue and (0, t) where it is not.
// Which of the two roots comes out is not specified: callers pick by the "larger" predicates below.
#pragma once
#include "pairing.h"

namespace blssqrt {

using bls::Fp;
using bls::Fp2;
using bls::NL;

GL_HD Fp fp_neg(const Fp &a) { return bls::fp_sub(bls::fp_zero(), a); }
// a / 2: (a + p) / 2 where a is odd. Linear, so it holds on Montgomery limbs as on plain ones.
GL_HD Fp fp_half(const Fp &a) {
  Fp r;
  const uint32_t odd = a.l[0] & 1;
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const uint32_t s = a.l[i] + (odd ? BLS_P[i] : 0u) + c;  // a + p < 2^382: no carry out of the top limb
    r.l[i] = s & bls::LM;
    c = s >> bls::LB;
  }
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = (r.l[i] >> 1) | (i + 1 < NL ? (r.l[i + 1] & 1) << (bls::LB - 1) : 0u);
  return r;
}
// digit k of (p - 3) / 4 in base 4: bits 2 k + 2, 2 k + 3 of p - 3 (p ends in ...aaab: no borrow; a digit never straddles a word)
GL_HD uint32_t p34_digit(int k) {
  const int bit = 2 * k + 2;
  const uint32_t w = BLS_P32[bit >> 5] - (bit < 32 ? 3u : 0u);
  return (w >> (bit & 31)) & 3;
}
constexpr int P34_DIGITS = 190;  // p has 381 bits: the top digit is bit 380 alone
// a^((p - 3) / 4)
PAIRING_FN Fp fp_pow_p34(const Fp &a) {
  const Fp a2 = bls::fp_sqr(a), a3 = bls::fp_mul(a2, a);
  Fp r = a;  // the top digit is 1
#pragma unroll 1
  for (int k = P34_DIGITS - 2; k >= 0; k--) {
    r = bls::fp_sqr(bls::fp_sqr(r));
    const uint32_t d = p34_digit(k);  // the same in every lane
    if (d) {
      Fp m;
#pragma unroll
      for (int i = 0; i < NL; i++) m.l[i] = d == 1 ? a.l[i] : d == 2 ? a2.l[i] : a3.l[i];
      r = bls::fp_mul(r, m);
    }
  }
  return r;
}
// t with t^2 = a or t^2 = -a (returns which: true for a), and 1 / t (0 for a = 0)
GL_HD bool fp_sqrt_either(const Fp &a, Fp &t, Fp &t_inv) {
  const Fp w = fp_pow_p34(a);
  t = bls::fp_mul(w, a);
  const bool residue = bls::fp_eq(bls::fp_sqr(t), a);
  t_inv = residue ? w : fp_neg(w);  // w t = a^((p - 1) / 2)
  return residue;
}
GL_HD bool fp_sqrt(const Fp &a, Fp *root) {
  Fp t, ti;
  if (!fp_sqrt_either(a, t, ti)) return false;
  *root = t;
  return true;
}
GL_HD bool fp2_sqrt(const Fp2 &a, Fp2 *root) {
  Fp t, ti;
  Fp2 r;
  if (bls::fp_is_zero(a.c1)) {
    if (fp_sqrt_either(a.c0, t, ti)) r = {t, bls::fp_zero()};
    else r = {bls::fp_zero(), t};
  } else {
    Fp s;
    if (!fp_sqrt(bls::fp_add(bls::fp_sqr(a.c0), bls::fp_sqr(a.c1)), &s)) return false;
    const bool residue = fp_sqrt_either(fp_half(bls::fp_add(a.c0, s)), t, ti);
    const Fp o = bls::fp_mul(fp_half(a.c1), ti);  // c1 / (2 t)
    if (residue) r = {t, o};
    else r = {o, t};
  }
  if (!bls::f_eq(bls::fp2_sqr(r), a)) return false;
  *root = r;
  return true;
}

// y > -y on canonical integers: y > (p - 1) / 2, that is 2 y > p (y = 0 is not larger)
GL_HD bool fp_is_larger(const Fp &y) {
  uint32_t w[12];
  bls::fp_to_canonical(y, w);
  int c = 0;  // 2 y (below 2^382: it fits the 12 words) against p, from the top word down
  for (int k = 11; k >= 0; k--) {
    const uint32_t d = (w[k] << 1) | (k ? w[k - 1] >> 31 : 0u);
    if (c == 0 && d != BLS_P32[k]) c = d > BLS_P32[k] ? 1 : -1;
  }
  return c > 0;
}
// in F_p^2: by c1, and by c0 where c1 = -c1 (c1 = 0)
GL_HD bool fp2_is_larger(const Fp2 &y) { return bls::fp_is_zero(y.c1) ? fp_is_larger(y.c0) : fp_is_larger(y.c1); }

// ---- one compressed element of the stored Groth16 proof: x little-endian, the flags in the two top bits of the last byte ----
// Status classes of cp_groth16_proofs_unpack_city_bls12381: 0 ok, 1 a flag bit that may not be set, 2 x >= p, 3 no such point.
// src: the 12 (G1) or 24 (G2: a0 then a1, the flags on a1) words as stored; xy: 24 / 48 words, affine canonical, written for status 0.
GL_HD int g1_decompress(const uint32_t *src, uint32_t *xy) {
  uint32_t w[12];
  for (int i = 0; i < 12; i++) w[i] = src[i];
  const uint32_t flags = w[11] >> 30;  // 0x80, 0x40 of byte 47
  w[11] &= 0x3FFFFFFFu;
  if (flags & 1) return 1;
  if (!pairing::words_below_p(w)) return 2;
  const Fp x = bls::fp_from_canonical(w);
  Fp y;
  if (!fp_sqrt(bls::fp_add(bls::fp_mul(bls::fp_sqr(x), x), bls::Field<Fp>::curve_b()), &y)) return 3;
  if (fp_is_larger(y) != ((flags & 2) != 0)) y = fp_neg(y);
  for (int i = 0; i < 12; i++) xy[i] = w[i];
  bls::fp_to_canonical(y, xy + 12);
  return 0;
}
GL_HD int g2_decompress(const uint32_t *src, uint32_t *xy) {
  uint32_t w[24];
  for (int i = 0; i < 24; i++) w[i] = src[i];
  const uint32_t flags = w[23] >> 30;
  w[23] &= 0x3FFFFFFFu;
  if ((flags & 1) || (w[11] >> 30)) return 1;
  if (!pairing::words_below_p(w) || !pairing::words_below_p(w + 12)) return 2;
  const Fp2 x = bls::Field<Fp2>::from_canonical(w);
  Fp2 y;
  if (!fp2_sqrt(bls::fp2_add(bls::fp2_mul(bls::fp2_sqr(x), x), bls::Field<Fp2>::curve_b()), &y)) return 3;
  if (fp2_is_larger(y) != ((flags & 2) != 0)) y = pairing::fp2_neg(y);
  for (int i = 0; i < 24; i++) xy[i] = w[i];
  bls::Field<Fp2>::to_canonical(y, xy + 24);
  return 0;
}

}  // namespace blssqrt
