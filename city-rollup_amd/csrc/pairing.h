// The optimal-ate pairing of BLS12-381 on top of bls12_381.h: the tower, the Miller loop, the final
// exponentiation. __host__ __device__ throughout, like that header: tests/pairingsim runs this very code on the CPU.
//
// F_p^12 = F_p^2[w] / (w^6 - xi), xi = 1 + u. An element is its six F_p^2 coefficients a_0 .. a_5 of w^0 .. w^5. This is the
// tower F_p^6 = F_p^2[v] / (v^3 - xi), F_p^12 = F_p^6[w] / (w^2 - v) with v = w^2: the even coefficients (a_0, a_2, a_4) are
// the F_p^6 part c0, the odd ones (a_1, a_3, a_5) are c1.
//
// An F_p^12 value is 168 registers, too many to hold beside anything else (the G2 kernels spill at 512 already), so the
// functions here never take one by value: they work on an F12 *reference* - a base pointer and a stride between limbs - and
// touch one F_p^2 coefficient at a time. Limb l of component h of coefficient k lives at p[((2 k + h) * 14 + l) * stride]. With
// stride = lanes the same code addresses an LDS array [coefficient limb][lane] (conflict-free: consecutive lanes, consecutive
// banks), a work array in HBM of the same shape (coalesced), or, with stride 1, a plain array on the host. The functions are
// loops over coefficients around the non-inlined F_p products, and are themselves not inlined: no body grows with the
// number of operations of a pairing (a 315 KiB body once outgrew the reach of a short branch, commit 2ef0361).
//
// The pairing computed is e(P, Q)^c with c = BLS_FINAL_EXP_C = 3: the hard part of the final exponentiation uses
//   3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3        (checked in gen_bls_tables.py; 3 is coprime to r).
// Lines are scaled by factors from F_p^2 and by w^3 (an element of F_p^4), which the final exponentiation sends to one.
#pragma once
#include "bls12_381.h"

namespace pairing {

using bls::Fp;
using bls::Fp2;
using bls::NL;

#if defined(__HIP_DEVICE_COMPILE__)
#define PAIRING_NOINLINE __attribute__((noinline))
#else
#define PAIRING_NOINLINE
#endif
#define PAIRING_FN __host__ __device__ PAIRING_NOINLINE inline

constexpr int F12_WORDS = 12 * NL;  // 168 limbs of 28 bits

struct F12 {
  uint32_t *p;
  size_t stride;
};
GL_HD Fp2 f12_get(const F12 &a, int k) {
  Fp2 r;
  const uint32_t *q = a.p + (size_t)(2 * k) * NL * a.stride;
#pragma unroll
  for (int l = 0; l < NL; l++) r.c0.l[l] = q[l * a.stride];
#pragma unroll
  for (int l = 0; l < NL; l++) r.c1.l[l] = q[(NL + l) * a.stride];
  return r;
}
GL_HD void f12_set(const F12 &a, int k, const Fp2 &v) {
  uint32_t *q = a.p + (size_t)(2 * k) * NL * a.stride;
#pragma unroll
  for (int l = 0; l < NL; l++) q[l * a.stride] = v.c0.l[l];
#pragma unroll
  for (int l = 0; l < NL; l++) q[(NL + l) * a.stride] = v.c1.l[l];
}

GL_HD Fp2 fp2_zero() { return {bls::fp_zero(), bls::fp_zero()}; }
GL_HD Fp2 fp2_one() { return {bls::fp_one(), bls::fp_zero()}; }
GL_HD Fp2 fp2_neg(const Fp2 &a) { return bls::fp2_sub(fp2_zero(), a); }
GL_HD Fp2 fp2_conj(const Fp2 &a) { return {a.c0, bls::fp_sub(bls::fp_zero(), a.c1)}; }
GL_HD Fp2 fp2_mul_xi(const Fp2 &a) { return {bls::fp_sub(a.c0, a.c1), bls::fp_add(a.c0, a.c1)}; }  // (c0 + c1 u)(1 + u)
GL_HD Fp2 fp2_mul_fp(const Fp2 &a, const Fp &s) { return {bls::fp_mul(a.c0, s), bls::fp_mul(a.c1, s)}; }
GL_HD Fp2 fp2_dbl(const Fp2 &a) { return bls::fp2_add(a, a); }

PAIRING_FN void f12_copy(F12 out, F12 a) {
  for (int i = 0; i < F12_WORDS; i++) out.p[i * out.stride] = a.p[i * a.stride];
}
PAIRING_FN void f12_set_one(F12 out) {
  for (int i = 0; i < F12_WORDS; i++) out.p[i * out.stride] = i < NL ? BLS_R1[i] : 0u;
}
PAIRING_FN bool f12_eq(F12 a, F12 b) {
  uint32_t o = 0;
  for (int i = 0; i < F12_WORDS; i++) o |= a.p[i * a.stride] ^ b.p[i * b.stride];
  return o == 0;
}
PAIRING_FN bool f12_is_one(F12 a) {
  uint32_t o = 0;
  for (int i = 0; i < F12_WORDS; i++) o |= a.p[i * a.stride] ^ (i < NL ? BLS_R1[i] : 0u);
  return o == 0;
}

// out = a b, schoolbook over the coefficients: 36 F_p^2 products. out must not alias a or b.
PAIRING_FN void f12_mul(F12 out, F12 a, F12 b) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fp2 lo = fp2_zero(), hi = fp2_zero();  // terms with i + j = k, and with i + j = k + 6 (times xi)
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
      const int j = k - i;
      const Fp2 t = bls::fp2_mul(f12_get(a, i), f12_get(b, j < 0 ? j + 6 : j));
      if (j < 0) hi = bls::fp2_add(hi, t); else lo = bls::fp2_add(lo, t);
    }
    f12_set(out, k, bls::fp2_add(lo, fp2_mul_xi(hi)));
  }
}
// out = a^2: 15 products doubled and 6 squares. out must not alias a.
PAIRING_FN void f12_sqr(F12 out, F12 a) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fp2 lo = fp2_zero(), hi = fp2_zero();
#pragma unroll 1
    for (int i = 0; i < 6; i++) {
      int j = k - i;
      const bool wrap = j < 0;
      if (wrap) j += 6;
      if (j < i) continue;
      Fp2 t;
      if (j == i) t = bls::fp2_sqr(f12_get(a, i));
      else t = fp2_dbl(bls::fp2_mul(f12_get(a, i), f12_get(a, j)));
      if (wrap) hi = bls::fp2_add(hi, t); else lo = bls::fp2_add(lo, t);
    }
    f12_set(out, k, bls::fp2_add(lo, fp2_mul_xi(hi)));
  }
}
// a line value of the Miller loop: l0 + l2 w^2 + l3 w^3
struct Line { Fp2 l0, l2, l3; };
// out = a (l0 + l2 w^2 + l3 w^3): 18 F_p^2 products. out must not alias a.
PAIRING_FN void f12_mul_sparse(F12 out, F12 a, const Line &ln) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fp2 r = bls::fp2_mul(f12_get(a, k), ln.l0);
    Fp2 t = bls::fp2_mul(f12_get(a, k >= 2 ? k - 2 : k + 4), ln.l2);
    r = bls::fp2_add(r, k >= 2 ? t : fp2_mul_xi(t));
    t = bls::fp2_mul(f12_get(a, k >= 3 ? k - 3 : k + 3), ln.l3);
    r = bls::fp2_add(r, k >= 3 ? t : fp2_mul_xi(t));
    f12_set(out, k, r);
  }
}
// in place: the conjugate over F_p^6, w -> -w (the inverse of an element of the cyclotomic subgroup)
PAIRING_FN void f12_conj(F12 a) {
  for (int k = 1; k < 6; k += 2) f12_set(a, k, fp2_neg(f12_get(a, k)));
}
// in place: a^(p^j), j = 1, 2, 3
PAIRING_FN void f12_frobenius(F12 a, int j) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fp2 c = f12_get(a, k), g;
    if (j & 1) c = fp2_conj(c);
    for (int l = 0; l < NL; l++) {
      g.c0.l[l] = BLS_FROB[j - 1][k][0][l];
      g.c1.l[l] = BLS_FROB[j - 1][k][1][l];
    }
    f12_set(a, k, bls::fp2_mul(c, g));
  }
}

// ---- F_p^6 by value: only the inversion needs it (once per final exponentiation) ----
struct Fp6 { Fp2 c[3]; };  // c0 + c1 v + c2 v^2, v^3 = xi
PAIRING_FN Fp6 f6_mul(const Fp6 &a, const Fp6 &b) {
  Fp6 r;
#pragma unroll 1
  for (int k = 0; k < 3; k++) {
    Fp2 lo = fp2_zero(), hi = fp2_zero();
#pragma unroll 1
    for (int i = 0; i < 3; i++) {
      const int j = k - i;
      const Fp2 t = bls::fp2_mul(a.c[i], b.c[j < 0 ? j + 3 : j]);
      if (j < 0) hi = bls::fp2_add(hi, t); else lo = bls::fp2_add(lo, t);
    }
    r.c[k] = bls::fp2_add(lo, fp2_mul_xi(hi));
  }
  return r;
}
GL_HD Fp6 f6_sqr(const Fp6 &a) { return f6_mul(a, a); }
GL_HD Fp6 f6_sub(const Fp6 &a, const Fp6 &b) { return {{bls::fp2_sub(a.c[0], b.c[0]), bls::fp2_sub(a.c[1], b.c[1]), bls::fp2_sub(a.c[2], b.c[2])}}; }
GL_HD Fp6 f6_neg(const Fp6 &a) { return {{fp2_neg(a.c[0]), fp2_neg(a.c[1]), fp2_neg(a.c[2])}}; }
GL_HD Fp6 f6_mul_v(const Fp6 &a) { return {{fp2_mul_xi(a.c[2]), a.c[0], a.c[1]}}; }
// 1 / a through one inversion in F_p^2, which is one f_inv in F_p (a = 0 gives 0)
PAIRING_FN Fp6 f6_inv(const Fp6 &a) {
  const Fp2 t0 = bls::fp2_sub(bls::fp2_sqr(a.c[0]), fp2_mul_xi(bls::fp2_mul(a.c[1], a.c[2])));
  const Fp2 t1 = bls::fp2_sub(fp2_mul_xi(bls::fp2_sqr(a.c[2])), bls::fp2_mul(a.c[0], a.c[1]));
  const Fp2 t2 = bls::fp2_sub(bls::fp2_sqr(a.c[1]), bls::fp2_mul(a.c[0], a.c[2]));
  const Fp2 d = bls::fp2_add(bls::fp2_mul(a.c[0], t0), fp2_mul_xi(bls::fp2_add(bls::fp2_mul(a.c[2], t1), bls::fp2_mul(a.c[1], t2))));
  const Fp2 di = bls::fp2_inv(d);
  return {{bls::fp2_mul(t0, di), bls::fp2_mul(t1, di), bls::fp2_mul(t2, di)}};
}
GL_HD Fp6 f12_get6(const F12 &a, int odd) { return {{f12_get(a, odd), f12_get(a, 2 + odd), f12_get(a, 4 + odd)}}; }
GL_HD void f12_set6(const F12 &a, int odd, const Fp6 &v) { for (int i = 0; i < 3; i++) f12_set(a, 2 * i + odd, v.c[i]); }
// out = 1 / a = (a0 - a1 w) / (a0^2 - v a1^2); out may alias a
PAIRING_FN void f12_inv(F12 out, F12 a) {
  const Fp6 a0 = f12_get6(a, 0), a1 = f12_get6(a, 1);
  const Fp6 d = f6_inv(f6_sub(f6_sqr(a0), f6_mul_v(f6_sqr(a1))));
  f12_set6(out, 0, f6_mul(a0, d));
  f12_set6(out, 1, f6_neg(f6_mul(a1, d)));
}

// ---- the cyclotomic subgroup (what the easy part of the final exponentiation maps into) ----
// (a + b s)^2 in F_p^4 = F_p^2[s] / (s^2 - xi)
PAIRING_FN void fp4_sqr(const Fp2 &a, const Fp2 &b, Fp2 &c0, Fp2 &c1) {
  const Fp2 t0 = bls::fp2_sqr(a), t1 = bls::fp2_sqr(b);
  c0 = bls::fp2_add(fp2_mul_xi(t1), t0);
  c1 = bls::fp2_sub(bls::fp2_sub(bls::fp2_sqr(bls::fp2_add(a, b)), t0), t1);
}
// in place: a^2 for a in the cyclotomic subgroup (Granger-Scott): three F_p^4 squarings, 9 F_p^2 squarings in all
PAIRING_FN void f12_cyclotomic_sqr(F12 a) {
  Fp2 t0, t1, t2, t3, z;
  fp4_sqr(f12_get(a, 0), f12_get(a, 3), t0, t1);
  z = f12_get(a, 0);
  z = bls::fp2_sub(t0, z);
  f12_set(a, 0, bls::fp2_add(fp2_dbl(z), t0));  // 3 t0 - 2 z0
  z = f12_get(a, 3);
  z = bls::fp2_add(t1, z);
  f12_set(a, 3, bls::fp2_add(fp2_dbl(z), t1));  // 3 t1 + 2 z1
  fp4_sqr(f12_get(a, 1), f12_get(a, 4), t0, t1);
  fp4_sqr(f12_get(a, 2), f12_get(a, 5), t2, t3);
  z = bls::fp2_sub(t0, f12_get(a, 2));
  f12_set(a, 2, bls::fp2_add(fp2_dbl(z), t0));
  z = bls::fp2_add(t1, f12_get(a, 5));
  f12_set(a, 5, bls::fp2_add(fp2_dbl(z), t1));
  t0 = fp2_mul_xi(t3);
  z = bls::fp2_add(t0, f12_get(a, 1));
  f12_set(a, 1, bls::fp2_add(fp2_dbl(z), t0));
  z = bls::fp2_sub(t2, f12_get(a, 4));
  f12_set(a, 4, bls::fp2_add(fp2_dbl(z), t2));
}
// out = a^|x| for a in the cyclotomic subgroup; tmp: scratch. out, a, tmp distinct.
PAIRING_FN void f12_exp_abs_x(F12 out, F12 a, F12 tmp) {
  f12_copy(out, a);
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    f12_cyclotomic_sqr(out);
    if ((BLS_X_ABS >> i) & 1) {
      f12_mul(tmp, out, a);
      f12_copy(out, tmp);
    }
  }
}
// out = a^x (x negative: the conjugate of a^|x|)
GL_HD void f12_exp_x(F12 out, F12 a, F12 tmp) {
  f12_exp_abs_x(out, a, tmp);
  f12_conj(out);
}

// ---- Miller loop: T on the twist y^2 = x^3 + 4 xi in Jacobian coordinates, lines evaluated at P = (xp, yp) in G1 ----
// With the untwist (x', y') -> (x' / w^2, y' / w^3) the line through the images with twist slope s, times w^3, is
//   yp w^3 - s xp w^2 + (s x'_T - y'_T).
// T <- 2 T. The tangent slope is 3 X^2 / Z3, Z3 = 2 Y Z; the line is scaled by Z3 Z^2:
//   l0 = 3 X^3 - 2 Y^2, l2 = -3 X^2 Z^2 xp, l3 = Z3 Z^2 yp.
PAIRING_FN Line miller_double(bls::Jac2 &t, const bls::Affine &p) {
  const Fp2 A = bls::fp2_sqr(t.x), B = bls::fp2_sqr(t.y), C = bls::fp2_sqr(B), zz = bls::fp2_sqr(t.z);
  const Fp2 E = bls::fp2_add(fp2_dbl(A), A);                                             // 3 X^2
  const Fp2 D = fp2_dbl(bls::fp2_sub(bls::fp2_sub(bls::fp2_sqr(bls::fp2_add(t.x, B)), A), C));  // 4 X Y^2
  const Fp2 z3 = fp2_dbl(bls::fp2_mul(t.y, t.z));
  Line ln;
  ln.l0 = bls::fp2_sub(bls::fp2_mul(E, t.x), fp2_dbl(B));
  ln.l2 = fp2_neg(fp2_mul_fp(bls::fp2_mul(E, zz), p.x));
  ln.l3 = fp2_mul_fp(bls::fp2_mul(z3, zz), p.y);
  const Fp2 x3 = bls::fp2_sub(bls::fp2_sqr(E), fp2_dbl(D));
  t.y = bls::fp2_sub(bls::fp2_mul(E, bls::fp2_sub(D, x3)), fp2_dbl(fp2_dbl(fp2_dbl(C))));
  t.x = x3;
  t.z = z3;
  return ln;
}
// T <- T + Q, Q affine. The chord slope is R / Z3 with R = yq Z^3 - Y, H = xq Z^2 - X, Z3 = Z H; the line is scaled by Z3:
//   l0 = R xq - yq Z3, l2 = -R xp, l3 = Z3 yp.
// Straight-line arithmetic: T = +-Q (outside the r-torsion only) gives a meaningless value, never a division.
PAIRING_FN Line miller_add(bls::Jac2 &t, const bls::Affine2 &q, const bls::Affine &p) {
  const Fp2 zz = bls::fp2_sqr(t.z);
  const Fp2 H = bls::fp2_sub(bls::fp2_mul(q.x, zz), t.x);
  const Fp2 R = bls::fp2_sub(bls::fp2_mul(bls::fp2_mul(q.y, t.z), zz), t.y);
  const Fp2 z3 = bls::fp2_mul(t.z, H);
  Line ln;
  ln.l0 = bls::fp2_sub(bls::fp2_mul(R, q.x), bls::fp2_mul(q.y, z3));
  ln.l2 = fp2_neg(fp2_mul_fp(R, p.x));
  ln.l3 = fp2_mul_fp(z3, p.y);
  const Fp2 hh = bls::fp2_sqr(H), hhh = bls::fp2_mul(H, hh), v = bls::fp2_mul(t.x, hh);
  const Fp2 x3 = bls::fp2_sub(bls::fp2_sub(bls::fp2_sqr(R), hhh), fp2_dbl(v));
  t.y = bls::fp2_sub(bls::fp2_mul(R, bls::fp2_sub(v, x3)), bls::fp2_mul(t.y, hhh));
  t.x = x3;
  t.z = z3;
  return ln;
}
// f = f_{|x|, Q}(P) conjugated (x is negative): 63 doubling steps, 5 addition steps. f: the running value (LDS on the
// device), tmp: scratch of the same shape; the result is in f.
PAIRING_FN void miller_loop(F12 f, F12 tmp, const bls::Affine &p, const bls::Affine2 &q) {
  bls::Jac2 t = {q.x, q.y, fp2_one()};
  f12_set_one(f);
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    f12_sqr(tmp, f);
    f12_mul_sparse(f, tmp, miller_double(t, p));
    if ((BLS_X_ABS >> i) & 1) {
      f12_copy(tmp, f);
      f12_mul_sparse(f, tmp, miller_add(t, q, p));
    }
  }
  f12_conj(f);
}

// ---- final exponentiation: f <- f^(c (p^12 - 1) / r), c = 3. t0 .. t3: scratch; f and the scratch values all distinct ----
// the easy part alone: f <- f^((p^6 - 1)(p^2 + 1)), into the cyclotomic subgroup (f = 0 stays 0)
PAIRING_FN void final_exp_easy(F12 f, F12 t0, F12 t1) {
  f12_inv(t0, f);
  f12_conj(f);
  f12_mul(t1, f, t0);  // f^(p^6 - 1)
  f12_copy(t0, t1);
  f12_frobenius(t0, 2);
  f12_mul(f, t0, t1);
}
// the hard part: m^((x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3) for m in the cyclotomic subgroup; the result replaces m
PAIRING_FN void final_exp_hard(F12 m, F12 t0, F12 t1, F12 t2, F12 t3) {
  // a = m^((x - 1)^2) -> t1
  f12_exp_x(t0, m, t3);   // m^x
  f12_copy(t1, m);
  f12_conj(t1);
  f12_mul(t2, t0, t1);    // m^(x - 1)
  f12_exp_x(t0, t2, t3);
  f12_conj(t2);
  f12_mul(t1, t0, t2);    // a
  // b = a^(x + p) -> t2
  f12_exp_x(t0, t1, t3);
  f12_frobenius(t1, 1);
  f12_mul(t2, t0, t1);    // b
  // d = b^(x^2 + p^2 - 1) -> t2
  f12_exp_x(t0, t2, t3);
  f12_exp_x(t1, t0, t3);  // b^(x^2)
  f12_copy(t0, t2);
  f12_conj(t0);           // b^-1
  f12_mul(t3, t1, t0);
  f12_frobenius(t2, 2);
  f12_mul(t0, t3, t2);    // d
  // d m^3
  f12_copy(t1, m);
  f12_cyclotomic_sqr(t1);
  f12_mul(t2, t1, m);
  f12_mul(m, t0, t2);
}
GL_HD void final_exp(F12 f, F12 t0, F12 t1, F12 t2, F12 t3) {
  final_exp_easy(f, t0, t1);
  final_exp_hard(f, t0, t1, t2, t3);
}

// ---- [r] P = infinity ? plain double-and-add over the 255 bits of r (the top bit starts the accumulator) ----
// (the two group operations are calls: inlined, the G2 check alone was a body of 123 KiB)
template <class F> PAIRING_FN void torsion_double(bls::JacT<F> &t) { t = bls::jac_double(t); }
template <class F> PAIRING_FN void torsion_add(bls::JacT<F> &t, const bls::AffineT<F> &p) {  // jac_add_mixed with its doubling as the call above
  if (bls::jac_is_inf(t)) { t = {p.x, p.y, bls::Field<F>::one()}; return; }
  const F z1z1 = bls::f_sqr(t.z);
  const F u2 = bls::f_mul(p.x, z1z1), s2 = bls::f_mul(bls::f_mul(p.y, t.z), z1z1);
  if (bls::f_eq(t.x, u2)) {
    if (bls::f_eq(t.y, s2)) torsion_double(t);
    else t = bls::jac_inf<F>();
    return;
  }
  const F h = bls::f_sub(u2, t.x), rr = bls::f_sub(s2, t.y);
  const F hh = bls::f_sqr(h), hhh = bls::f_mul(h, hh), v = bls::f_mul(t.x, hh);
  const F x3 = bls::f_sub(bls::f_sub(bls::f_sqr(rr), hhh), bls::f_dbl(v));
  t.y = bls::f_sub(bls::f_mul(rr, bls::f_sub(v, x3)), bls::f_mul(t.y, hhh));
  t.x = x3;
  t.z = bls::f_mul(t.z, h);
}
template <class F>
PAIRING_FN bool in_r_torsion(const bls::AffineT<F> &p) {
  bls::JacT<F> t = {p.x, p.y, bls::Field<F>::one()};
#pragma unroll 1
  for (int i = 253; i >= 0; i--) {
    torsion_double(t);
    if ((BLS_FR_P32[i >> 5] >> (i & 31)) & 1) torsion_add(t, p);
  }
  return bls::jac_is_inf(t);
}
// ---- [k] P in G1 for a short scalar: k < 2^128 as four 32-bit words, plain double-and-add from the top bit with the group
// law of bls12_381.h. Infinity comes out only for k = 0 or a P of small order (outside the r-torsion). ----
PAIRING_FN bls::Jac g1_mul_u128(const bls::Affine &p, const uint32_t *k) {
  bls::Jac t = bls::jac_inf<Fp>();
#pragma unroll 1
  for (int i = 127; i >= 0; i--) {
    t = bls::jac_double(t);
    if ((k[i >> 5] >> (i & 31)) & 1) t = bls::jac_add_mixed(t, p);
  }
  return t;
}
GL_HD bool words_below_p(const uint32_t *w) {  // 12 words < p ?
  for (int k = 11; k >= 0; k--) {
    if (w[k] < BLS_P32[k]) return true;
    if (w[k] > BLS_P32[k]) return false;
  }
  return false;
}
// an affine canonical point from the API: 0 ok, 1 a coordinate >= p, 2 not on the curve / twist, 3 not in the r-torsion
template <class F>
GL_HD int point_status(const uint32_t *xy, bool check_torsion, bls::AffineT<F> &out) {
  constexpr int W = bls::Field<F>::WORDS;
  for (int h = 0; h < 2 * W / 12; h++)
    if (!words_below_p(xy + 12 * h)) return 1;
  out = bls::affine_from_canonical<F>(xy);
  if (!bls::affine_on_curve(out)) return 2;
  if (check_torsion && !in_r_torsion(out)) return 3;
  return 0;
}

}  // namespace pairing
