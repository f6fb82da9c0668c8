// TEST-ONLY: the __host__ __device__ arithmetic of the pairing (city-rollup_amd/csrc/pairing.h) built for the CPU, so that the
// exact code the kernels run is held against Python integers without a GPU. Never loaded by the product path. Every value
// crosses as canonical little-endian u64 words: 6 per F_p element, F_p^2 as c0 | c1, F_p^12 as its 6 coefficients of w^0 .. w^5.
#include "../../city-rollup_amd/csrc/pairing.h"

namespace {
using namespace pairing;
struct V12 {
  uint32_t w[F12_WORDS];
  F12 ref() { return {w, 1}; }
};
Fp2 in2(const uint64_t *w) { return bls::Field<Fp2>::from_canonical((const uint32_t *)w); }
void out2(const Fp2 &a, uint64_t *w) { bls::Field<Fp2>::to_canonical(a, (uint32_t *)w); }
void in12(const uint64_t *w, V12 &v) { for (int k = 0; k < 6; k++) f12_set(v.ref(), k, in2(w + 12 * k)); }
void out12(V12 &v, uint64_t *w) { for (int k = 0; k < 6; k++) out2(f12_get(v.ref(), k), w + 12 * k); }
Fp6 in6(const uint64_t *w) { return {{in2(w), in2(w + 12), in2(w + 24)}}; }
void out6(const Fp6 &a, uint64_t *w) { for (int i = 0; i < 3; i++) out2(a.c[i], w + 12 * i); }
}  // namespace

extern "C" {
unsigned ps_final_exp_c(void) { return BLS_FINAL_EXP_C; }
void ps_f12_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) { V12 x, y, z; in12(a, x); in12(b, y); f12_mul(z.ref(), x.ref(), y.ref()); out12(z, out); }
void ps_f12_sqr(const uint64_t *a, uint64_t *out) { V12 x, z; in12(a, x); f12_sqr(z.ref(), x.ref()); out12(z, out); }
void ps_f12_inv(const uint64_t *a, uint64_t *out) { V12 x; in12(a, x); f12_inv(x.ref(), x.ref()); out12(x, out); }
void ps_f12_conj(const uint64_t *a, uint64_t *out) { V12 x; in12(a, x); f12_conj(x.ref()); out12(x, out); }
void ps_f12_frobenius(const uint64_t *a, int j, uint64_t *out) { V12 x; in12(a, x); f12_frobenius(x.ref(), j); out12(x, out); }
void ps_f12_mul_sparse(const uint64_t *a, const uint64_t *l0, const uint64_t *l2, const uint64_t *l3, uint64_t *out) {
  V12 x, z;
  in12(a, x);
  f12_mul_sparse(z.ref(), x.ref(), Line{in2(l0), in2(l2), in2(l3)});
  out12(z, out);
}
void ps_f12_cyclotomic_sqr(const uint64_t *a, uint64_t *out) { V12 x; in12(a, x); f12_cyclotomic_sqr(x.ref()); out12(x, out); }
void ps_f12_exp_abs_x(const uint64_t *a, uint64_t *out) { V12 x, z, t; in12(a, x); f12_exp_abs_x(z.ref(), x.ref(), t.ref()); out12(z, out); }
int ps_f12_is_one(const uint64_t *a) { V12 x; in12(a, x); return f12_is_one(x.ref()) ? 1 : 0; }
void ps_final_exp_easy(const uint64_t *a, uint64_t *out) { V12 x, t0, t1; in12(a, x); final_exp_easy(x.ref(), t0.ref(), t1.ref()); out12(x, out); }
void ps_final_exp(const uint64_t *a, uint64_t *out) {
  V12 x, t0, t1, t2, t3;
  in12(a, x);
  final_exp(x.ref(), t0.ref(), t1.ref(), t2.ref(), t3.ref());
  out12(x, out);
}
void ps_f6_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) { out6(f6_mul(in6(a), in6(b)), out); }
void ps_f6_sqr(const uint64_t *a, uint64_t *out) { out6(f6_sqr(in6(a)), out); }
void ps_f6_inv(const uint64_t *a, uint64_t *out) { out6(f6_inv(in6(a)), out); }
// t: Jacobian twist point (X, Y, Z: 36 words, Montgomery conversion inside), replaced by 2 t; line: l0 | l2 | l3
void ps_miller_double(uint64_t *t, const uint64_t *p, uint64_t *line) {
  bls::Jac2 T = {in2(t), in2(t + 12), in2(t + 24)};
  const Line ln = miller_double(T, bls::affine_from_canonical<Fp>((const uint32_t *)p));
  out2(T.x, t); out2(T.y, t + 12); out2(T.z, t + 24);
  out2(ln.l0, line); out2(ln.l2, line + 12); out2(ln.l3, line + 24);
}
void ps_miller_add(uint64_t *t, const uint64_t *q, const uint64_t *p, uint64_t *line) {
  bls::Jac2 T = {in2(t), in2(t + 12), in2(t + 24)};
  const Line ln = miller_add(T, bls::affine_from_canonical<Fp2>((const uint32_t *)q), bls::affine_from_canonical<Fp>((const uint32_t *)p));
  out2(T.x, t); out2(T.y, t + 12); out2(T.z, t + 24);
  out2(ln.l0, line); out2(ln.l2, line + 12); out2(ln.l3, line + 24);
}
void ps_miller_loop(const uint64_t *p, const uint64_t *q, uint64_t *out) {
  V12 f, t;
  miller_loop(f.ref(), t.ref(), bls::affine_from_canonical<Fp>((const uint32_t *)p), bls::affine_from_canonical<Fp2>((const uint32_t *)q));
  out12(f, out);
}
void ps_pairing(const uint64_t *p, const uint64_t *q, uint64_t *out) {
  V12 f, t0, t1, t2, t3;
  miller_loop(f.ref(), t0.ref(), bls::affine_from_canonical<Fp>((const uint32_t *)p), bls::affine_from_canonical<Fp2>((const uint32_t *)q));
  final_exp(f.ref(), t0.ref(), t1.ref(), t2.ref(), t3.ref());
  out12(f, out);
}
int ps_point_status_g1(const uint64_t *xy, int check_torsion) { bls::Affine a; return point_status<Fp>((const uint32_t *)xy, check_torsion != 0, a); }
int ps_point_status_g2(const uint64_t *xy, int check_torsion) { bls::Affine2 a; return point_status<Fp2>((const uint32_t *)xy, check_torsion != 0, a); }
}
