// TEST-ONLY: one element of every BLS12-381 wrapper of hostsim (`hs_bls_*`, `hs_r1cs_mul_small`) and of its device twin
// (tests/devsim `ds_bls_*`), as __host__ __device__ functions: op codes and argument layouts exist once.
#pragma once
#include "../../city-rollup_amd/csrc/bls12_381.h"
#include "../../city-rollup_amd/csrc/bls12_381_fr.h"
#include "../../city-rollup_amd/csrc/r1cs.h"

namespace sim {

// canonical 12-word operands -> canonical (a*b mod p, a+b, a-b by op 0/1/2; 3: a^-1; 4: a^2 by the dedicated square)
GL_HD void bls_fp_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  bls::Fp x = bls::fp_from_canonical(a), y = bls::fp_from_canonical(b), r;
  switch (op) {
    case 0: r = bls::fp_mul(x, y); break;
    case 1: r = bls::fp_add(x, y); break;
    case 2: r = bls::fp_sub(x, y); break;
    case 4: r = bls::fp_sqr_mont(x); break;
    default: r = bls::fp_inv(x); break;
  }
  bls::fp_to_canonical(r, out);
}
// F_p^2: 24-word operands (c0, c1); op 0 mul, 1 sqr, 2 inv
GL_HD void bls_fp2_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  using F2 = bls::Field<bls::Fp2>;
  bls::Fp2 x = F2::from_canonical(a), y = F2::from_canonical(b), r;
  switch (op) {
    case 0: r = bls::fp2_mul(x, y); break;
    case 1: r = bls::fp2_sqr(x); break;
    default: r = bls::fp2_inv(x); break;
  }
  F2::to_canonical(r, out);
}
// op 0: general add (both lifted to Jacobian, p scaled to a non-trivial z first), 1: mixed add, 2: double p, 3: p * k
template <class F>
GL_HD int group_op(int op, const uint32_t *p_xy, int p_inf, const uint32_t *q_xy, int q_inf, uint32_t k, uint32_t *out_xy) {
  using Fd = bls::Field<F>;
  bls::JacT<F> p = bls::jac_inf<F>(), q = bls::jac_inf<F>(), r;
  bls::AffineT<F> qa = bls::affine_from_canonical<F>(q_xy);
  if (!p_inf) {  // give p a z != 1 so the projective formulas are exercised: (x z^2, y z^3, z), z = 3
    const bls::AffineT<F> pa = bls::affine_from_canonical<F>(p_xy);
    const F z = bls::f_add(Fd::one(), bls::f_add(Fd::one(), Fd::one())), z2 = bls::f_sqr(z);
    p = {bls::f_mul(pa.x, z2), bls::f_mul(pa.y, bls::f_mul(z2, z)), z};
  }
  if (!q_inf) q = {qa.x, qa.y, Fd::one()};
  switch (op) {
    case 0: r = bls::jac_add(p, q); break;
    case 1: r = q_inf ? p : bls::jac_add_mixed(p, qa); break;
    case 2: r = bls::jac_double(p); break;
    default: r = bls::jac_mul_small(p, k); break;
  }
  return bls::jac_to_affine_canonical(r, out_xy) ? 1 : 0;
}
// the bucket accumulation on loose (bounded, unreduced) values: sum of n affine points (xy: n x 2 x WORDS canonical words,
// none at infinity) through xyzz_add_mixed_loose, result canonical affine; returns 1 for infinity
template <class F>
GL_HD int bucket_chain(const uint32_t *xy, size_t n, uint32_t *out_xy) {
  constexpr int W = bls::Field<F>::WORDS;
  bls::XyzzT<F> acc = bls::xyzz_inf<F>();
  for (size_t i = 0; i < n; i++) acc = bls::xyzz_add_mixed_loose(acc, bls::affine_from_canonical<F>(xy + 2 * W * i));
  return bls::jac_to_affine_canonical(bls::xyzz_to_jac_loose(acc), out_xy) ? 1 : 0;
}
// loose field primitives against Python integers: op 0 lz_mul, 1 lz_add, 2 lz_sub<8>, 3 lz_weak<16>, 4 lz_canon; a, b: 14 raw limbs
GL_HD void bls_lz_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  bls::Fp x, y, r;
  for (int i = 0; i < bls::NL; i++) x.l[i] = a[i], y.l[i] = b[i];
  switch (op) {
    case 0: r = bls::lz_mul(x, y); break;
    case 1: r = bls::lz_add(x, y); break;
    case 2: r = bls::lz_sub<8>(x, y); break;
    case 3: r = bls::lz_weak<16>(x); break;
    default: r = bls::lz_canon(x); break;
  }
  for (int i = 0; i < bls::NL; i++) out[i] = r.l[i];
}
GL_HD int bls_lz_maybe_zero(const uint32_t *a) {
  bls::Fp x;
  for (int i = 0; i < bls::NL; i++) x.l[i] = a[i];
  return bls::lz_maybe_zero(x) ? 1 : 0;
}
// ---- what tests/bls_rare_paths.py restates, on raw limbs ----
// one xyzz_add_mixed_loose: acc = x, y, zz, zzz as raw 28-bit limbs (NL per F_p component), q canonical words. Returns which
// way the addition went, decided with the same primitives the addition itself uses:
// 0 first point, 1 loose general, 2 doubling, 3 cancellation, 4 loose general after the filter passed on a non-zero difference
template <class F>
GL_HD int loose_step(const uint32_t *acc_limbs, const uint32_t *q_xy, uint32_t *out_limbs) {
  using B = bls::LooseBound<F>;
  bls::XyzzT<F> p;
  static_assert(sizeof(p) == 4 * sizeof(F) && sizeof(F) % sizeof(bls::Fp) == 0, "an accumulator is nothing but limbs");
  __builtin_memcpy(&p, acc_limbs, sizeof p);
  const bls::AffineT<F> q = bls::affine_from_canonical<F>(q_xy);
  int way = 0;
  if (!bls::f_is_zero(p.zz)) {
    const F pp_ = bls::lf_sub<B::X>(bls::lf_mul(q.x, p.zz), p.x);
    const bool maybe = bls::lf_maybe_zero(pp_), zero = bls::f_is_zero(bls::lf_canon(pp_));
    if (zero) way = bls::f_eq(bls::lf_canon(p.y), bls::f_mul(q.y, bls::lf_canon(p.zzz))) ? 2 : 3;
    else way = maybe ? 4 : 1;
    if (zero && !maybe) way = -1;  // the filter is a necessary condition
  }
  const bls::XyzzT<F> r = bls::xyzz_add_mixed_loose(p, q);
  __builtin_memcpy(out_limbs, &r, sizeof r);
  return way;
}
// the accumulator as the kernels hand it on: canonical affine words; returns 1 for infinity
template <class F>
GL_HD int loose_out(const uint32_t *acc_limbs, uint32_t *out_xy) {
  bls::XyzzT<F> p;
  __builtin_memcpy(&p, acc_limbs, sizeof p);
  return bls::jac_to_affine_canonical(bls::xyzz_to_jac_loose(p), out_xy) ? 1 : 0;
}
// raw limbs in, raw limbs out: op 0 fp_mul, 1 lz_mul, 2 lz_sqr (of a), 3 fp_sqr_mont (of a), 4 lz_add_nc
GL_HD void bls_fp_raw(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  bls::Fp x, y, r;
  for (int i = 0; i < bls::NL; i++) x.l[i] = a[i], y.l[i] = b[i];
  switch (op) {
    case 0: r = bls::fp_mul(x, y); break;
    case 1: r = bls::lz_mul(x, y); break;
    case 2: r = bls::lz_sqr(x); break;
    case 3: r = bls::fp_sqr_mont(x); break;
    default: r = bls::lz_add_nc(x, y); break;
  }
  for (int i = 0; i < bls::NL; i++) out[i] = r.l[i];
}
// lz_sub<K> / lz_weak<K> for every K the two accumulations use; returns -1 for any other
#define SIM_K(K) case K: r = weak ? bls::lz_weak<K>(x) : bls::lz_sub<K>(x, y); break;
GL_HD int bls_lz_k(int weak, int K, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  bls::Fp x, y, r;
  for (int i = 0; i < bls::NL; i++) x.l[i] = a[i], y.l[i] = b[i];
  switch (K) {
    SIM_K(2) SIM_K(4) SIM_K(6) SIM_K(8) SIM_K(10) SIM_K(12) SIM_K(16) SIM_K(18) SIM_K(22)
    default: return -1;
  }
  for (int i = 0; i < bls::NL; i++) out[i] = r.l[i];
  return 0;
}
#undef SIM_K

// ---- BLS12-381 scalar field (csrc/bls12_381_fr.h) ----
// 8-word canonical operands; op 0 mul, 1 add, 2 sub, 3 inverse of a, 4 a^(b[0] + 2^32 b[1])
GL_HD void bls_fr_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  blsfr::Fr x = blsfr::fr_from_canonical(a), y = blsfr::fr_from_canonical(b), r;
  switch (op) {
    case 0: r = blsfr::fr_mul(x, y); break;
    case 1: r = blsfr::fr_add(x, y); break;
    case 2: r = blsfr::fr_sub(x, y); break;
    case 3: r = blsfr::fr_inv(x); break;
    default: r = blsfr::fr_pow_u64(x, ((uint64_t)b[1] << 32) | b[0]); break;
  }
  blsfr::fr_to_canonical(r, out);
}
// raw limbs in, raw limbs out: op 0 fr_mul, 1 fr_add, 2 fr_sub, 3 fr_from_canonical (a: 8 words in an array of NL)
GL_HD void bls_fr_raw(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
  blsfr::Fr x = blsfr::fr_zero(), y, r;
  if (op != 3) for (int i = 0; i < blsfr::NL; i++) x.l[i] = a[i];
  for (int i = 0; i < blsfr::NL; i++) y.l[i] = b[i];
  switch (op) {
    case 0: r = blsfr::fr_mul(x, y); break;
    case 1: r = blsfr::fr_add(x, y); break;
    case 2: r = blsfr::fr_sub(x, y); break;
    default: r = blsfr::fr_from_canonical(a); break;
  }
  for (int i = 0; i < blsfr::NL; i++) out[i] = r.l[i];
}
// ---- r1cs.h: the one-limb product ----
GL_HD void r1cs_mul_small(const uint32_t *w, uint32_t c, uint32_t *out) {
  blsfr::Fr x, r;
  for (int i = 0; i < blsfr::NL; i++) x.l[i] = w[i];
  r = r1cs::mul_small(x, c);
  for (int i = 0; i < blsfr::NL; i++) out[i] = r.l[i];
}

}  // namespace sim
