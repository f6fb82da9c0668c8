// TEST-ONLY: the device twin of the BLS12-381 part of tests/hostsim/hostsim.hip (bls12_381.h, bls12_381_fr.h, the one-limb product
// of r1cs.h): every `hs_bls_*` / `hs_r1cs_mul_small` has a `ds_*` here that applies the same element-wise body
// (../hostsim/sim_bls.h) to arrays on the device, under a per-element mask (devsim.h). Arguments: the ones of the `hs_*` entry as
// arrays of n elements, then mask, then n; a value the `hs_*` entry returns goes into `ret`; the return value is the hipError_t.
// Never loaded by the product path.
#include "devsim.h"
#include "../hostsim/sim_bls.h"

namespace devsim {
int unit_init() { return 0; }
}  // namespace devsim
using devsim::Job;
typedef const uint8_t *mask_t;
typedef const uint32_t *in_t;

// a, b, out: n x WORDS
template <int WORDS, class F>
static int binary(F f, int op, in_t a, in_t b, uint32_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  in_t da = j.in(a, WORDS * n), db = j.in(b, WORDS * n);
  uint32_t *o = j.inout(out, WORDS * n);
  return j.run(DS_EACH { f(op, da + WORDS * i, db + WORDS * i, o + WORDS * i); });
}
struct FpOp { __device__ void operator()(int op, in_t a, in_t b, uint32_t *o) const { sim::bls_fp_op(op, a, b, o); } };
struct Fp2Op { __device__ void operator()(int op, in_t a, in_t b, uint32_t *o) const { sim::bls_fp2_op(op, a, b, o); } };
struct LzOp { __device__ void operator()(int op, in_t a, in_t b, uint32_t *o) const { sim::bls_lz_op(op, a, b, o); } };
struct FpRaw { __device__ void operator()(int op, in_t a, in_t b, uint32_t *o) const { sim::bls_fp_raw(op, a, b, o); } };
struct FrOp { __device__ void operator()(int op, in_t a, in_t b, uint32_t *o) const { sim::bls_fr_op(op, a, b, o); } };
struct FrRaw { __device__ void operator()(int op, in_t a, in_t b, uint32_t *o) const { sim::bls_fr_raw(op, a, b, o); } };

// p_xy, q_xy, out_xy: n x 2 WORDS; p_inf, q_inf, k per element
template <class F>
static int group(int op, in_t p_xy, const int *p_inf, in_t q_xy, const int *q_inf, in_t k, uint32_t *out_xy, int *ret, mask_t mask, size_t n) {
  constexpr int W2 = 2 * bls::Field<F>::WORDS;
  Job j(mask, n);
  in_t dp = j.in(p_xy, W2 * n), dq = j.in(q_xy, W2 * n), dk = j.in(k, n);
  const int *dpi = j.in(p_inf, n), *dqi = j.in(q_inf, n);
  uint32_t *o = j.inout(out_xy, W2 * n);
  int *r = j.inout(ret, n);
  return j.run(DS_EACH { r[i] = sim::group_op<F>(op, dp + W2 * i, dpi[i], dq + W2 * i, dqi[i], dk[i], o + W2 * i); });
}
// every element sums the same number of points: xy: n x count x 2 WORDS
template <class F>
static int chain(in_t xy, size_t count, uint32_t *out_xy, int *ret, mask_t mask, size_t n) {
  constexpr int W2 = 2 * bls::Field<F>::WORDS;
  Job j(mask, n);
  in_t d = j.in(xy, W2 * count * n);
  uint32_t *o = j.inout(out_xy, W2 * n);
  int *r = j.inout(ret, n);
  return j.run(DS_EACH { r[i] = sim::bucket_chain<F>(d + W2 * count * i, count, o + W2 * i); });
}
template <class F>
static int loose_step(in_t acc, in_t q_xy, uint32_t *out, int *ret, mask_t mask, size_t n) {
  constexpr int W2 = 2 * bls::Field<F>::WORDS, A = sizeof(bls::XyzzT<F>) / 4;
  Job j(mask, n);
  in_t da = j.in(acc, A * n), dq = j.in(q_xy, W2 * n);
  uint32_t *o = j.inout(out, A * n);
  int *r = j.inout(ret, n);
  return j.run(DS_EACH { r[i] = sim::loose_step<F>(da + A * i, dq + W2 * i, o + A * i); });
}
template <class F>
static int loose_out(in_t acc, uint32_t *out_xy, int *ret, mask_t mask, size_t n) {
  constexpr int W2 = 2 * bls::Field<F>::WORDS, A = sizeof(bls::XyzzT<F>) / 4;
  Job j(mask, n);
  in_t da = j.in(acc, A * n);
  uint32_t *o = j.inout(out_xy, W2 * n);
  int *r = j.inout(ret, n);
  return j.run(DS_EACH { r[i] = sim::loose_out<F>(da + A * i, o + W2 * i); });
}

extern "C" {
int ds_bls_fp_op(int op, in_t a, in_t b, uint32_t *out, mask_t mask, size_t n) { return binary<12>(FpOp(), op, a, b, out, mask, n); }
int ds_bls_fp2_op(int op, in_t a, in_t b, uint32_t *out, mask_t mask, size_t n) { return binary<24>(Fp2Op(), op, a, b, out, mask, n); }
int ds_bls_lz_op(int op, in_t a, in_t b, uint32_t *out, mask_t mask, size_t n) { return binary<bls::NL>(LzOp(), op, a, b, out, mask, n); }
int ds_bls_fp_raw(int op, in_t a, in_t b, uint32_t *out, mask_t mask, size_t n) { return binary<bls::NL>(FpRaw(), op, a, b, out, mask, n); }
int ds_bls_fr_op(int op, in_t a, in_t b, uint32_t *out, mask_t mask, size_t n) { return binary<8>(FrOp(), op, a, b, out, mask, n); }
int ds_bls_fr_raw(int op, in_t a, in_t b, uint32_t *out, mask_t mask, size_t n) { return binary<blsfr::NL>(FrRaw(), op, a, b, out, mask, n); }
int ds_bls_lz_maybe_zero(in_t a, int *ret, mask_t mask, size_t n) {
  Job j(mask, n);
  in_t da = j.in(a, bls::NL * n);
  int *r = j.inout(ret, n);
  return j.run(DS_EACH { r[i] = sim::bls_lz_maybe_zero(da + bls::NL * i); });
}
// K per element (the switch over it diverges inside a wave)
int ds_bls_lz_k(int weak, const int *K, in_t a, in_t b, uint32_t *out, int *ret, mask_t mask, size_t n) {
  Job j(mask, n);
  in_t da = j.in(a, bls::NL * n), db = j.in(b, bls::NL * n);
  const int *dk = j.in(K, n);
  uint32_t *o = j.inout(out, bls::NL * n);
  int *r = j.inout(ret, n);
  return j.run(DS_EACH { r[i] = sim::bls_lz_k(weak, dk[i], da + bls::NL * i, db + bls::NL * i, o + bls::NL * i); });
}
int ds_bls_g1_op(int op, in_t p_xy, const int *p_inf, in_t q_xy, const int *q_inf, in_t k, uint32_t *out_xy, int *ret, mask_t mask, size_t n) {
  return group<bls::Fp>(op, p_xy, p_inf, q_xy, q_inf, k, out_xy, ret, mask, n);
}
int ds_bls_g2_op(int op, in_t p_xy, const int *p_inf, in_t q_xy, const int *q_inf, in_t k, uint32_t *out_xy, int *ret, mask_t mask, size_t n) {
  return group<bls::Fp2>(op, p_xy, p_inf, q_xy, q_inf, k, out_xy, ret, mask, n);
}
int ds_bls_g1_chain(in_t xy, size_t count, uint32_t *out_xy, int *ret, mask_t mask, size_t n) { return chain<bls::Fp>(xy, count, out_xy, ret, mask, n); }
int ds_bls_g2_chain(in_t xy, size_t count, uint32_t *out_xy, int *ret, mask_t mask, size_t n) { return chain<bls::Fp2>(xy, count, out_xy, ret, mask, n); }
int ds_bls_g1_loose_step(in_t acc, in_t q_xy, uint32_t *out, int *ret, mask_t mask, size_t n) { return loose_step<bls::Fp>(acc, q_xy, out, ret, mask, n); }
int ds_bls_g2_loose_step(in_t acc, in_t q_xy, uint32_t *out, int *ret, mask_t mask, size_t n) { return loose_step<bls::Fp2>(acc, q_xy, out, ret, mask, n); }
int ds_bls_g1_loose_out(in_t acc, uint32_t *out_xy, int *ret, mask_t mask, size_t n) { return loose_out<bls::Fp>(acc, out_xy, ret, mask, n); }
int ds_bls_g2_loose_out(in_t acc, uint32_t *out_xy, int *ret, mask_t mask, size_t n) { return loose_out<bls::Fp2>(acc, out_xy, ret, mask, n); }
int ds_r1cs_mul_small(in_t w, in_t c, uint32_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  in_t dw = j.in(w, blsfr::NL * n), dc = j.in(c, n);
  uint32_t *o = j.inout(out, blsfr::NL * n);
  return j.run(DS_EACH { sim::r1cs_mul_small(dw + blsfr::NL * i, dc[i], o + blsfr::NL * i); });
}
}
