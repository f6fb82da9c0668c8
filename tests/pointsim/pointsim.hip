// TEST-ONLY: the host-callable pieces of the point transforms and of the SRS setup (city-rollup_amd/csrc/point_ntt.h: the
// 256-bit scalar multiplication on operands in memory, the butterfly and twiddle indexing, the bit reversal; groth16_srs.h: the
// same multiplication over an affine operand) built for the CPU, so that the exact code the kernels run is checked against the
// oracle and Python integers without a GPU. Never loaded by the product path.
#include "../../city-rollup_amd/csrc/groth16_srs.h"

namespace {
// k * P through form 0 (Jacobian operand, pointntt::jac_mul_u256_at) or 1 (affine operand, g16srs::affine_mul_u256_at)
template <class F>
int mul(int form, const uint64_t *xy, int inf, const uint64_t *k, uint64_t *out_xy) {
  const bls::AffineT<F> a = bls::affine_from_canonical<F>((const uint32_t *)xy);
  bls::JacT<F> p = inf ? bls::jac_inf<F>() : bls::JacT<F>{a.x, a.y, bls::Field<F>::one()}, r;
  if (form == 0) pointntt::jac_mul_u256_at<F>(&r, &p, (const uint32_t *)k);
  else g16srs::affine_mul_u256_at<F>(&r, &a, (const uint32_t *)k);
  return bls::jac_to_affine_canonical(r, (uint32_t *)out_xy) ? 1 : 0;
}
}  // namespace

extern "C" {
int ps_g1_mul(int form, const uint64_t *xy, int inf, const uint64_t *k, uint64_t *out_xy) { return mul<bls::Fp>(form, xy, inf, k, out_xy); }
int ps_g2_mul(int form, const uint64_t *xy, int inf, const uint64_t *k, uint64_t *out_xy) { return mul<bls::Fp2>(form, xy, inf, k, out_xy); }
int ps_top_bit(const uint64_t *k) { return pointntt::top_bit((const uint32_t *)k); }
// out = (lo, hi, twiddle exponent) of butterfly t of stage s
void ps_butterfly(uint64_t t, int s, int log_n, uint64_t *out) {
  const pointntt::Butterfly b = pointntt::butterfly((size_t)t, s, log_n);
  out[0] = b.lo;
  out[1] = b.hi;
  out[2] = b.twiddle;
}
uint64_t ps_bit_reverse(uint64_t i, int log_n) { return pointntt::bit_reverse((size_t)i, log_n); }
int ps_results_per_lane(void) { return pointntt::K; }
}
