// TEST-ONLY: the host-callable per-lane code of g16srs::k_scale_each (city-rollup_amd/csrc/groth16_srs.h: the scalar a lane
// takes for entry k of an SRS array under a contribution (t, a, b), and the multiplication it steers) built for the CPU, so that
// the exact code the kernel runs is checked against the oracle and Python integers without a GPU. Never loaded by the product
// path.
#include "../../city-rollup_amd/csrc/groth16_srs.h"

#include <vector>

namespace {
using blsfr::Fr;
enum { TAU_G1 = 0, TAU_G2 = 1, ALPHA_TAU_G1 = 2, BETA_TAU_G1 = 3 };

// the table the library fills with frntt::k_powers (fr_pow_u64 per entry) and the three selections contribute_run makes of it
struct Selection {
  std::vector<Fr> powers;
  g16srs::EachScalar S;
  Selection(int array, size_t count, const uint64_t *t, const uint64_t *a, const uint64_t *b) : powers(count) {
    const Fr tf = blsfr::fr_from_canonical((const uint32_t *)t);
    for (size_t i = 0; i < count; i++) powers[i] = blsfr::fr_pow_u64(tf, i);
    if (array == ALPHA_TAU_G1) S = {powers.data(), blsfr::fr_from_canonical((const uint32_t *)a), 1};
    else if (array == BETA_TAU_G1) S = {powers.data(), blsfr::fr_from_canonical((const uint32_t *)b), 1};
    else S = {powers.data(), tf, 0};
  }
};

// out = scalar(k) * pts[k] for a one-entry-per-k array that holds the same point everywhere but at k (a poisoned neighbour
// on either side shows a lane that reads the wrong entry)
template <class F>
int lane(int array, uint64_t k, uint64_t count, const uint64_t *t, const uint64_t *a, const uint64_t *b, const uint64_t *xy, const uint64_t *other_xy,
         uint64_t *out_xy) {
  const Selection sel(array, (size_t)count, t, a, b);
  std::vector<bls::AffineT<F>> pts((size_t)count, bls::affine_from_canonical<F>((const uint32_t *)other_xy));
  pts[(size_t)k] = bls::affine_from_canonical<F>((const uint32_t *)xy);
  bls::JacT<F> prod;
  uint32_t ks[pointntt::SCALAR_WORDS];
  g16srs::scale_each_lane<F>(&prod, ks, pts.data(), (size_t)k, sel.S);
  return bls::jac_to_affine_canonical(prod, (uint32_t *)out_xy) ? 1 : 0;
}
}  // namespace

extern "C" {
// the canonical scalar of entry k of `array` (0 tau_g1, 1 tau_g2, 2 alpha_tau_g1, 3 beta_tau_g1) into out[4]
void sp_each_scalar(int array, uint64_t k, uint64_t count, const uint64_t *t, const uint64_t *a, const uint64_t *b, uint64_t *out) {
  const Selection sel(array, (size_t)count, t, a, b);
  g16srs::each_scalar(sel.S, (size_t)k, (uint32_t *)out);
}
int sp_g1_lane(int array, uint64_t k, uint64_t count, const uint64_t *t, const uint64_t *a, const uint64_t *b, const uint64_t *xy, const uint64_t *other_xy,
               uint64_t *out_xy) {
  return lane<bls::Fp>(array, k, count, t, a, b, xy, other_xy, out_xy);
}
int sp_g2_lane(int array, uint64_t k, uint64_t count, const uint64_t *t, const uint64_t *a, const uint64_t *b, const uint64_t *xy, const uint64_t *other_xy,
               uint64_t *out_xy) {
  return lane<bls::Fp2>(array, k, count, t, a, b, xy, other_xy, out_xy);
}
}
