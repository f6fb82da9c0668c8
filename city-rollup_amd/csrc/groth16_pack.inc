// The Groth16 proof as the worker stores it: `CityGroth16ProofData { pi_a, pi_b_a0, pi_b_a1, pi_c }`, four 48-byte
// `Serialized2DFeltBLS12381` (city_rollup_common/src/block_template/data.rs:6-34; produced from gnark's JSON at
// city_rollup_circuit/src/worker/toolbox/root.rs:296-315, stored by city_rollup_core_worker/src/actors/simple.rs:74-81,
// pushed on chain for OP_CHECKGROTH16VERIFY by `encode_witness_script`, data.rs:48-62).
//
// Encoding — PINNED on the two reference samples at data.rs:72-73 (tests/test_groth16_pack.py): each element is the
// compressed form of a curve point, x little-endian with the flags in the two top bits of the LAST byte
// (0x80: y is the larger of {y, -y}; 0x40: point at infinity) — the arkworks `serialize_compressed` layout. pi_a and pi_c
// are G1 points (48 bytes); pi_b is ONE G2 point whose x = a0 + a1 u is split into pi_b_a0 = a0 (no flag bits) and
// pi_b_a1 = a1 (carrying the flags). Decompressing the eight sample elements gives points on the curve AND in the
// r-torsion subgroup (a random x fails that with probability 1 - 2^-126), and the (a1, a0) order does not even give a
// point on the twist: byte order, flag position and the a0 / a1 order are reference-held facts. What the samples cannot
// pin is which root the 0x80 flag names; this follows arkworks 0.4 (`y > -y`, F_p^2 compared by c1 then c0).
// Host-only arithmetic (no GPU): included by bls.hip after msm.inc.
#include "bls_sqrt.h"

namespace g16pack {

// the square roots and the "larger root" predicates: bls_sqrt.h, shared with the kernels of pairing.hip
using blssqrt::fp_sqrt;
using blssqrt::fp2_sqrt;
using blssqrt::fp_is_larger;
using blssqrt::fp2_is_larger;

}  // namespace g16pack

extern "C" {

int cp_groth16_proof_pack_city(const uint64_t a_xy[12], const uint64_t b_xy[24], const uint64_t c_xy[12], uint8_t out[192]) try {
  if (!a_xy || !b_xy || !c_xy || !out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  const uint32_t *wa = (const uint32_t *)a_xy, *wb = (const uint32_t *)b_xy, *wc = (const uint32_t *)c_xy;
  for (int h = 0; h < 2; h++)
    if (!canonical_words(wa + 12 * h) || !canonical_words(wc + 12 * h)) return set_error(nullptr, CP_ERR_INVALID_ARG, "G1 coordinate is not canonical (>= p)");
  for (int h = 0; h < 4; h++)
    if (!canonical_words(wb + 12 * h)) return set_error(nullptr, CP_ERR_INVALID_ARG, "G2 coordinate is not canonical (>= p)");
  const bls::AffineT<bls::Fp> A = bls::affine_from_canonical<bls::Fp>(wa), C = bls::affine_from_canonical<bls::Fp>(wc);
  const bls::AffineT<bls::Fp2> B = bls::affine_from_canonical<bls::Fp2>(wb);
  if (!bls::affine_on_curve(A) || !bls::affine_on_curve(C)) return set_error(nullptr, CP_ERR_INVALID_ARG, "pi_a / pi_c is not on the curve");
  if (!bls::affine_on_curve(B)) return set_error(nullptr, CP_ERR_INVALID_ARG, "pi_b is not on the twist");
  memcpy(out, wa, 48);         // pi_a: x little-endian
  memcpy(out + 48, wb, 48);    // pi_b_a0: x.c0
  memcpy(out + 96, wb + 12, 48);  // pi_b_a1: x.c1
  memcpy(out + 144, wc, 48);   // pi_c
  if (g16pack::fp_is_larger(A.y)) out[47] |= 0x80;
  if (g16pack::fp2_is_larger(B.y)) out[143] |= 0x80;
  if (g16pack::fp_is_larger(C.y)) out[191] |= 0x80;
  return CP_OK;
} CP_CATCH(nullptr)

int cp_groth16_proof_unpack_city(const uint8_t in[192], uint64_t a_xy[12], uint64_t b_xy[24], uint64_t c_xy[12]) try {
  if (!in || !a_xy || !b_xy || !c_xy) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  if ((in[47] | in[143] | in[191]) & 0x40) return set_error(nullptr, CP_ERR_INVALID_ARG, "a proof element is the point at infinity");
  if (in[95] & 0xC0) return set_error(nullptr, CP_ERR_INVALID_ARG, "pi_b_a0 carries flag bits");
  auto g1 = [&](const uint8_t *src, uint64_t *xy, const char *name) -> int {
    uint8_t x[48];
    memcpy(x, src, 48);
    const bool larger = x[47] & 0x80;
    x[47] &= 0x3F;
    uint32_t w[12];
    memcpy(w, x, 48);
    if (!canonical_words(w)) return set_error(nullptr, CP_ERR_INVALID_ARG, "%s: x is not canonical (>= p)", name);
    const bls::Fp X = bls::fp_from_canonical(w);
    bls::Fp Y;
    if (!g16pack::fp_sqrt(bls::fp_add(bls::fp_mul(bls::fp_sqr(X), X), bls::Field<bls::Fp>::curve_b()), &Y))
      return set_error(nullptr, CP_ERR_INVALID_ARG, "%s: x is not the abscissa of a curve point", name);
    if (g16pack::fp_is_larger(Y) != larger) Y = bls::fp_sub(bls::fp_zero(), Y);
    memcpy(xy, w, 48);
    bls::fp_to_canonical(Y, (uint32_t *)xy + 12);
    return CP_OK;
  };
  CP_TRY(g1(in, a_xy, "pi_a"));
  CP_TRY(g1(in + 144, c_xy, "pi_c"));
  uint8_t x1[48];
  memcpy(x1, in + 96, 48);
  const bool larger = x1[47] & 0x80;
  x1[47] &= 0x3F;
  uint32_t w[24];
  memcpy(w, in + 48, 48);
  memcpy(w + 12, x1, 48);
  if (!canonical_words(w) || !canonical_words(w + 12)) return set_error(nullptr, CP_ERR_INVALID_ARG, "pi_b: x is not canonical (>= p)");
  const bls::Fp2 X = bls::Field<bls::Fp2>::from_canonical(w);
  bls::Fp2 Y;
  if (!g16pack::fp2_sqrt(bls::fp2_add(bls::fp2_mul(bls::fp2_sqr(X), X), bls::Field<bls::Fp2>::curve_b()), &Y))
    return set_error(nullptr, CP_ERR_INVALID_ARG, "pi_b: x is not the abscissa of a point of the twist");
  if (g16pack::fp2_is_larger(Y) != larger) Y = bls::fp2_sub(bls::Field<bls::Fp2>::zero(), Y);
  memcpy(b_xy, w, 96);
  bls::Field<bls::Fp2>::to_canonical(Y, (uint32_t *)b_xy + 24);
  return CP_OK;
} CP_CATCH(nullptr)

}  // extern "C"
