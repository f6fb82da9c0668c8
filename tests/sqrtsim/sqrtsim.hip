// TEST-ONLY: the __host__ __device__ square roots and element decoding of city-rollup_amd/csrc/bls_sqrt.h built for the CPU, so
// that the exact code the kernels run is held against Python integers without a GPU. Never loaded by the product path. Every
// value crosses as canonical little-endian u64 words: 6 per F_p element, F_p^2 as c0 | c1.
#include <string.h>

#include "../../city-rollup_amd/csrc/bls_sqrt.h"

namespace {
using namespace blssqrt;
Fp in1(const uint64_t *w) { return bls::fp_from_canonical((const uint32_t *)w); }
Fp2 in2(const uint64_t *w) { return bls::Field<Fp2>::from_canonical((const uint32_t *)w); }
}  // namespace

extern "C" {
// 1 and the root in `out` where a has one, else 0 (out untouched)
int ss_fp_sqrt(const uint64_t *a, uint64_t *out) {
  Fp r;
  if (!fp_sqrt(in1(a), &r)) return 0;
  bls::fp_to_canonical(r, (uint32_t *)out);
  return 1;
}
int ss_fp2_sqrt(const uint64_t *a, uint64_t *out) {
  Fp2 r;
  if (!fp2_sqrt(in2(a), &r)) return 0;
  bls::Field<Fp2>::to_canonical(r, (uint32_t *)out);
  return 1;
}
int ss_fp_is_larger(const uint64_t *y) { return fp_is_larger(in1(y)) ? 1 : 0; }
int ss_fp2_is_larger(const uint64_t *y) { return fp2_is_larger(in2(y)) ? 1 : 0; }
void ss_fp_half(const uint64_t *a, uint64_t *out) { bls::fp_to_canonical(fp_half(in1(a)), (uint32_t *)out); }
void ss_fp_pow_p34(const uint64_t *a, uint64_t *out) { bls::fp_to_canonical(fp_pow_p34(in1(a)), (uint32_t *)out); }
// a compressed element as stored (48 / 96 bytes) -> the status class and, for 0, x | y (12 / 24 u64)
int ss_g1_decompress(const uint8_t *src, uint64_t *xy) {
  uint32_t w[12];
  memcpy(w, src, sizeof w);
  return g1_decompress(w, (uint32_t *)xy);
}
int ss_g2_decompress(const uint8_t *src, uint64_t *xy) {
  uint32_t w[24];
  memcpy(w, src, sizeof w);
  return g2_decompress(w, (uint32_t *)xy);
}
}
