// TEST-ONLY: the __host__ __device__ point conversions of city-rollup_amd/csrc/groth16_keyfile.h built for the CPU, so that the
// exact code the key-file kernels run per lane is held against Python integers without a GPU. Never loaded by the product
// path. A point in the internal form crosses as its affine canonical coordinates (12 / 24 u64).
#include <string.h>

#include "../../city-rollup_amd/csrc/groth16_keyfile.h"

namespace {
using namespace keyfile;

template <class F>
int unpack(const uint8_t *src, int raw, uint64_t *xy, int *is_inf) {
  constexpr int W = Field<F>::WORDS;
  uint32_t w[2 * W];
  memcpy(w, src, (raw ? 2 * W : W) * 4);
  AffineT<F> a = {Field<F>::zero(), Field<F>::zero()};
  bool inf = false;
  const int st = unpack_point<F>(w, raw != 0, a, inf);
  *is_inf = inf ? 1 : 0;
  if (st == ST_OK && !inf) {
    Field<F>::to_canonical(a.x, (uint32_t *)xy);
    Field<F>::to_canonical(a.y, (uint32_t *)xy + W);
  }
  return st;
}
template <class F>
void pack(const uint64_t *xy, int is_inf, int raw, uint8_t *out) {
  constexpr int W = Field<F>::WORDS;
  uint32_t w[2 * W];
  pack_point<F>(bls::affine_from_canonical<F>((const uint32_t *)xy), is_inf != 0, raw != 0, w);
  memcpy(out, w, (raw ? 2 * W : W) * 4);
}
}  // namespace

extern "C" {
// the file's form (48 / 96 bytes, raw: 96 / 192) -> the status class, the infinity flag and, for a finite point, x | y
int ks_unpack_g1(const uint8_t *src, int raw, uint64_t *xy, int *is_inf) { return unpack<Fp>(src, raw, xy, is_inf); }
int ks_unpack_g2(const uint8_t *src, int raw, uint64_t *xy, int *is_inf) { return unpack<Fp2>(src, raw, xy, is_inf); }
// x | y and the flag -> the file's form
void ks_pack_g1(const uint64_t *xy, int is_inf, int raw, uint8_t *out) { pack<Fp>(xy, is_inf, raw, out); }
void ks_pack_g2(const uint64_t *xy, int is_inf, int raw, uint8_t *out) { pack<Fp2>(xy, is_inf, raw, out); }
}
