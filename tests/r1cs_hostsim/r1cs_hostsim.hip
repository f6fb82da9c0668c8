// TEST-ONLY: the __host__ __device__ arithmetic of city-rollup_amd/csrc/r1cs.h instantiated on the host, so that the exact
// formulas the kernels run (limb split, term classes, the one-limb product and its quotient estimate) are checked against
// Python integers on the CPU. Never loaded by the product path.
#include "../../city-rollup_amd/csrc/r1cs.h"

extern "C" {
// out = c * w mod r, c one limb, w canonical
void hs_r1cs_mul_small(const uint64_t *w, uint32_t c, uint64_t *out) {
  r1cs::join_words(r1cs::mul_small(r1cs::split_words((const uint32_t *)w), c), (uint32_t *)out);
}
uint32_t hs_r1cs_classify(const uint64_t *c, uint32_t *small) { return r1cs::classify(c, small); }
// out = acc + c * w mod r the way a kernel does it: c classified, its table entry in Montgomery form, acc and w canonical limbs
void hs_r1cs_term(const uint64_t *acc, const uint64_t *c, const uint64_t *w, uint64_t *out) {
  uint32_t small = 0;
  const uint32_t cls = r1cs::classify(c, &small);
  const blsfr::Fr a = r1cs::split_words((const uint32_t *)acc);
  if (cls == r1cs::CLS_ZERO) { r1cs::join_words(a, (uint32_t *)out); return; }  // dropped at create
  const blsfr::Fr table[1] = {blsfr::fr_from_canonical((const uint32_t *)c)};
  r1cs::join_words(r1cs::apply_class(a, cls, cls == r1cs::CLS_GENERAL ? 0 : small, table, r1cs::split_words((const uint32_t *)w)), (uint32_t *)out);
}
}
