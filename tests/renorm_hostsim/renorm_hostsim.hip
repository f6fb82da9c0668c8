// TEST-ONLY: the partial rounds' carry normalisation in units of 2^32 (city-rollup_amd/csrc/poseidon.h `renorm32_d`), the two forms of
// its constants through `recombine_d`, and the four permutation forms, instantiated on the host. Never loaded by the product path.
// The element-wise bodies are in ../hostsim/sim_gl.h, shared with the device twins (tests/devsim).
#include "../hostsim/sim_gl.h"

extern "C" {
int hs_rn_units32() { return poseidon::UNITS32 ? 1 : 0; }
// which: 0 renorm32_d (planes in units of 2^32), 1 renorm_d (units of 1)
void hs_rn_renorm(int which, const double *in, double *out) { sim::renorm(which, in, out); }
// recombine_d on limbs l, h with entry i of a table. table: 0 POSEIDON_DOMD_K, 1 POSEIDON_DOMD_LAST (limbs in units of 1),
// 2 POSEIDON_DOMD32_K, 3 POSEIDON_DOMD32_LAST (limbs in units of 2^32: the caller passes l 2^-32, h 2^-32)
uint64_t hs_rn_recombine(double l, double h, int table, int i) {
  const uint64_t *t = table == 0 ? POSEIDON_DOMD_K : table == 1 ? POSEIDON_DOMD_LAST : table == 2 ? POSEIDON_DOMD32_K : POSEIDON_DOMD32_LAST;
  return sim::recombine_bits(l, h, t[2 * i], t[2 * i + 1]);
}
// states: n x 12 in place. form: 0 permute, 1 permute_absorb, 2 permute_squeeze, 3 permute_node, 4 permute_textbook
int hs_rn_permute(uint64_t *states, size_t n, int form) {
  if (form < 0 || form > 4) return -1;
  for (size_t i = 0; i < n; i++) sim::permute(states + 12 * i, form);
  return 0;
}
}
