// TEST-ONLY: the sponge-aware forms of the Poseidon permutation (city-rollup_amd/csrc/poseidon.h `permute_until<OUT, ZERO_CAP>`)
// instantiated on the host next to `permute_textbook`. Never loaded by the product path.
#include "../../city-rollup_amd/csrc/gl.h"
#include "../../city-rollup_amd/csrc/poseidon.h"

namespace {
template <int OUT, bool ZERO>
void run_static(uint64_t (&s)[12]) { poseidon::permute_until<OUT, ZERO>(s, poseidon::NeverStop()); }
}  // namespace

extern "C" {
// states: n x 12, permuted in place by the form (out, zero_cap). Words the form does not keep come back as whatever the
// permutation left there. Returns -1 for an unknown form.
int hs_sponge_permute(uint64_t *states, size_t n, int out, int zero_cap) {
  using namespace poseidon;
  if (out != OUT_ALL && out != OUT_CAPACITY && out != OUT_DIGEST) return -1;
  for (size_t i = 0; i < n; i++) {
    uint64_t s[12];
    for (int k = 0; k < 12; k++) s[k] = states[12 * i + k];
    if (out == OUT_ALL && !zero_cap) run_static<OUT_ALL, false>(s);
    else if (out == OUT_ALL) run_static<OUT_ALL, true>(s);
    else if (out == OUT_CAPACITY && !zero_cap) run_static<OUT_CAPACITY, false>(s);
    else if (out == OUT_CAPACITY) run_static<OUT_CAPACITY, true>(s);
    else if (!zero_cap) run_static<OUT_DIGEST, false>(s);
    else run_static<OUT_DIGEST, true>(s);
    for (int k = 0; k < 12; k++) states[12 * i + k] = s[k];
  }
  return 0;
}
void hs_sponge_textbook(uint64_t *states, size_t n) {
  for (size_t i = 0; i < n; i++) {
    uint64_t s[12];
    for (int k = 0; k < 12; k++) s[k] = states[12 * i + k];
    poseidon::permute_textbook(s);
    for (int k = 0; k < 12; k++) states[12 * i + k] = s[k];
  }
}
// hash_no_pad of `total` > 4 words the way merkle::k_leaf_hash_cols runs it (one call per form), digest -> out[4];
// poison: what the dead words are overwritten with between permutations (a form that reads one gives another digest)
void hs_sponge_hash(const uint64_t *words, int total, uint64_t poison, uint64_t *out) {
  using namespace poseidon;
  uint64_t s[12] = {0};
  const int rem = total % RATE;
  const int n_absorb = (total - 1) / RATE - (rem ? 1 : 0);
  int j = 0;
  for (int c = 0; c < n_absorb; c++, j += RATE) {
    for (int k = 0; k < RATE; k++) s[k] = words[j + k];
    permute_absorb(s);
    for (int k = 0; k < RATE; k++) s[k] = poison;
  }
  if (rem && total > RATE) {
    for (int k = 0; k < RATE; k++) s[k] = words[j + k];
    permute(s);
    j += RATE;
  }
  for (int k = 0; k < RATE; k++)
    if (j + k < total) s[k] = words[j + k];
  permute_squeeze(s);
  for (int k = 0; k < 4; k++) out[k] = s[k];
}
// one tree node: the two child digests in words 0..7, capacity declared zero (poisoned here: never read)
void hs_sponge_node(const uint64_t *children, uint64_t poison, uint64_t *out) {
  uint64_t s[12];
  for (int k = 0; k < 12; k++) s[k] = k < 8 ? children[k] : poison;
  poseidon::permute_node(s);
  for (int k = 0; k < 4; k++) out[k] = s[k];
}
// the same sponge with the textbook permutation and nothing skipped
void hs_sponge_hash_textbook(const uint64_t *words, int total, uint64_t *out) {
  uint64_t s[12] = {0};
  for (int j = 0; j < total; j += poseidon::RATE) {
    for (int k = 0; k < poseidon::RATE; k++)
      if (j + k < total) s[k] = words[j + k];
    poseidon::permute_textbook(s);
  }
  for (int k = 0; k < 4; k++) out[k] = s[k];
}
}
