// TEST-ONLY: csrc/fri_verify.h compiled for the host, so that check_path and check_query - the code the kernels k_paths and
// k_arith run per lane - can be held against the oracle and the reference proofs without a GPU. Never loaded by the product.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../city-rollup_amd/csrc/poseidon_tables.h"
#include "../../city-rollup_amd/csrc/fri_verify.h"

extern "C" {
size_t vh_instance_size() { return sizeof(friv::Instance); }
int vh_check_path(const uint64_t *leaf, uint32_t leaf_len, uint64_t index, const uint64_t *sib, uint32_t depth, const uint64_t *cap,
                  uint32_t cap_height) {
  return friv::check_path(leaf, leaf_len, index, sib, depth, cap, cap_height) ? 1 : 0;
}
// The whole query phase of one proof, folded into the key exactly as the kernels do: every (query round, tree) of k_paths'
// grid, every query round of k_arith's, combined with min.
uint32_t vh_query_phase(const friv::Instance *inst, const uint64_t *proof_words, const uint64_t *rec, const uint64_t *shared_caps) {
  uint32_t key = friv::KEY_NONE;
  const friv::InstancePtr I = (friv::InstancePtr)inst;  // a plain pointer on the host
  for (uint32_t qi = 0; qi < inst->n_queries; qi++) {
    for (uint32_t tree = 0; tree < inst->n_oracles + inst->n_layers; tree++) {
      const uint32_t k = friv::path_key(I, proof_words, rec, shared_caps, qi, tree);
      if (k < key) key = k;
    }
    const uint32_t k = friv::check_query(I, proof_words, rec, qi);
    if (k < key) key = k;
  }
  return key;
}
// vh_query_phase over n (proof, record) pairs laid out as the kernels get them: [proof][proof_words], [proof][rec_words]
void vh_query_phase_many(const friv::Instance *inst, const uint64_t *proofs, size_t proof_words, const uint64_t *recs, size_t rec_words,
                         const uint64_t *shared_caps, size_t n, uint32_t *keys_out) {
  unsigned T = std::thread::hardware_concurrency();
  T = T < 1 ? 1 : T > 8 ? 8 : T;
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < T; t++)
    pool.emplace_back([=] {
      for (size_t p = t; p < n; p += T) keys_out[p] = vh_query_phase(inst, proofs + p * proof_words, recs + p * rec_words, shared_caps);
    });
  for (std::thread &th : pool) th.join();
}
// compute_evaluation alone: evals = 2^ab extension values in the proof's (bit-reversed) order
void vh_coset_eval(const uint64_t *evals, uint64_t x, uint32_t within, uint32_t ab, uint64_t g, const uint64_t *beta, uint64_t *out) {
  uint64_t xn = x;
  for (uint32_t k = 0; k < ab; k++) xn = gl::mul(xn, xn);
  const gl::Ext r = friv::coset_eval(evals, x, xn, within, ab, g, gl::Ext{beta[0], beta[1]});
  out[0] = r.a;
  out[1] = r.b;
}
}
