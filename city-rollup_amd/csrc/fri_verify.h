// The query phase of plonky2 `verify_fri_proof` over proofs of ONE shape, one definition for the host and the device: what
// verify.inc's verify_fri_queries does for one proof on one core, per (proof, query round, tree) and per (proof, query round).
// cp_verify_batch and cp_verify_fri_queries_with_challenges_batch (verify.inc) launch k_paths and k_arith below, cp_stark_verify_batch
// (stark.inc) k_arith and either k_paths or its twelve-lane form k_paths_coop; tests/verify_hostsim compiles check_path / check_query
// for the host. Nothing here knows plonky2's four oracles or a STARK's two or three: the instance table says how many oracles there
// are, how long their leaves are and where every field of a query round lies.
//
// Proofs of one shape have the same length and every field at the same offset (the shape dictates every length prefix:
// parse_fri_proof, parse_proof_bytes), so a batch is an array [proof][words] with one stride, read where the prover's bytes lie.
#pragma once
#include "gl.h"
#include "poseidon.h"
#if defined(__HIPCC__)
#include "poseidon_coop.h"
#endif

namespace friv {

constexpr int MAX_ORACLES = 8, MAX_LAYERS = 8, MAX_BATCHES = 4, MAX_RANGES = 16;
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;  // nothing failed

// POD twin of verify.inc's FriVerifyInstance, built once per call on the host. Offsets are u64 words; `*_off` of a query round
// are relative to the round (round qi of a proof starts at q_base + qi * q_words), the others to the start of the proof.
struct Instance {
  uint32_t n_oracles, n_layers, n_batches, n_ranges, n_queries, cap_height, log_n, final_len;
  uint32_t q_base, q_words, final_off, depth0;
  uint32_t leaf_len[MAX_ORACLES];  // salt included
  uint32_t leaf_off[MAX_ORACLES], sib_off[MAX_ORACLES];
  uint32_t cap_src[MAX_ORACLES];   // 0: this oracle's paths are not checked (cap unknown); 1: cap in the proof at cap_off; 2: in the call's shared array
  uint32_t cap_off[MAX_ORACLES];
  uint32_t arity_bits[MAX_LAYERS], layer_depth[MAX_LAYERS], ev_off[MAX_LAYERS], path_off[MAX_LAYERS], fcap_off[MAX_LAYERS];
  uint32_t batch_first[MAX_BATCHES + 1];  // opening batch b = ranges [batch_first[b], batch_first[b + 1])
  uint32_t r_oracle[MAX_RANGES], r_first[MAX_RANGES], r_count[MAX_RANGES];
  uint64_t omega;                 // generator of the LDE domain (order 2^log_n)
  uint64_t arity_g[MAX_LAYERS];   // generator of order 2^arity_bits[l]
};

// Per-proof challenge record (u64 words): alpha | per batch: point, reduced openings, alpha^count | per layer: beta | x_index per round
GL_HD uint32_t rec_alpha() { return 0; }
GL_HD uint32_t rec_batch(uint32_t b) { return 2 + 6 * b; }
GL_HD uint32_t rec_beta(uint32_t n_batches, uint32_t l) { return 2 + 6 * n_batches + 2 * l; }
GL_HD uint32_t rec_index(uint32_t n_batches, uint32_t n_layers, uint32_t qi) { return 2 + 6 * n_batches + 2 * n_layers + qi; }
inline uint32_t rec_words(uint32_t n_batches, uint32_t n_layers, uint32_t n_queries) { return rec_index(n_batches, n_layers, n_queries); }

// Position of a check inside a query round, in verify_fri_queries' order: the key of a failure is query << 8 | ordinal, and the
// minimum over a proof is the first failure the host verifier would name.
GL_HD uint32_t ord_oracle(uint32_t o) { return o; }
GL_HD uint32_t ord_coset(uint32_t n_oracles) { return n_oracles; }
GL_HD uint32_t ord_value(uint32_t n_oracles, uint32_t l) { return n_oracles + 1 + 2 * l; }
GL_HD uint32_t ord_layer_path(uint32_t n_oracles, uint32_t l) { return n_oracles + 2 + 2 * l; }
GL_HD uint32_t ord_final(uint32_t n_oracles, uint32_t n_layers) { return n_oracles + 1 + 2 * n_layers; }

// The instance table is read at wave-uniform addresses. Through the constant address space those reads are scalar loads (the
// kernels never write what they read this way), as air.h reads its bytecode and tables.
#if defined(__HIP_DEVICE_COMPILE__)
#define FRIV_CONSTANT_AS __attribute__((address_space(4)))
#else
#define FRIV_CONSTANT_AS
#endif
typedef const FRIV_CONSTANT_AS Instance *InstancePtr;

GL_HD gl::Ext ext_inv(gl::Ext x) {  // 1 / (a + bX) = (a - bX) / (a^2 - 7 b^2)
  const uint64_t ni = gl::inv(gl::sub(gl::mul(x.a, x.a), gl::mul(7, gl::mul(x.b, x.b))));
  return gl::Ext{gl::mul(x.a, ni), gl::mul(gl::neg(x.b), ni)};
}
GL_HD uint32_t rev_bits(uint32_t x, uint32_t bits) { return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0; }

// hash_or_noop of a leaf, the climb to the cap, the comparison with the cap entry (host_merkle_verify).
GL_HD bool check_path(const uint64_t *leaf, uint32_t leaf_len, uint64_t index, const uint64_t *sib, uint32_t depth, const uint64_t *cap,
                      uint32_t cap_height) {
  constexpr int RATE = poseidon::RATE;
  uint64_t s[poseidon::W];
#pragma unroll
  for (int k = 0; k < poseidon::W; k++) s[k] = 0;
  if (leaf_len <= 4) {  // a leaf of at most four elements is its own digest
#pragma unroll
    for (int k = 0; k < 4; k++)
      if ((uint32_t)k < leaf_len) s[k] = leaf[k];
  } else {
    // as merkle.h's leaf hash: a chunk whose successor overwrites all eight rate words keeps only the capacity; the chunk
    // before a PARTIAL last one keeps everything; the last gives the digest
    const uint32_t rem = leaf_len % RATE;
    const int n_absorb = (int)((leaf_len - 1) / RATE) - (rem ? 1 : 0);  // -1 for a leaf of 5 .. 7 elements: none
    uint32_t j = 0;
#pragma unroll 1
    for (int c = 0; c < n_absorb; c++, j += RATE) {
#pragma unroll
      for (int k = 0; k < RATE; k++) s[k] = leaf[j + k];
      poseidon::permute_absorb(s);
    }
    if (rem && leaf_len > (uint32_t)RATE) {
#pragma unroll
      for (int k = 0; k < RATE; k++) s[k] = leaf[j + k];
      poseidon::permute(s);
      j += RATE;
    }
#pragma unroll
    for (int k = 0; k < RATE; k++)
      if (j + k < leaf_len) s[k] = leaf[j + k];
    poseidon::permute_squeeze(s);
  }
#pragma unroll 1
  for (uint32_t i = 0; i < depth; i++) {
    const uint64_t *sb = sib + 4 * i;
    const bool right = (index >> i) & 1;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t c = s[k], o = sb[k];
      s[k] = right ? o : c;
      s[4 + k] = right ? c : o;
    }
    poseidon::permute_node(s);  // zero capacity in, digest out
  }
  const uint64_t top = depth < 64 ? index >> depth : 0;
  if (top >= ((uint64_t)1 << cap_height)) return false;  // an index past the cap
  const uint64_t *c = cap + 4 * top;
  return s[0] == c[0] && s[1] == c[1] && s[2] == c[2] && s[3] == c[3];
}

// Tree `tree` (oracle 0 .. n_oracles - 1, then FRI layer 0 .. n_layers - 1) of query round qi of one proof: KEY_NONE or the key
// of the failed path. pw: the proof's words; rec: its challenge record; shared_caps: the call's shared cap array (cap_src 2).
GL_HD uint32_t path_key(InstancePtr I, const uint64_t *pw, const uint64_t *rec, const uint64_t *shared_caps, uint32_t qi, uint32_t tree) {
  const uint32_t n_or = I->n_oracles;
  const uint64_t *round = pw + I->q_base + (size_t)qi * I->q_words;
  const uint64_t x_index = rec[rec_index(I->n_batches, I->n_layers, qi)];
  if (tree < n_or) {
    const uint32_t src = I->cap_src[tree];
    if (src == 0) return KEY_NONE;
    const uint64_t *cap = (src == 1 ? pw : shared_caps) + I->cap_off[tree];
    const bool ok = check_path(round + I->leaf_off[tree], I->leaf_len[tree], x_index, round + I->sib_off[tree], I->depth0, cap, I->cap_height);
    return ok ? KEY_NONE : (qi << 8 | ord_oracle(tree));
  }
  const uint32_t l = tree - n_or;
  uint32_t bits = 0;
  for (uint32_t k = 0; k <= l; k++) bits += I->arity_bits[k];
  const bool ok = check_path(round + I->ev_off[l], 2u << I->arity_bits[l], x_index >> bits, round + I->path_off[l], I->layer_depth[l],
                             pw + I->fcap_off[l], I->cap_height);
  return ok ? KEY_NONE : (qi << 8 | ord_layer_path(n_or, l));
}

// plonky2 `compute_evaluation`: the interpolant through the coset's 2^ab opened values, at beta. The values stay where the proof
// holds them (bit-reversed order); for the coset {p_i = s g^i} with s^n = x^n the interpolant is
//   (1 / (n x^n)) sum_i v_i p_i prod_{j != i} (beta - p_j)
// (Z(X) = X^n - x^n, Z'(p_i) = n x^n / p_i): running products, one inversion, no per-lane array. The arithmetic is exact, so this
// is fold_eval's value. xn = x^n.
GL_HD gl::Ext coset_eval(const uint64_t *evals, uint64_t x, uint64_t xn, uint32_t within, uint32_t ab, uint64_t g, gl::Ext beta) {
  const uint32_t n = 1u << ab;
  const uint64_t s = gl::mul(x, gl::pow(g, n - rev_bits(within, ab)));
  gl::Ext acc{0, 0};
  uint64_t pi = s;
#pragma unroll 1
  for (uint32_t i = 0; i < n; i++) {
    gl::Ext prod{pi, 0};
    uint64_t pj = s;
#pragma unroll 1
    for (uint32_t j = 0; j < n; j++) {
      if (j != i) prod = gl::ext_mul(prod, gl::Ext{gl::sub(beta.a, pj), beta.b});
      pj = gl::mul(pj, g);
    }
    const uint32_t r = rev_bits(i, ab);
    acc = gl::ext_add(acc, gl::ext_mul(prod, gl::Ext{evals[2 * r], evals[2 * r + 1]}));
    pi = gl::mul(pi, g);
  }
  return gl::ext_scale(acc, gl::inv(gl::mul((uint64_t)n, xn)));
}

// All the arithmetic of query round qi of one proof (fri_combine_initial, per layer the opened value against the running value
// and compute_evaluation, the final polynomial): KEY_NONE or the key of the first check that fails.
GL_HD uint32_t check_query(InstancePtr I, const uint64_t *pw, const uint64_t *rec, uint32_t qi) {
  const uint32_t n_or = I->n_oracles, nb = I->n_batches, nl = I->n_layers, lb = I->log_n;
  const uint64_t *round = pw + I->q_base + (size_t)qi * I->q_words;
  const uint64_t x_index = rec[rec_index(nb, nl, qi)];
  const gl::Ext alpha{rec[rec_alpha()], rec[rec_alpha() + 1]};
  uint64_t x = gl::mul(7, gl::pow(I->omega, rev_bits((uint32_t)x_index, lb)));
  gl::Ext sum{0, 0};
#pragma unroll 1
  for (uint32_t b = 0; b < nb; b++) {
    const uint64_t *rb = rec + rec_batch(b);
    gl::Ext re{0, 0};
#pragma unroll 1
    for (uint32_t r = I->batch_first[b + 1]; r-- > I->batch_first[b];) {
      const uint64_t *ev = round + I->leaf_off[I->r_oracle[r]] + I->r_first[r];  // unsalted_eval: the salt lies behind the values
#pragma unroll 1
      for (uint32_t j = I->r_count[r]; j-- > 0;) {
        re = gl::ext_mul(re, alpha);
        re.a = gl::add(re.a, ev[j]);
      }
    }
    const gl::Ext den{gl::sub(x, rb[0]), gl::neg(rb[1])};
    if (den.a == 0 && den.b == 0) return qi << 8 | ord_coset(n_or);  // the opening point lies on the LDE coset
    const gl::Ext red{rb[2], rb[3]}, shift{rb[4], rb[5]};
    sum = gl::ext_add(gl::ext_mul(sum, shift), gl::ext_mul(gl::ext_sub(re, red), ext_inv(den)));
  }
  gl::Ext old = sum;
  uint64_t xi = x_index;
#pragma unroll 1
  for (uint32_t l = 0; l < nl; l++) {
    const uint32_t ab = I->arity_bits[l];
    const uint64_t *fe = round + I->ev_off[l];
    const uint32_t within = (uint32_t)xi & ((1u << ab) - 1);
    if (fe[2 * within] != old.a || fe[2 * within + 1] != old.b) return qi << 8 | ord_value(n_or, l);
    uint64_t xn = x;
    for (uint32_t k = 0; k < ab; k++) xn = gl::mul(xn, xn);
    const uint64_t *bt = rec + rec_beta(nb, l);
    old = coset_eval(fe, x, xn, within, ab, I->arity_g[l], gl::Ext{bt[0], bt[1]});
    x = xn;
    xi >>= ab;
  }
  const uint64_t *fp = pw + I->final_off;
  gl::Ext v{0, 0};
#pragma unroll 1
  for (uint32_t i = I->final_len; i-- > 0;) v = gl::ext_add(gl::ext_scale(v, x), gl::Ext{fp[2 * i], fp[2 * i + 1]});
  if (v.a != old.a || v.b != old.b) return qi << 8 | ord_final(n_or, nl);
  return KEY_NONE;
}

#if defined(__HIPCC__)
struct KArgs {
  const Instance *inst;         // device memory, read through the constant address space
  const uint64_t *proofs;       // [proof][proof_words] as uploaded
  const uint64_t *recs;         // [proof][rec_words]
  const uint64_t *shared_caps;  // caps of the oracles with cap_src 2 (the circuit's constants / sigmas cap), or null
  const uint8_t *active;        // [proof] 0: the host phase has this proof's verdict already
  uint32_t *keys;               // [proof] atomicMin of the failure keys
  size_t proof_words;
  uint32_t rec_words, n_proofs, n_queries;
};

// grid (ceil(n_proofs n_queries / 64), n_oracles + n_layers), one wave per workgroup; one lane per (proof, query round).
// blockIdx.y names the tree, so leaf length and depth are wave-uniform.
__global__ __launch_bounds__(64) void k_paths(KArgs a) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= (size_t)a.n_proofs * a.n_queries) return;
  const uint32_t p = (uint32_t)(t / a.n_queries), qi = (uint32_t)(t % a.n_queries);
  if (!a.active[p]) return;
  const uint32_t key = path_key((InstancePtr)a.inst, a.proofs + p * a.proof_words, a.recs + (size_t)p * a.rec_words, a.shared_caps, qi, blockIdx.y);
  if (key != KEY_NONE) atomicMin(a.keys + p, key);
}

// check_path / path_key with TWELVE lanes per path (poseidon_coop.h), for batches of few proofs with long leaves: three STARK proofs
// of 84 query rounds are 252 paths per tree - with k_paths four waves, each alone on its SIMD with a chain of up to 114
// permutations. Here a group of twelve lanes holds one sponge state, one element per lane; five paths per wave, lanes 60..63 idle.
// grid (ceil(n_proofs n_queries / 20), n_oracles + n_layers), four waves per workgroup. blockIdx.y names the tree, so leaf
// length, depth and with them every trip count are uniform over the workgroup: all 64 lanes of a wave make every pcoop::permute
// call together, groups past the end or of an inactive proof with dummies (they load nothing and report nothing).
__global__ __launch_bounds__(256) void k_paths_coop(KArgs a) {
  using namespace pcoop;
  __shared__ __attribute__((aligned(16))) uint64_t sh[WAVES][STATES_PER_WAVE * GROUP];
  const InstancePtr I = (InstancePtr)a.inst;
  const uint32_t tree = blockIdx.y, n_or = I->n_oracles;
  // the tree's own numbers (path_key), all wave-uniform
  uint32_t leaf_off, leaf_len, sib_off, depth, cap_off, ord, shift = 0;
  bool shared = false;
  if (tree < n_or) {
    const uint32_t src = I->cap_src[tree];
    if (src == 0) return;  // the whole workgroup: this oracle's paths are not checked
    shared = src == 2;
    leaf_off = I->leaf_off[tree]; leaf_len = I->leaf_len[tree]; sib_off = I->sib_off[tree]; depth = I->depth0; cap_off = I->cap_off[tree];
    ord = ord_oracle(tree);
  } else {
    const uint32_t l = tree - n_or;
    for (uint32_t k = 0; k <= l; k++) shift += I->arity_bits[k];
    leaf_off = I->ev_off[l]; leaf_len = 2u << I->arity_bits[l]; sib_off = I->path_off[l]; depth = I->layer_depth[l]; cap_off = I->fcap_off[l];
    ord = ord_layer_path(n_or, l);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool lane_used = lane < STATES_PER_WAVE * GROUP;
  const int g = lane_used ? lane / GROUP : 0, e = lane_used ? lane - g * GROUP : 0;  // lanes 60..63 shadow group 0 / element 0
  const size_t t = (size_t)blockIdx.x * STATES_PER_BLOCK + wave * STATES_PER_WAVE + g;
  bool active = lane_used && t < (size_t)a.n_proofs * a.n_queries;
  const uint32_t p = active ? (uint32_t)(t / a.n_queries) : 0, qi = active ? (uint32_t)(t % a.n_queries) : 0;
  active = active && a.active[p];
  const uint64_t *pw = a.proofs + p * a.proof_words;
  const uint64_t *round = pw + I->q_base + (size_t)qi * I->q_words;
  const uint64_t *leaf = round + leaf_off, *sib = round + sib_off;
  const uint64_t index = active ? a.recs[(size_t)p * a.rec_words + rec_index(I->n_batches, I->n_layers, qi)] >> shift : 0;
  uint32_t coef[GROUP];
#pragma unroll
  for (int k = 0; k < GROUP; k++) coef[k] = mds_coef(e, k);
  // hash_or_noop of the leaf: the overwrite sponge, which is check_path's case analysis with whole permutations - a full chunk
  // overwrites the eight rate lanes and keeps the capacity, a partial last chunk keeps what it does not cover (so the chunk before
  // it keeps everything), a leaf of 5 .. 7 elements is one partial chunk over the zero state
  uint64_t x = 0;
  if (leaf_len <= 4) {  // a leaf of at most four elements is its own digest
    if (active && (uint32_t)e < leaf_len) x = leaf[e];
  } else {
    uint64_t nxt = (active && e < RATE_ && (uint32_t)e < leaf_len) ? leaf[e] : 0;
#pragma unroll 1
    for (uint32_t j = 0; j < leaf_len; j += RATE_) {
      if (e < RATE_ && j + e < leaf_len) x = nxt;
      const uint32_t n0 = j + RATE_;
      nxt = (active && e < RATE_ && n0 + e < leaf_len) ? leaf[n0 + e] : 0;  // fetched under the permutation
      x = permute(x, g, e, lane_used, sh[wave], coef);
    }
  }
  // the climb: the digest sits in lanes 0..3 of the group; it stays there or moves to lanes 4..7 by the index bit, the sibling takes
  // the other half, lanes 8..11 carry the zero capacity
#pragma unroll 1
  for (uint32_t i = 0; i < depth; i++) {
    const bool right = (index >> i) & 1;
    const uint64_t below = __shfl(x, (lane + 60) & 63);  // lane e of a group sees lane e - 4: the digest, for e = 4..7
    const uint64_t s = (active && e < 8) ? sib[4 * i + (e & 3)] : 0;
    x = e < 4 ? (right ? s : x) : e < 8 ? (right ? below : s) : 0;
    x = permute(x, g, e, lane_used, sh[wave], coef);
  }
  const uint64_t top = index >> depth;  // depth <= 30
  bool bad = false;
  if (active && e < 4) {
    bad = top >= ((uint64_t)1 << I->cap_height);  // an index past the cap
    if (!bad) bad = x != ((shared ? a.shared_caps : pw) + cap_off)[4 * top + e];
  }
  const uint64_t failed = __ballot(bad);
  if (active && e == 0 && ((failed >> (g * GROUP)) & 0xF)) atomicMin(a.keys + p, qi << 8 | ord);
}

// grid (ceil(n_proofs n_queries / 64)), one lane per (proof, query round)
__global__ __launch_bounds__(64) void k_arith(KArgs a) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (t >= (size_t)a.n_proofs * a.n_queries) return;
  const uint32_t p = (uint32_t)(t / a.n_queries), qi = (uint32_t)(t % a.n_queries);
  if (!a.active[p]) return;
  const uint32_t key = check_query((InstancePtr)a.inst, a.proofs + p * a.proof_words, a.recs + (size_t)p * a.rec_words, qi);
  if (key != KEY_NONE) atomicMin(a.keys + p, key);
}
#endif

}  // namespace friv
