// cp_verify — host-side verifier of ProofWithPublicInputs (plonky2 `CircuitData::verify`, called by the
// reference at city_common_circuit/src/proof_minifier/pm_chain.rs:264-268). Verification is ~3 K
// permutations and a few thousand field operations: it runs on the host, like plonky2's, with the same
// __host__ __device__ arithmetic as the kernels. Included at the end of cityprover.hip.
//
// Checks, in plonky2's order: proof shape; transcript challenges; the vanishing identity
// Z_H(zeta) * sum_i zeta^(n i) t_i(zeta) == vanishing(zeta) from the openings (needs the gate set);
// proof of work; for every query round the Merkle paths of the four oracles, fri_combine_initial, the
// fold chain with its layer Merkle paths, and the final polynomial.

namespace {

struct Rd {
  const uint8_t *p;
  size_t len, o = 0;
  bool bad = false;
  bool noncanonical = false;  // some field element read through felts() was >= p
  uint64_t u64() {
    if (o + 8 > len) { bad = true; return 0; }
    uint64_t v;
    memcpy(&v, p + o, 8);
    o += 8;
    return v;
  }
  const uint64_t *felts(size_t n) {
    if (n > (len - o) / 8) { bad = true; return nullptr; }
    const uint64_t *v = (const uint64_t *)(p + o);
    for (size_t i = 0; i < n; i++) {
      uint64_t e;
      memcpy(&e, p + o + 8 * i, 8);
      noncanonical |= e >= gl::P;
    }
    o += 8 * n;
    return v;
  }
};

inline gl::Ext ext(uint64_t a) { return gl::Ext{a, 0}; }
inline bool ext_eq(gl::Ext x, gl::Ext y) { return x.a == y.a && x.b == y.b; }

void host_hash_or_noop(const uint64_t *in, size_t n, uint64_t out[4]) {
  if (n <= 4) {
    for (int i = 0; i < 4; i++) out[i] = (size_t)i < n ? in[i] : 0;
    return;
  }
  uint64_t st[12] = {0};
  for (size_t off = 0; off < n; off += 8) {
    size_t c = n - off < 8 ? n - off : 8;
    memcpy(st, in + off, c * 8);
    poseidon::permute_host(st);
  }
  memcpy(out, st, 32);
}

bool host_merkle_verify(const uint64_t *leaf, size_t leaf_len, size_t index, const uint64_t *sib, size_t depth,
                        const uint64_t *cap, int cap_height) {
  uint64_t cur[4];
  host_hash_or_noop(leaf, leaf_len, cur);
  for (size_t i = 0; i < depth; i++) {
    uint64_t st[12] = {0};
    if ((index & 1) == 0) { memcpy(st, cur, 32); memcpy(st + 4, sib + 4 * i, 32); }
    else { memcpy(st, sib + 4 * i, 32); memcpy(st + 4, cur, 32); }
    poseidon::permute_host(st);
    memcpy(cur, st, 32);
    index >>= 1;
  }
  if (index >= ((size_t)1 << cap_height)) return false;
  return memcmp(cur, cap + 4 * index, 32) == 0;
}

size_t rev_bits(size_t x, int bits) {
  size_t r = 0;
  for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
  return r;
}

// plonky2 `compute_evaluation`: interpolate the coset values and evaluate at beta
gl::Ext fold_eval(uint64_t x, size_t within, int arity_bits, const uint64_t *evals, gl::Ext beta) {
  const size_t arity = (size_t)1 << arity_bits;
  const uint64_t g = GL_ROOTS[arity_bits];
  std::vector<gl::Ext> ev(arity);
  std::vector<uint64_t> pts(arity);
  for (size_t i = 0; i < arity; i++) { size_t r = rev_bits(i, arity_bits); ev[i] = gl::Ext{evals[2 * r], evals[2 * r + 1]}; }
  uint64_t start = gl::mul(x, gl::pow(g, arity - rev_bits(within, arity_bits)));
  uint64_t gp = 1;
  for (size_t i = 0; i < arity; i++) { pts[i] = gl::mul(start, gp); gp = gl::mul(gp, g); }
  gl::Ext acc{0, 0};
  for (size_t i = 0; i < arity; i++) {
    gl::Ext num{1, 0};
    uint64_t den = 1;
    for (size_t j = 0; j < arity; j++)
      if (j != i) {
        num = gl::ext_mul(num, gl::ext_sub(beta, ext(pts[j])));
        den = gl::mul(den, gl::sub(pts[i], pts[j]));
      }
    acc = gl::ext_add(acc, gl::ext_mul(ev[i], gl::ext_scale(num, gl::inv(den))));
  }
  return acc;
}

// vanishing(zeta) for every challenge from the openings (ext-field twin of quotient.h)
int host_vanishing(const cp_circuit &c, const uint64_t pi_hash[4], gl::Ext x, gl::Ext l0, const gl::Ext *consts,
                   const gl::Ext *wires, const gl::Ext *zs, const gl::Ext *zs_next, const gl::Ext *pps,
                   const gl::Ext *sigmas, const uint64_t *k_is, const uint64_t *betas, const uint64_t *gammas,
                   const uint64_t *alphas, gl::Ext *out) {
  const cp_shape &sh = c.sh;
  const int nc = sh.num_challenges, R = sh.num_routed_wires, chunk = sh.quotient_degree_factor, npp = sh.num_partial_products;
  int ngc = 0;
  for (auto &g : c.gates) {
    int k = quot::gate_num_constraints(g);
    if (k > ngc) ngc = k;
  }
  std::vector<gl::Ext> terms((size_t)nc + (size_t)nc * (npp + 1) + ngc, gl::Ext{0, 0});
  size_t t = 0;
  for (int ch = 0; ch < nc; ch++) terms[t++] = gl::ext_mul(l0, gl::ext_sub(zs[ch], ext(1)));
  for (int ch = 0; ch < nc; ch++)
    for (int k = 0; k <= npp; k++) {
      gl::Ext prev = k == 0 ? zs[ch] : pps[ch * npp + k - 1];
      gl::Ext next = k == npp ? zs_next[ch] : pps[ch * npp + k];
      gl::Ext pn{1, 0}, pd{1, 0};
      for (int j = k * chunk; j < R && j < (k + 1) * chunk; j++) {
        gl::Ext sid = gl::ext_scale(x, k_is[j]);
        gl::Ext num = gl::ext_add(gl::ext_add(wires[j], gl::ext_scale(sid, betas[ch])), ext(gammas[ch]));
        gl::Ext den = gl::ext_add(gl::ext_add(wires[j], gl::ext_scale(sigmas[j], betas[ch])), ext(gammas[ch]));
        pn = gl::ext_mul(pn, num);
        pd = gl::ext_mul(pd, den);
      }
      terms[t++] = gl::ext_sub(gl::ext_mul(prev, pn), gl::ext_mul(next, pd));
    }
  for (size_t gi = 0; gi < c.gates.size(); gi++) {
    const quot::Gate &g = c.gates[gi];
    gl::Ext sv = consts[g.selector_index];
    gl::Ext f{1, 0};
    for (int r = g.group_start; r < g.group_end; r++)
      if (r != (int)gi) f = gl::ext_mul(f, gl::ext_sub(ext((uint64_t)r), sv));
    if (c.num_selectors > 1) f = gl::ext_mul(f, gl::ext_sub(ext(quot::UNUSED_SELECTOR), sv));
    const gl::Ext *gc = consts + c.num_selectors;
    gates::eval<gl::Ext>(
        g, [&](int j) { return wires[j]; }, [&](int j) { return gc[j]; }, [&](int j) { return ext(pi_hash[j]); },
        [&](int k, gl::Ext v) { terms[t + k] = gl::ext_add(terms[t + k], gl::ext_mul(f, v)); });
  }
  for (int ch = 0; ch < nc; ch++) {
    gl::Ext acc{0, 0};
    for (size_t i = terms.size(); i-- > 0;) acc = gl::ext_add(gl::ext_scale(acc, alphas[ch]), terms[i]);
    out[ch] = acc;
  }
  return 0;
}

// ---- the generic FRI verifier: plonky2 `verify_fri_proof` over arbitrary oracles and opening batches -------------------
// One code path for cp_verify (four oracles, batches at zeta and g*zeta), cp_verify_fri_queries_with_challenges (the
// same with the challenges supplied: the reference proofs of qbench_data/example.bin) and cp_fri_verify (any instance).
struct FriVerifyInstance {
  int db = 0;
  FriCfg cfg{};
  int n_oracles = 0;
  size_t kk[fri::MAX_ORACLES] = {0};        // polynomials per oracle (FriOracleInfo::num_polys)
  size_t leaf_len[fri::MAX_ORACLES] = {0};  // + CP_SALT_SIZE for a blinded oracle under FriParams::hiding
  const uint64_t *caps[fri::MAX_ORACLES] = {nullptr};  // nullptr: that oracle's Merkle paths are not checked (cap unknown)
  std::vector<gl::Ext> points;                          // one per opening batch
  std::vector<std::vector<cp_fri_poly_range>> ranges;   // FriBatchInfo::polynomials as runs
  std::vector<std::vector<gl::Ext>> opened;             // FriOpenings: the claimed values, list order
};
struct ParsedFri {
  const uint64_t *fcap[8] = {nullptr};
  const uint64_t *final_poly = nullptr;
  size_t final_len = 0, q_off = 0;
  uint64_t pow_witness = 0;
};

// Shape-directed parse of bincode `FriProof` starting at r.o (plonky2 `validate_fri_proof_shape`): every length prefix
// must be the one the instance dictates. Leaves r.o behind the pow witness.
int parse_fri_proof(cp_ctx *ctx, const FriVerifyInstance &I, Rd &r, ParsedFri &pf) {
#define VFAIL(...) return set_error(ctx, CP_ERR_VERIFY, __VA_ARGS__)
  const FriCfg &c = I.cfg;
  const size_t N = ((size_t)1 << I.db) << c.rate_bits, cap_n = (size_t)1 << c.cap_height;
  if (r.u64() != (uint64_t)c.n_arity) VFAIL("malformed proof: number of FRI layers");
  for (int l = 0; l < c.n_arity; l++) {
    if (r.u64() != cap_n) VFAIL("malformed proof: FRI cap %d length", l);
    pf.fcap[l] = r.felts(cap_n * 4);
  }
  if (r.u64() != (uint64_t)c.num_query_rounds) VFAIL("malformed proof: number of query rounds");
  if (r.bad) VFAIL("malformed proof: truncated");
  pf.q_off = r.o;
  const int depth0 = I.db + c.rate_bits - c.cap_height;
  int total_arity = 0;
  for (int l = 0; l < c.n_arity; l++) total_arity += c.arity_bits[l];
  for (int qi = 0; qi < c.num_query_rounds; qi++) {
    if (r.u64() != (uint64_t)I.n_oracles) VFAIL("malformed proof: query %d", qi);
    for (int b = 0; b < I.n_oracles; b++) {
      if (r.u64() != I.leaf_len[b]) VFAIL("malformed proof: query %d oracle %d", qi, b);
      r.felts(I.leaf_len[b]);
      if (r.u64() != (uint64_t)depth0) VFAIL("malformed proof: query %d path %d", qi, b);
      r.felts((size_t)depth0 * 4);
    }
    if (r.u64() != (uint64_t)c.n_arity) VFAIL("malformed proof: query %d steps", qi);
    size_t nl = N;
    for (int l = 0; l < c.n_arity; l++) {
      size_t arity = (size_t)1 << c.arity_bits[l];
      nl >>= c.arity_bits[l];
      if (r.u64() != arity) VFAIL("malformed proof: query %d step %d", qi, l);
      r.felts(2 * arity);
      int depth = ilog2(nl) - c.cap_height;
      if (depth < 0) depth = 0;
      if (r.u64() != (uint64_t)depth) VFAIL("malformed proof: query %d step %d path", qi, l);
      r.felts((size_t)depth * 4);
    }
    if (r.bad) VFAIL("malformed proof: truncated");
  }
  pf.final_len = r.u64();
  if (pf.final_len != ((size_t)1 << I.db) >> total_arity) VFAIL("malformed proof: final polynomial length");
  pf.final_poly = r.felts(pf.final_len * 2);
  pf.pow_witness = r.u64();
  if (r.bad) VFAIL("malformed proof: truncated");
#undef VFAIL
  return CP_OK;
}

// The query phase of `verify_fri_proof` (plonky2 fri/verifier.rs `fri_verifier_query_round`): for every query round the
// Merkle paths of the initial oracles, fri_combine_initial, the fold chain with its layer Merkle paths and the final
// polynomial.
int verify_fri_queries(cp_ctx *ctx, const FriVerifyInstance &I, const uint8_t *bytes, size_t len, const ParsedFri &pf, gl::Ext alpha,
                       const gl::Ext *fbetas, const uint64_t *x_indices) {
#define VFAIL(...) return set_error(ctx, CP_ERR_VERIFY, __VA_ARGS__)
  const FriCfg &c = I.cfg;
  const int lb = I.db + c.rate_bits, ch = c.cap_height;
  const size_t N = (size_t)1 << lb;
  const int depth0 = lb - ch;
  const size_t nb = I.points.size();
  // PrecomputedReducedOpenings: alpha.reduce over each batch's claimed values; ReducingFactor::shift by the batch's count
  std::vector<gl::Ext> red(nb, gl::Ext{0, 0}), shift(nb);
  for (size_t b = 0; b < nb; b++) {
    for (size_t j = I.opened[b].size(); j-- > 0;) red[b] = gl::ext_add(gl::ext_mul(red[b], alpha), I.opened[b][j]);
    shift[b] = host_ext_pow(alpha, (uint64_t)I.opened[b].size());
  }
  Rd q{bytes, len, pf.q_off};
  for (int qi = 0; qi < c.num_query_rounds; qi++) {
    const size_t x_index = (size_t)(x_indices[qi] % N);
    q.u64();
    const uint64_t *ev[fri::MAX_ORACLES];
    for (int b = 0; b < I.n_oracles; b++) {
      q.u64();
      ev[b] = q.felts(I.leaf_len[b]);
      q.u64();
      const uint64_t *sib = q.felts((size_t)depth0 * 4);
      if (I.caps[b] && !host_merkle_verify(ev[b], I.leaf_len[b], x_index, sib, depth0, I.caps[b], ch)) VFAIL("query %d: Merkle path of oracle %d", qi, b);
    }
    uint64_t x = gl::mul(7, gl::pow(GL_ROOTS[lb], rev_bits(x_index, lb)));
    gl::Ext sum{0, 0};  // fri_combine_initial
    for (size_t b = 0; b < nb; b++) {
      gl::Ext re{0, 0};
      for (size_t r = I.ranges[b].size(); r-- > 0;) {
        const cp_fri_poly_range &R = I.ranges[b][r];
        for (size_t j = R.count; j-- > 0;) re = gl::ext_add(gl::ext_mul(re, alpha), ext(ev[R.oracle][R.first + j]));  // unsalted_eval
      }
      const gl::Ext den = gl::ext_sub(ext(x), I.points[b]);
      if (den.a == 0 && den.b == 0) VFAIL("query %d: opening point %zu lies on the LDE coset", qi, b);
      sum = gl::ext_add(gl::ext_mul(sum, shift[b]), gl::ext_mul(gl::ext_sub(re, red[b]), host_ext_inv(den)));
    }
    q.u64();
    gl::Ext old = sum;
    size_t xi = x_index, nl = N;
    for (int l = 0; l < c.n_arity; l++) {
      const int ab = c.arity_bits[l];
      const size_t arity = (size_t)1 << ab;
      nl >>= ab;
      q.u64();
      const uint64_t *fe = q.felts(2 * arity);
      int depth = ilog2(nl) - ch;
      if (depth < 0) depth = 0;
      q.u64();
      const uint64_t *sib = q.felts((size_t)depth * 4);
      const size_t within = xi & (arity - 1), coset = xi >> ab;
      if (fe[2 * within] != old.a || fe[2 * within + 1] != old.b) VFAIL("query %d: FRI layer %d value mismatch", qi, l);
      old = fold_eval(x, within, ab, fe, fbetas[l]);
      if (!host_merkle_verify(fe, 2 * arity, coset, sib, depth, pf.fcap[l], ch)) VFAIL("query %d: Merkle path of FRI layer %d", qi, l);
      for (int s = 0; s < ab; s++) x = gl::mul(x, x);
      xi = coset;
    }
    gl::Ext fp{0, 0};
    for (size_t i = pf.final_len; i-- > 0;) fp = gl::ext_add(gl::ext_scale(fp, x), gl::Ext{pf.final_poly[2 * i], pf.final_poly[2 * i + 1]});
    if (!ext_eq(fp, old)) VFAIL("query %d: final polynomial mismatch", qi);
  }
#undef VFAIL
  return CP_OK;
}

// plonky2 `Challenger::fri_challenges`: alpha, the layer betas, the proof-of-work response, the query indices
int fri_challenges(cp_ctx *ctx, HostChallenger &C, const FriVerifyInstance &I, const ParsedFri &pf, gl::Ext &alpha, std::vector<gl::Ext> &fbetas,
                   std::vector<uint64_t> &x_indices) {
  const FriCfg &c = I.cfg;
  const size_t cap_n = (size_t)1 << c.cap_height, N = ((size_t)1 << I.db) << c.rate_bits;
  alpha = C.ext_challenge();
  fbetas.resize(c.n_arity);
  for (int l = 0; l < c.n_arity; l++) { C.observe(pf.fcap[l], cap_n * 4); fbetas[l] = C.ext_challenge(); }
  C.observe(pf.final_poly, pf.final_len * 2);
  if (pf.pow_witness >= gl::P) return set_error(ctx, CP_ERR_VERIFY, "proof-of-work witness is not canonical");
  C.observe(&pf.pow_witness, 1);
  const uint64_t resp = C.challenge();
  if (c.pow_bits > 0 && (resp >> (64 - c.pow_bits)) != 0)
    return set_error(ctx, CP_ERR_VERIFY, "proof of work: response has fewer than %d leading zero bits", c.pow_bits);
  x_indices.resize(c.num_query_rounds);
  for (int qi = 0; qi < c.num_query_rounds; qi++) x_indices[qi] = C.challenge() % N;
  return CP_OK;
}

// ---- ProofWithPublicInputs ---------------------------------------------------------------------------------------------
// caps[0] == nullptr: the constants/sigmas cap is unknown, that oracle's Merkle path is not checked.
struct ParsedProof {
  const uint64_t *caps[4];
  const uint64_t *op[9];
  size_t cnt[9];
  size_t leaf_len[4], kk[4];
  ParsedFri fri;
  const uint64_t *pi;
  size_t n_pi;
};
FriCfg shape_fri_cfg(const cp_shape &sh) {
  FriCfg c;
  c.rate_bits = sh.rate_bits; c.cap_height = sh.cap_height; c.pow_bits = sh.pow_bits; c.num_query_rounds = sh.num_query_rounds;
  c.n_arity = sh.n_arity;
  for (int l = 0; l < 8; l++) c.arity_bits[l] = sh.arity_bits[l];
  return c;
}
// plonky2's FRI instance of a proof (`CommonCircuitData::get_fri_instance`): four oracles; everything at zeta, the Z
// polynomials at g*zeta. Opened values are taken from the parsed OpeningSet when pp is given.
void plonky2_fri_instance(const cp_shape &sh, const ParsedProof *pp, gl::Ext zeta, FriVerifyInstance &I) {
  const int nc = sh.num_challenges;
  const size_t k_cs = (size_t)sh.num_constants + sh.num_routed_wires, k_w = sh.num_wires,
               k_z = (size_t)nc * (1 + sh.num_partial_products), k_q = (size_t)nc * sh.quotient_degree_factor;
  const size_t kk[4] = {k_cs, k_w, k_z, k_q};
  I.db = sh.degree_bits;
  I.cfg = shape_fri_cfg(sh);
  I.n_oracles = 4;
  for (int b = 0; b < 4; b++) {
    I.kk[b] = kk[b];
    // FriParams::hiding: leaves of the blinded oracles end with CP_SALT_SIZE salt elements — under the Merkle paths,
    // outside fri_combine_initial (FriInitialTreeProof::unsalted_eval)
    I.leaf_len[b] = kk[b] + ((sh.zero_knowledge && b >= 1) ? CP_SALT_SIZE : 0);
    I.caps[b] = pp ? pp->caps[b] : nullptr;
  }
  I.points = {zeta, gl::ext_scale(zeta, GL_ROOTS[sh.degree_bits])};
  I.ranges = {{{0, 0, (uint32_t)k_cs}, {1, 0, (uint32_t)k_w}, {2, 0, (uint32_t)k_z}, {3, 0, (uint32_t)k_q}}, {{2, 0, (uint32_t)nc}}};
  I.opened.assign(2, {});
  if (pp) {
    const int zorder[6] = {0, 1, 2, 3, 5, 6};  // constants, sigmas, wires, zs, partial products, quotient
    for (int i = 0; i < 6; i++)
      for (size_t j = 0; j < pp->cnt[zorder[i]]; j++) I.opened[0].push_back(gl::Ext{pp->op[zorder[i]][2 * j], pp->op[zorder[i]][2 * j + 1]});
    for (size_t j = 0; j < pp->cnt[4]; j++) I.opened[1].push_back(gl::Ext{pp->op[4][2 * j], pp->op[4][2 * j + 1]});  // zs_next
  }
}
// Shape-directed parse of bincode `ProofWithPublicInputs` (SURVEY.md Appendix A): every length prefix must be the one the
// shape dictates, every field element canonical, no byte left over. cs_cap: the circuit's constants/sigmas cap (or null).
int parse_proof_bytes(cp_ctx *ctx, const cp_shape &sh, const uint64_t *cs_cap, const uint8_t *proof, size_t len, ParsedProof &pp) {
#define VFAIL(...) return set_error(ctx, CP_ERR_VERIFY, __VA_ARGS__)
  const int nc = sh.num_challenges;
  const size_t cap_n = (size_t)1 << sh.cap_height;
  const size_t k_cs = (size_t)sh.num_constants + sh.num_routed_wires, k_w = sh.num_wires,
               k_z = (size_t)nc * (1 + sh.num_partial_products), k_q = (size_t)nc * sh.quotient_degree_factor;
  const size_t kk[4] = {k_cs, k_w, k_z, k_q};
  Rd r{proof, len};
  pp.caps[0] = cs_cap;
  for (int b = 1; b <= 3; b++) {
    if (r.u64() != cap_n) VFAIL("malformed proof: cap %d length", b);
    pp.caps[b] = r.felts(cap_n * 4);
  }
  const size_t cnt[9] = {(size_t)sh.num_constants, (size_t)sh.num_routed_wires, k_w, (size_t)nc, (size_t)nc, k_z - nc, k_q, 0, 0};
  for (int i = 0; i < 9; i++) {
    if (r.u64() != cnt[i]) VFAIL("malformed proof: opening set %d length", i);
    pp.op[i] = r.felts(cnt[i] * 2);
    pp.cnt[i] = cnt[i];
  }
  if (r.bad) VFAIL("malformed proof: truncated");
  FriVerifyInstance I;
  plonky2_fri_instance(sh, nullptr, gl::Ext{0, 0}, I);
  for (int b = 0; b < 4; b++) { pp.kk[b] = kk[b]; pp.leaf_len[b] = I.leaf_len[b]; }
  CP_TRY(parse_fri_proof(ctx, I, r, pp.fri));
  const size_t n_pi = r.u64();
  const uint64_t *pi = r.felts(n_pi);
  if (r.bad || r.o != len) VFAIL("malformed proof: length");
  // plonky2 `validate_proof_with_pis_shape`: the number of public inputs is the circuit's, not the proof's
  // (hash_no_pad is an unpadded overwrite sponge: [a, b] and [a, b, 0] have the same hash)
  if (n_pi != (size_t)sh.num_public_inputs) VFAIL("%zu public inputs, the circuit has %d", n_pi, sh.num_public_inputs);
  // Every field element of the proof must be canonical (< p): gl::add / gl::sub assume it, so v and v + p would
  // act as different values where they are added and as the same value where they are multiplied — caps, openings,
  // leaves, siblings, FRI evaluations, the final polynomial and the public inputs alike.
  if (r.noncanonical) VFAIL("a field element of the proof is not canonical (>= p)");
  pp.pi = pi;
  pp.n_pi = n_pi;
#undef VFAIL
  return CP_OK;
}

int verify_queries(cp_ctx *ctx, const cp_shape &sh, const uint8_t *proof, size_t len, const ParsedProof &pp, gl::Ext alpha, gl::Ext zeta,
                   const gl::Ext *fbetas, const uint64_t *x_indices) {
  FriVerifyInstance I;
  plonky2_fri_instance(sh, &pp, zeta, I);
  return verify_fri_queries(ctx, I, proof, len, pp.fri, alpha, fbetas, x_indices);
}

}  // namespace

extern "C" int cp_verify(cp_circuit *circ, const uint8_t *proof, size_t len) try {
  if (!circ) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_ctx *ctx = circ->ctx;
  if (!proof) return set_error(ctx, CP_ERR_INVALID_ARG, "proof is NULL");
  if (!circ->has_gates) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit has no gate set (cp_circuit_set_gates)");
#define VFAIL(...) return set_error(ctx, CP_ERR_VERIFY, __VA_ARGS__)
  const cp_shape &sh = circ->sh;
  const int db = sh.degree_bits, rb = sh.rate_bits, ch = sh.cap_height, nc = sh.num_challenges;
  const size_t n = (size_t)1 << db, N = n << rb, cap_n = (size_t)1 << ch;
  ParsedProof pp;
  CP_TRY(parse_proof_bytes(ctx, sh, circ->cs.cap_host.data(), proof, len, pp));
  const uint64_t *const *caps = pp.caps, *const *op = pp.op;
  const size_t *cnt = pp.cnt;
  const uint64_t *pi = pp.pi;
  const size_t n_pi = pp.n_pi;
  hostu::alloc_checkpoint();

  // ---- transcript ----
  uint64_t pi_hash[4];
  {
    uint64_t st[12] = {0};
    for (size_t off = 0; off < n_pi; off += 8) {
      size_t c = n_pi - off < 8 ? n_pi - off : 8;
      memcpy(st, pi + off, c * 8);
      poseidon::permute_host(st);
    }
    memcpy(pi_hash, st, 32);
  }
  HostChallenger C;
  C.observe(circ->digest, 4);
  C.observe(pi_hash, 4);
  C.observe(caps[1], cap_n * 4);
  std::vector<uint64_t> betas(nc), gammas(nc), alphas(nc);
  for (int i = 0; i < nc; i++) betas[i] = C.challenge();
  for (int i = 0; i < nc; i++) gammas[i] = C.challenge();
  C.observe(caps[2], cap_n * 4);
  for (int i = 0; i < nc; i++) alphas[i] = C.challenge();
  C.observe(caps[3], cap_n * 4);
  const gl::Ext zeta = C.ext_challenge();
  const gl::Ext zeta_next = gl::ext_scale(zeta, GL_ROOTS[db]);
  const int zorder[6] = {0, 1, 2, 3, 5, 6};
  for (int i = 0; i < 6; i++) C.observe(op[zorder[i]], cnt[zorder[i]] * 2);
  C.observe(op[4], cnt[4] * 2);

  // ---- vanishing identity at zeta ----
  {
    std::vector<uint64_t> ks(sh.num_routed_wires);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ks.empty()) HIP_TRY(ctx, hipMemcpy(ks.data(), circ->k_is, ks.size() * 8, hipMemcpyDeviceToHost));
    const gl::Ext zn = host_ext_pow(zeta, n);
    const gl::Ext zh = gl::ext_sub(zn, ext(1));
    if (zh.a == 0 && zh.b == 0) VFAIL("zeta is in the subgroup");
    const gl::Ext l0 = gl::ext_mul(zh, host_ext_inv(gl::ext_scale(gl::ext_sub(zeta, ext(1)), (uint64_t)n % gl::P)));
    std::vector<gl::Ext> van(nc);
    host_vanishing(*circ, pi_hash, zeta, l0, (const gl::Ext *)op[0], (const gl::Ext *)op[2], (const gl::Ext *)op[3],
                   (const gl::Ext *)op[4], (const gl::Ext *)op[5], (const gl::Ext *)op[1], ks.data(), betas.data(),
                   gammas.data(), alphas.data(), van.data());
    const int qdf = sh.quotient_degree_factor;
    for (int c = 0; c < nc; c++) {
      gl::Ext acc{0, 0};
      for (int i = qdf - 1; i >= 0; i--)
        acc = gl::ext_add(gl::ext_mul(acc, zn), gl::Ext{op[6][2 * (c * qdf + i)], op[6][2 * (c * qdf + i) + 1]});
      if (!ext_eq(gl::ext_mul(acc, zh), van[c])) VFAIL("vanishing identity fails for challenge %d (constraints not satisfied)", c);
    }
  }

  // ---- FRI ----
#undef VFAIL
  FriVerifyInstance I;
  plonky2_fri_instance(sh, &pp, zeta, I);
  gl::Ext alpha;
  std::vector<gl::Ext> fbetas;
  std::vector<uint64_t> x_indices;
  CP_TRY(fri_challenges(ctx, C, I, pp.fri, alpha, fbetas, x_indices));
  return verify_fri_queries(ctx, I, proof, len, pp.fri, alpha, fbetas.data(), x_indices.data());
} CP_CATCH(circ ? circ->ctx : nullptr)

// Audit hook: the query phase of cp_verify on proof bytes whose transcript cannot be replayed — the reference proofs of
// qbench_data/example.bin come without their circuits (no digest, no constants/sigmas cap), but their FRI challenges can
// be RECOVERED algebraically from the proof itself (tests/reference_challenges.py). With them, the very code cp_verify
// runs is held against plonky2's own output: leaf hashing and Merkle paths of the wires / Z / quotient oracles and of
// every FRI layer, fri_combine_initial (polynomial order, alpha powers, g * zeta), compute_evaluation, the final
// polynomial. Host arithmetic only: no context, no GPU.
extern "C" int cp_verify_fri_queries_with_challenges(const cp_shape *shape, const uint8_t *proof, size_t proof_len, const uint64_t alpha[2],
                                                     const uint64_t zeta[2], const uint64_t *fri_betas, const uint64_t *x_indices) try {
  if (!shape || !proof || !alpha || !zeta || !x_indices || (shape->n_arity > 0 && !fri_betas))
    return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  const cp_shape &sh = *shape;
  if (sh.degree_bits < 2 || sh.degree_bits + sh.rate_bits > 30 || sh.rate_bits < 0 || sh.num_challenges < 1 || sh.num_challenges > 8 ||
      sh.n_arity < 0 || sh.n_arity > 8 || sh.cap_height < 0 || sh.cap_height > sh.degree_bits + sh.rate_bits || sh.num_query_rounds < 1 ||
      sh.num_query_rounds > 255 || sh.num_wires < 1 || sh.num_constants < 0 || sh.num_routed_wires < 0 || sh.num_partial_products < 0 ||
      sh.quotient_degree_factor < 1)
    return set_error(nullptr, CP_ERR_INVALID_ARG, "shape out of range");
  for (int l = 0; l < sh.n_arity; l++)
    if (sh.arity_bits[l] < 1 || sh.arity_bits[l] > 5) return set_error(nullptr, CP_ERR_INVALID_ARG, "FRI arity out of range");
  for (int i = 0; i < 2; i++)
    if (alpha[i] >= gl::P || zeta[i] >= gl::P) return set_error(nullptr, CP_ERR_INVALID_ARG, "challenge is not canonical");
  std::vector<gl::Ext> fb(sh.n_arity);
  for (int l = 0; l < sh.n_arity; l++) {
    if (fri_betas[2 * l] >= gl::P || fri_betas[2 * l + 1] >= gl::P) return set_error(nullptr, CP_ERR_INVALID_ARG, "challenge is not canonical");
    fb[l] = gl::Ext{fri_betas[2 * l], fri_betas[2 * l + 1]};
  }
  ParsedProof pp;
  CP_TRY(parse_proof_bytes(nullptr, sh, nullptr, proof, proof_len, pp));
  if (pp.n_pi != (size_t)sh.num_public_inputs) return set_error(nullptr, CP_ERR_VERIFY, "%zu public inputs, the shape says %d", pp.n_pi, sh.num_public_inputs);
  return verify_queries(nullptr, sh, proof, proof_len, pp, gl::Ext{alpha[0], alpha[1]}, gl::Ext{zeta[0], zeta[1]}, fb.data(), x_indices);
} CP_CATCH(nullptr)

// ---- batches of proofs of one shape: the query phase on the device (fri_verify.h) ------------------------------------------
namespace {

// Staged proof bytes per device pass when the caller leaves chunk_proofs 0 (include/cityprover.h says so too)
constexpr size_t VERIFY_BATCH_PASS_BYTES = (size_t)64 << 20;

// The word offsets of bincode `FriProof` starting at word `o`, field by field as parse_fri_proof walks it; returns the word
// behind the proof-of-work witness. D's oracle caps (cap_src, cap_off) are the caller's.
size_t friv_layout(const FriVerifyInstance &I, size_t o, friv::Instance &D) {
  const FriCfg &c = I.cfg;
  const int lb = I.db + c.rate_bits;
  const size_t cap_n = (size_t)1 << c.cap_height;
  D.n_oracles = (uint32_t)I.n_oracles; D.n_layers = (uint32_t)c.n_arity; D.n_queries = (uint32_t)c.num_query_rounds;
  D.cap_height = (uint32_t)c.cap_height; D.log_n = (uint32_t)lb; D.depth0 = (uint32_t)(lb - c.cap_height);
  D.omega = GL_ROOTS[lb];
  o += 1;
  for (int l = 0; l < c.n_arity; l++) { o += 1; D.fcap_off[l] = (uint32_t)o; o += cap_n * 4; }
  o += 1;
  D.q_base = (uint32_t)o;
  size_t r = 1;
  for (int b = 0; b < I.n_oracles; b++) {
    D.leaf_len[b] = (uint32_t)I.leaf_len[b];
    r += 1; D.leaf_off[b] = (uint32_t)r; r += I.leaf_len[b];
    r += 1; D.sib_off[b] = (uint32_t)r; r += (size_t)D.depth0 * 4;
  }
  r += 1;
  int bits = lb, total_arity = 0;
  for (int l = 0; l < c.n_arity; l++) {
    const int ab = c.arity_bits[l];
    bits -= ab; total_arity += ab;
    int depth = bits - c.cap_height;
    if (depth < 0) depth = 0;
    D.arity_bits[l] = (uint32_t)ab; D.layer_depth[l] = (uint32_t)depth; D.arity_g[l] = GL_ROOTS[ab];
    r += 1; D.ev_off[l] = (uint32_t)r; r += (size_t)2 << ab;
    r += 1; D.path_off[l] = (uint32_t)r; r += (size_t)depth * 4;
  }
  D.q_words = (uint32_t)r;
  o += (size_t)c.num_query_rounds * r;
  D.final_len = (uint32_t)(((size_t)1 << I.db) >> total_arity);
  o += 1; D.final_off = (uint32_t)o; o += (size_t)D.final_len * 2;
  return o + 1;
}

// plonky2's instance as the kernels read it: the table, and the length in words every proof of the shape has
int plonky2_layout(cp_ctx *ctx, const cp_shape &sh, bool check_cs, friv::Instance &D, size_t &proof_words) {
  FriVerifyInstance I;
  plonky2_fri_instance(sh, nullptr, gl::Ext{0, 0}, I);
  memset(&D, 0, sizeof D);
  const size_t cap_n = (size_t)1 << sh.cap_height, nc = (size_t)sh.num_challenges;
  size_t o = 0;
  for (int b = 1; b <= 3; b++) { o += 1; D.cap_src[b] = 1; D.cap_off[b] = (uint32_t)o; o += cap_n * 4; }
  D.cap_src[0] = check_cs ? 2 : 0;
  const size_t cnt[9] = {(size_t)sh.num_constants, (size_t)sh.num_routed_wires, I.kk[1], nc, nc, I.kk[2] - nc, I.kk[3], 0, 0};
  for (int i = 0; i < 9; i++) o += 1 + cnt[i] * 2;
  const size_t fri_end = friv_layout(I, o, D);
  proof_words = fri_end + 1 + (size_t)sh.num_public_inputs;
  if (I.ranges.size() > (size_t)friv::MAX_BATCHES) return set_error(ctx, CP_ERR_INTERNAL, "too many opening batches");
  D.n_batches = (uint32_t)I.ranges.size();
  uint32_t nr = 0;
  for (size_t b = 0; b < I.ranges.size(); b++) {
    D.batch_first[b] = nr;
    for (const cp_fri_poly_range &R : I.ranges[b]) {
      if (nr >= (uint32_t)friv::MAX_RANGES) return set_error(ctx, CP_ERR_INTERNAL, "too many opening ranges");
      D.r_oracle[nr] = R.oracle; D.r_first[nr] = R.first; D.r_count[nr] = R.count;
      nr++;
    }
  }
  D.batch_first[I.ranges.size()] = nr;
  D.n_ranges = nr;
  if (proof_words > ((size_t)1 << 31)) return set_error(ctx, CP_ERR_INVALID_ARG, "shape out of range");
  return CP_OK;
}

// One proof's challenge record (fri_verify.h): what verify_fri_queries precomputes, and the challenges
void fill_record(const FriVerifyInstance &I, gl::Ext alpha, const gl::Ext *fbetas, const uint64_t *x_indices, uint64_t *rec) {
  const uint32_t nb = (uint32_t)I.points.size(), nl = (uint32_t)I.cfg.n_arity;
  const uint64_t N = (uint64_t)1 << (I.db + I.cfg.rate_bits);
  rec[friv::rec_alpha()] = alpha.a; rec[friv::rec_alpha() + 1] = alpha.b;
  for (uint32_t b = 0; b < nb; b++) {
    gl::Ext red{0, 0};
    for (size_t j = I.opened[b].size(); j-- > 0;) red = gl::ext_add(gl::ext_mul(red, alpha), I.opened[b][j]);
    const gl::Ext shift = host_ext_pow(alpha, (uint64_t)I.opened[b].size());
    uint64_t *rb = rec + friv::rec_batch(b);
    rb[0] = I.points[b].a; rb[1] = I.points[b].b; rb[2] = red.a; rb[3] = red.b; rb[4] = shift.a; rb[5] = shift.b;
  }
  for (uint32_t l = 0; l < nl; l++) { rec[friv::rec_beta(nb, l)] = fbetas[l].a; rec[friv::rec_beta(nb, l) + 1] = fbetas[l].b; }
  for (int qi = 0; qi < I.cfg.num_query_rounds; qi++) rec[friv::rec_index(nb, nl, (uint32_t)qi)] = x_indices[qi] % N;
}

cp_verify_verdict verdict(int status, int query = -1, int detail = -1) { return cp_verify_verdict{status, query, detail, 0}; }
// which of parse_proof_bytes' refusals this thread's last error is
cp_verify_verdict parse_verdict() {
  const char *m = g_tls_error.c_str();
  return verdict(strstr(m, "malformed proof") ? 1 : strstr(m, "public inputs") ? 3 : 2);
}
cp_verify_verdict key_verdict(const friv::Instance &D, uint32_t key) {
  if (key == friv::KEY_NONE) return verdict(0);
  const int q = (int)(key >> 8);
  const uint32_t ord = key & 0xFF, n_or = D.n_oracles;
  if (ord < n_or) return verdict(7, q, (int)ord);
  if (ord == friv::ord_coset(n_or)) return verdict(4, q);
  if (ord == friv::ord_final(n_or, D.n_layers)) return verdict(10, q);
  const uint32_t k = ord - n_or - 1;
  return verdict(k & 1 ? 9 : 8, q, (int)(k >> 1));
}

// Everything cp_verify does before its query phase, for one proof of a batch, on whatever thread: the shape-directed parse, the
// transcript, the vanishing identity at zeta, the FRI challenges and the proof of work - the same functions, in the same
// order. ctx is never touched (errors go to the thread's own message). ks: the circuit's k_is, fetched once per call.
// Status 0: `rec` holds the proof's challenge record and the query phase is the device's.
cp_verify_verdict verify_host_phase(const cp_circuit &circ, const uint64_t *ks, const uint8_t *proof, size_t len, uint64_t *rec) {
  const cp_shape &sh = circ.sh;
  const int db = sh.degree_bits, nc = sh.num_challenges;
  const size_t n = (size_t)1 << db, cap_n = (size_t)1 << sh.cap_height;
  ParsedProof pp;
  if (parse_proof_bytes(nullptr, sh, circ.cs.cap_host.data(), proof, len, pp) != CP_OK) return parse_verdict();
  const uint64_t *const *caps = pp.caps, *const *op = pp.op;
  const size_t *cnt = pp.cnt;
  uint64_t pi_hash[4];
  {
    uint64_t st[12] = {0};
    for (size_t off = 0; off < pp.n_pi; off += 8) {
      size_t c = pp.n_pi - off < 8 ? pp.n_pi - off : 8;
      memcpy(st, pp.pi + off, c * 8);
      poseidon::permute_host(st);
    }
    memcpy(pi_hash, st, 32);
  }
  HostChallenger C;
  C.observe(circ.digest, 4);
  C.observe(pi_hash, 4);
  C.observe(caps[1], cap_n * 4);
  std::vector<uint64_t> betas(nc), gammas(nc), alphas(nc);
  for (int i = 0; i < nc; i++) betas[i] = C.challenge();
  for (int i = 0; i < nc; i++) gammas[i] = C.challenge();
  C.observe(caps[2], cap_n * 4);
  for (int i = 0; i < nc; i++) alphas[i] = C.challenge();
  C.observe(caps[3], cap_n * 4);
  const gl::Ext zeta = C.ext_challenge();
  const int zorder[6] = {0, 1, 2, 3, 5, 6};
  for (int i = 0; i < 6; i++) C.observe(op[zorder[i]], cnt[zorder[i]] * 2);
  C.observe(op[4], cnt[4] * 2);
  {
    const gl::Ext zn = host_ext_pow(zeta, n);
    const gl::Ext zh = gl::ext_sub(zn, ext(1));
    if (zh.a == 0 && zh.b == 0) return verdict(4);
    const gl::Ext l0 = gl::ext_mul(zh, host_ext_inv(gl::ext_scale(gl::ext_sub(zeta, ext(1)), (uint64_t)n % gl::P)));
    std::vector<gl::Ext> van(nc);
    host_vanishing(circ, pi_hash, zeta, l0, (const gl::Ext *)op[0], (const gl::Ext *)op[2], (const gl::Ext *)op[3], (const gl::Ext *)op[4],
                   (const gl::Ext *)op[5], (const gl::Ext *)op[1], ks, betas.data(), gammas.data(), alphas.data(), van.data());
    const int qdf = sh.quotient_degree_factor;
    for (int c = 0; c < nc; c++) {
      gl::Ext acc{0, 0};
      for (int i = qdf - 1; i >= 0; i--)
        acc = gl::ext_add(gl::ext_mul(acc, zn), gl::Ext{op[6][2 * (c * qdf + i)], op[6][2 * (c * qdf + i) + 1]});
      if (!ext_eq(gl::ext_mul(acc, zh), van[c])) return verdict(5, -1, c);
    }
  }
  FriVerifyInstance I;
  plonky2_fri_instance(sh, &pp, zeta, I);
  gl::Ext alpha;
  std::vector<gl::Ext> fbetas;
  std::vector<uint64_t> x_indices;
  if (fri_challenges(nullptr, C, I, pp.fri, alpha, fbetas, x_indices) != CP_OK) return verdict(6);
  fill_record(I, alpha, fbetas.data(), x_indices.data(), rec);
  return verdict(0);
}

size_t verify_threads(size_t n) {
  const unsigned hw = std::thread::hardware_concurrency();
  size_t T = n / 4;  // at least four proofs per thread
  if (T > 16) T = 16;
  if (hw && T > hw) T = hw;
  return T;
}
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The passes of a batch. host(p, rec) is the host phase of proof p (any thread; it must not touch ctx or the HIP API): its
// verdict, and with status 0 the challenge record. shared_cap: 2^cap_height x 4 words on the host, or null. path_form: which kernel
// checks the Merkle paths of a pass (PATHS_AUTO decides per pass by its number of paths).
enum PathForm : unsigned { PATHS_AUTO = 0, PATHS_LANE = 1, PATHS_COOP = 2 };
// PATHS_AUTO takes the twelve-lane kernel for passes of fewer than this many paths per tree (active proofs x query rounds). Measured
// at the SHA-256 STARK's shape (DESIGN.md section 1.1a, profiles/stark_verify_batch.json): the twelve-lane kernel is the faster one up
// to 10 752 paths per pass (3.1 against 4.2 ms), the lane-per-path kernel from 21 504 on (4.3 against 5.1 ms); the twelve-lane
// kernel's time between the two, taken as a straight line, meets the other's flat 4.2 ms at about 16 600.
constexpr size_t PATHS_COOP_BELOW = 16384;
template <class Host>
int verify_batch_passes(cp_ctx *ctx, const friv::Instance &D, size_t proof_words, const uint64_t *shared_cap, const uint8_t *const *proofs,
                        const size_t *lens, size_t n, size_t chunk, PathForm path_form, cp_verify_verdict *out, Host host) {
  const size_t L = proof_words * 8, rec_w = friv::rec_words(D.n_batches, D.n_layers, D.n_queries), nq = D.n_queries;
  if (chunk == 0) chunk = VERIFY_BATCH_PASS_BYTES / L ? VERIFY_BATCH_PASS_BYTES / L : 1;
  if (chunk > n) chunk = n;
  if (chunk > ((size_t)1 << 20)) chunk = (size_t)1 << 20;  // lanes of a pass are counted in 32 bits
  const size_t cap_words = shared_cap ? (size_t)4 << D.cap_height : 0;
  ArenaScope scope(ctx);  // drains the stream and recycles the staging area, whichever way the call ends
  // page-locked staging of one pass: proofs | records | instance | shared cap | keys | active
  const size_t o_rec = align256(chunk * L), o_inst = o_rec + align256(chunk * rec_w * 8), o_cap = o_inst + align256(sizeof(friv::Instance)),
               o_keys = o_cap + align256(cap_words * 8), o_act = o_keys + align256(chunk * 4), st_bytes = o_act + align256(chunk);
  char *st;
  CP_TRY(pin_reserve(ctx, st_bytes, &st));
  memcpy(st + o_inst, &D, sizeof D);
  if (cap_words) memcpy(st + o_cap, shared_cap, cap_words * 8);
  uint64_t *st_recs = (uint64_t *)(st + o_rec);
  uint32_t *st_keys = (uint32_t *)(st + o_keys);
  uint8_t *st_act = (uint8_t *)(st + o_act);
  DevBag bag = ctx->bag();  // the device side, allocated by the first pass that has something to launch
  char *d_proofs = nullptr, *d_recs = nullptr, *d_misc = nullptr;
  const size_t m_cap = align256(sizeof(friv::Instance)), m_keys = m_cap + align256(cap_words * 8), m_act = m_keys + align256(chunk * 4),
               m_bytes = m_act + align256(chunk);
  for (size_t base = 0; base < n; base += chunk) {
    const size_t m = n - base < chunk ? n - base : chunk;
    host_phase(ctx, "verify_host");
    hostu::parallel_for(m, verify_threads(m), [&](size_t i) {
      out[base + i] = host(base + i, st_recs + i * rec_w);
      st_act[i] = out[base + i].status == 0;
    });
    size_t n_active = 0;
    for (size_t i = 0; i < m; i++) {
      n_active += st_act[i];
      if (st_act[i] && lens[base + i] != L) return set_error(ctx, CP_ERR_INTERNAL, "a parsed proof has %zu bytes, the shape's layout %zu", lens[base + i], L);
    }
    if (n_active == 0) continue;  // every verdict is the host's: nothing to launch
    host_phase(ctx, "verify_upload");
    hostu::parallel_for(m, verify_threads(m), [&](size_t i) {
      if (st_act[i]) memcpy(st + i * L, proofs[base + i], L);  // also cures an unaligned caller pointer
    });
    if (!d_proofs) {
      CP_TRY(alloc_status(ctx, bag.alloc(&d_proofs, chunk * L), chunk * L));
      CP_TRY(alloc_status(ctx, bag.alloc(&d_recs, chunk * rec_w * 8), chunk * rec_w * 8));
      CP_TRY(alloc_status(ctx, bag.alloc(&d_misc, m_bytes), m_bytes));
      HIP_TRY(ctx, hipMemcpyAsync(d_misc, st + o_inst, sizeof(friv::Instance), hipMemcpyHostToDevice, ctx->stream));
      if (cap_words) HIP_TRY(ctx, hipMemcpyAsync(d_misc + m_cap, st + o_cap, cap_words * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_proofs, st, m * L, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_recs, st_recs, m * rec_w * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_misc + m_act, st_act, m, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(d_misc + m_keys, 0xFF, m * 4, ctx->stream));
    if (ctx->profiling) HIP_TRY(ctx, sync_stream(ctx));  // the upload is then inside the phase that names it
    host_phase(ctx, "verify_device");
    friv::KArgs a;
    a.inst = (const friv::Instance *)d_misc;
    a.proofs = (const uint64_t *)d_proofs;
    a.recs = (const uint64_t *)d_recs;
    a.shared_caps = cap_words ? (const uint64_t *)(d_misc + m_cap) : nullptr;
    a.active = (const uint8_t *)(d_misc + m_act);
    a.keys = (uint32_t *)(d_misc + m_keys);
    a.proof_words = proof_words;
    a.rec_words = (uint32_t)rec_w;
    a.n_proofs = (uint32_t)m;
    a.n_queries = (uint32_t)nq;
    const unsigned blocks = blocks_for(m * nq, 64);
    const bool coop = path_form == PATHS_COOP || (path_form == PATHS_AUTO && n_active * nq < PATHS_COOP_BELOW);
    if (coop)
      LAUNCH(ctx, "verify_paths_coop", friv::k_paths_coop, dim3(blocks_for(m * nq, pcoop::STATES_PER_BLOCK), D.n_oracles + D.n_layers),
             dim3(64 * pcoop::WAVES), a);
    else
      LAUNCH(ctx, "verify_paths", friv::k_paths, dim3(blocks, D.n_oracles + D.n_layers), dim3(64), a);
    LAUNCH(ctx, "verify_arith", friv::k_arith, dim3(blocks), dim3(64), a);
    HIP_TRY(ctx, hipMemcpyAsync(st_keys, d_misc + m_keys, m * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, sync_stream(ctx));
    for (size_t i = 0; i < m; i++)
      if (st_act[i]) out[base + i] = key_verdict(D, st_keys[i]);
  }
  host_phase(ctx, nullptr);
  return CP_OK;
}

// the bounds cp_verify_fri_queries_with_challenges puts on a shape, with its words
const char *hook_shape_problem(const cp_shape &sh) {
  if (sh.degree_bits < 2 || sh.degree_bits + sh.rate_bits > 30 || sh.rate_bits < 0 || sh.num_challenges < 1 || sh.num_challenges > 8 ||
      sh.n_arity < 0 || sh.n_arity > 8 || sh.cap_height < 0 || sh.cap_height > sh.degree_bits + sh.rate_bits || sh.num_query_rounds < 1 ||
      sh.num_query_rounds > 255 || sh.num_wires < 1 || sh.num_constants < 0 || sh.num_routed_wires < 0 || sh.num_partial_products < 0 ||
      sh.quotient_degree_factor < 1)
    return "shape out of range";
  for (int l = 0; l < sh.n_arity; l++)
    if (sh.arity_bits[l] < 1 || sh.arity_bits[l] > 5) return "FRI arity out of range";
  return nullptr;
}

}  // namespace

extern "C" int cp_verify_batch(cp_circuit *circ, const uint8_t *const *proofs, const size_t *proof_lens, size_t n_proofs, size_t chunk_proofs,
                               cp_verify_verdict *verdicts_out) try {
  if (!circ) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_ctx *ctx = circ->ctx;
  CHECK_CTX(ctx);
  if (!proofs || !proof_lens || !verdicts_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (n_proofs == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "no proofs");
  if (!circ->has_gates) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit has no gate set (cp_circuit_set_gates)");
  for (size_t p = 0; p < n_proofs; p++)
    if (!proofs[p] && proof_lens[p]) return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu is NULL", p);
  const cp_shape &sh = circ->sh;
  if (const char *why = hook_shape_problem(sh)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s", why);
  hostu::alloc_checkpoint();
  friv::Instance D;
  size_t proof_words;
  CP_TRY(plonky2_layout(ctx, sh, true, D, proof_words));
  std::vector<uint64_t> ks(sh.num_routed_wires);  // once per call, not once per proof
  if (!ks.empty()) HIP_TRY(ctx, hipMemcpy(ks.data(), circ->k_is, ks.size() * 8, hipMemcpyDeviceToHost));
  return verify_batch_passes(ctx, D, proof_words, circ->cs.cap_host.data(), proofs, proof_lens, n_proofs, chunk_proofs, PATHS_LANE, verdicts_out,
                             [&](size_t p, uint64_t *rec) { return verify_host_phase(*circ, ks.data(), proofs[p], proof_lens[p], rec); });
} CP_CATCH(circ ? circ->ctx : nullptr)

// Device twin of cp_verify_fri_queries_with_challenges: the query phase of n proofs of one shape with the challenges supplied
// per proof, through the kernels cp_verify_batch launches.
extern "C" int cp_verify_fri_queries_with_challenges_batch(cp_ctx *ctx, const cp_shape *shape, const uint64_t *cs_cap, const uint8_t *const *proofs,
                                                           const size_t *proof_lens, size_t n_proofs, const uint64_t *alphas, const uint64_t *zetas,
                                                           const uint64_t *fri_betas, const uint64_t *x_indices, size_t chunk_proofs,
                                                           cp_verify_verdict *verdicts_out) try {
  // the arguments first, the device last: what is wrong with a call is said without a GPU too
  if (!shape || !proofs || !proof_lens || !alphas || !zetas || !x_indices || !verdicts_out || (shape->n_arity > 0 && !fri_betas))
    return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (n_proofs == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "no proofs");
  const cp_shape &sh = *shape;
  if (const char *why = hook_shape_problem(sh)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s", why);
  if (const char *why = shape_problem(sh)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s", why);  // the kernels index by what the loader bounds
  const size_t nl = (size_t)sh.n_arity, nq = (size_t)sh.num_query_rounds;
  for (size_t p = 0; p < n_proofs; p++) {
    if (!proofs[p] && proof_lens[p]) return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu is NULL", p);
    bool canonical = alphas[2 * p] < gl::P && alphas[2 * p + 1] < gl::P && zetas[2 * p] < gl::P && zetas[2 * p + 1] < gl::P;
    for (size_t l = 0; l < 2 * nl; l++) canonical = canonical && fri_betas[2 * nl * p + l] < gl::P;
    if (!canonical) return set_error(ctx, CP_ERR_INVALID_ARG, "challenge is not canonical");
  }
  CHECK_CTX(ctx);
  hostu::alloc_checkpoint();
  friv::Instance D;
  size_t proof_words;
  CP_TRY(plonky2_layout(ctx, sh, cs_cap != nullptr, D, proof_words));
  return verify_batch_passes(ctx, D, proof_words, cs_cap, proofs, proof_lens, n_proofs, chunk_proofs, PATHS_LANE, verdicts_out, [&](size_t p, uint64_t *rec) {
    ParsedProof pp;
    if (parse_proof_bytes(nullptr, sh, nullptr, proofs[p], proof_lens[p], pp) != CP_OK) return parse_verdict();
    const gl::Ext alpha{alphas[2 * p], alphas[2 * p + 1]}, zeta{zetas[2 * p], zetas[2 * p + 1]};
    std::vector<gl::Ext> fb(nl);
    for (size_t l = 0; l < nl; l++) fb[l] = gl::Ext{fri_betas[2 * (nl * p + l)], fri_betas[2 * (nl * p + l) + 1]};
    FriVerifyInstance I;
    plonky2_fri_instance(sh, &pp, zeta, I);
    fill_record(I, alpha, fb.data(), x_indices + nq * p, rec);
    return verdict(0);
  });
} CP_CATCH(ctx)
