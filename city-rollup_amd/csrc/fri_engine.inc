// The FRI opening proof over ARBITRARY oracles and opening batches — plonky2 0.2.2 `PolynomialBatch::prove_openings`
// (batch polynomial per FriBatchInfo, `fri_proof`: commit phase, proof of work, query rounds) for B independent
// instances of one shape at once. `CircuitData::prove` is one client (four oracles, the batches at zeta and g*zeta:
// prover_tail.inc tail_fri); the C-ABI entry point cp_fri_prove (fri_prove.inc) is the other — what a STARK prover built on
// plonky2's FRI calls (starkyx `ByteStark::prove`: city_common_circuit/src/hash/accelerator/sha256/smartgadget.rs:518-524,
// which proves through `plonky2::{stark::config::GenericCombinedConfig, Plonky2Air}`, smartgadget.rs:48-49).
// Included by prover_tail.inc after its host helpers (arena, staging, ByteBuf, HostChallenger).

namespace {

struct FriCfg {  // plonky2 FriParams minus degree_bits
  int rate_bits, cap_height, pow_bits, num_query_rounds, n_arity;
  int arity_bits[8];
};

// one oracle (a PolynomialBatch per proof) as the engine sees it: fixed per-proof strides, or per-proof pointer tables
struct OracleRef {
  size_t k = 0;
  const uint64_t *coeffs = nullptr, *lde = nullptr, *digests = nullptr;
  size_t coeffs_stride = 0, lde_stride = 0, dig_stride = 0;
  const uint64_t *const *t_coeffs = nullptr, *const *t_lde = nullptr, *const *t_dig = nullptr;  // device tables [proof] or null
  const uint64_t *salt = nullptr;  // [proof][n_salt][N] extra leaf elements, else null
  size_t salt_stride = 0;
  int n_salt = 0;
};

struct FriBatchDesc {  // FriBatchInfo::polynomials as runs; the point lives in the zpow / zinv tables
  std::vector<cp_fri_poly_range> ranges;
  size_t n_polys = 0;
};

// What a FRI run leaves for the host, filled by ctx's next fetch_flush (the engine enqueues, it never synchronises): the
// caller flushes once — after it has enqueued its own outputs too — and then calls fri_bytes().
struct FriHostOut {
  FriCfg cfg{};
  size_t Bn = 0, cap_n = 0, words = 0, final_len = 0;
  std::vector<std::vector<uint64_t>> layer_caps;  // per layer: B x cap_n x 4
  std::vector<uint64_t> qwords, fin;              // B x nq x words ; B x final_len x 2
  std::vector<unsigned long long> best;           // B proof-of-work witnesses
  std::vector<unsigned> flags;                    // B: bit 0 = an opening point in the subgroup, bit 1 = proof-of-work check failed
  // bincode FriProof { commit_phase_merkle_caps, query_round_proofs, final_poly, pow_witness } of instance p, appended to out
  void bytes(size_t p, ByteBuf &out) const {
    const int nq = cfg.num_query_rounds;
    out.v.reserve(out.v.size() + 8 * (nq * words + 4096));
    out.u64(cfg.n_arity);
    for (int l = 0; l < cfg.n_arity; l++) { out.u64(cap_n); out.felts(layer_caps[l].data() + p * cap_n * 4, cap_n * 4); }
    out.u64(nq);
    out.felts(qwords.data() + p * nq * words, nq * words);
    out.u64(final_len); out.felts(fin.data() + p * 2 * final_len, 2 * final_len);
    out.u64(best[p]);
  }
  int check(cp_ctx *ctx) const {
    for (size_t p = 0; p < Bn; p++) {
      if (flags[p] & 1u) return set_error(ctx, CP_ERR_INTERNAL, "opening point is in the subgroup");
      if (flags[p] & 2u) return set_error(ctx, CP_ERR_INTERNAL, "proof of work response check failed");
      if (best[p] == ~0ull) return set_error(ctx, CP_ERR_INTERNAL, "proof of work search failed");
    }
    return CP_OK;
  }
};

// The Fiat-Shamir transcripts of a batch, in one of two places:
//   * on the DEVICE (transcript.h): a phase is one small launch and the whole proof is enqueued without a host round trip —
//     the mode of a batch: B chains advance side by side in 1.5 ms whatever B is, and no host thread hashes;
//   * on the HOST (HostChallenger on poseidon::permute_host, the integer round structure): a phase is one synchronisation, a
//     copy of what it observes, ~2.5 us per permutation and a copy of the challenges back. A lone chain is FASTER here (the
//     cooperative permutation needs ~13 us: the chain is sequential, 115 permutations, and one wave cannot out-run a CPU core
//     on it), so small batches (< 8 proofs) keep the host transcript — block latency depends on it (one block alone on three
//     contexts: 61.5 ms host or chosen per batch, 76-78 ms device; 64 blocks in flight: 31.7 blocks/s host, 34.6-35.0 device or
//     chosen per batch — profiles/r03_qbench_transcript_modes_v2.txt).
// Same bytes either way; everything that depends on a challenge is computed on the device from device memory in both modes.
// cp_ctx_set_device_transcript / CITYPROVER_DEVICE_TRANSCRIPT = 0 | 1 force a mode (measurements, tests).
struct Transcript {
  bool device = true;
  size_t Bn = 0;
  tr::DevCh *d_ch = nullptr;       // always allocated: the proof-of-work search reads its state from here
  std::vector<HostChallenger> C;   // host mode only

  static bool choose_device(const cp_ctx *ctx, size_t Bn) {
    const int env = (int)CP_KNOB(ctx, "DEVICE_TRANSCRIPT", -1);
    const int mode = ctx->transcript_mode >= 0 ? ctx->transcript_mode : env;
    return mode >= 0 ? mode != 0 : Bn >= 8;
  }
  // zero transcripts
  int init(cp_ctx *ctx, size_t n) {
    Bn = n;
    device = choose_device(ctx, n);
    CP_TRY(arena_alloc(ctx, n * sizeof(tr::DevCh), (void **)&d_ch));
    if (device) HIP_TRY(ctx, hipMemsetAsync(d_ch, 0, n * sizeof(tr::DevCh), ctx->stream));
    else C.assign(n, HostChallenger());
    return CP_OK;
  }
  static tr::DevCh pack(const HostChallenger &c) {
    tr::DevCh h;
    memcpy(h.state, c.state, sizeof h.state);
    memset(h.in, 0, sizeof h.in);
    memcpy(h.in, c.in, (size_t)c.n_in * 8);
    h.n_in = c.n_in;
    h.n_out = c.n_out;
    return h;
  }
  // transcripts (cp_fri_prove: one; cp_stark_prove_batch: one per instance) from states that crossed the ABI
  int init_from(cp_ctx *ctx, const HostChallenger *c, size_t n) {
    Bn = n;
    device = choose_device(ctx, n);
    CP_TRY(arena_alloc(ctx, n * sizeof(tr::DevCh), (void **)&d_ch));
    if (device) {
      std::vector<tr::DevCh> h(n);
      for (size_t p = 0; p < n; p++) h[p] = pack(c[p]);
      CP_TRY(push(ctx, d_ch, h.data(), n * sizeof(tr::DevCh)));
    } else {
      C.assign(c, c + n);
    }
    return CP_OK;
  }
  int init_from(cp_ctx *ctx, const HostChallenger &c) { return init_from(ctx, &c, 1); }
  // host mode: the device copy of the states (the proof-of-work kernels start from it)
  int states_to_device(cp_ctx *ctx) {
    if (device) return CP_OK;
    std::vector<tr::DevCh> h(Bn);
    for (size_t p = 0; p < Bn; p++) h[p] = pack(C[p]);
    return push(ctx, d_ch, h.data(), Bn * sizeof(tr::DevCh));
  }
};

// one transcript phase: observe `segs`, then draw n_chal challenges into chal[proof*stride + i] (device memory in both modes)
int transcript_step(cp_ctx *ctx, Transcript &T, std::initializer_list<tr::Seg> segs, int n_chal, uint64_t *chal, size_t stride) {
  const size_t Bn = T.Bn;
  if (T.device) {
    tr::StepArgs a;
    memset(&a, 0, sizeof a);
    a.ch = T.d_ch;
    a.n_proofs = (unsigned)Bn;
    for (const tr::Seg &s : segs) {
      if (a.n_seg >= tr::MAX_SEG) return set_error(ctx, CP_ERR_INTERNAL, "too many transcript segments");
      if (s.count) a.seg[a.n_seg++] = s;
    }
    a.n_chal = n_chal;
    a.chal = chal;
    a.chal_stride = stride;
    LAUNCH(ctx, "transcript_step", tr::k_step, dim3(blocks_for(Bn, pcoop::STATES_PER_WAVE)), dim3(64), a);
    return CP_OK;
  }
  // host mode: bring what is observed to the host (one synchronisation), hash, send the challenges back
  std::vector<std::vector<uint64_t>> data;
  std::vector<uint32_t> counts;
  for (const tr::Seg &s : segs) {
    if (!s.count) continue;
    if (s.table) return set_error(ctx, CP_ERR_INTERNAL, "host transcript: a segment behind a pointer table");
    data.emplace_back(Bn * (size_t)s.count);
    counts.push_back(s.count);
    if (s.proof_stride == s.count) {
      CP_TRY(fetch_async(ctx, data.back().data(), s.base, Bn * (size_t)s.count * 8));
    } else {
      for (size_t p = 0; p < Bn; p++) CP_TRY(fetch_async(ctx, data.back().data() + p * s.count, s.base + p * s.proof_stride, (size_t)s.count * 8));
    }
  }
  if (!data.empty()) CP_TRY(fetch_flush(ctx));
  std::vector<uint64_t> out(Bn * (size_t)n_chal);
  host_for(Bn, [&](size_t p) {
    for (size_t k = 0; k < data.size(); k++) T.C[p].observe(data[k].data() + p * counts[k], counts[k]);
    for (int i = 0; i < n_chal; i++) out[p * (size_t)n_chal + (size_t)i] = T.C[p].challenge();
  });
  if (n_chal) {
    if (stride != (size_t)n_chal) return set_error(ctx, CP_ERR_INTERNAL, "host transcript: challenges must be contiguous per proof");
    CP_TRY(push(ctx, chal, out.data(), out.size() * 8));
  }
  return CP_OK;
}

// zpow / zinv: powers of every instance's opening points and of their inverses, [(proof*n_batches + batch)*n + j].
// T: the transcripts, already past the commitments; `opened` (count may be 0): the opened values the transcript
// observes before alpha is drawn (plonky2 `observe_openings`; a caller that has observed them itself passes count 0).
// Advances the transcripts through alpha, the layer betas, the final polynomial, the proof-of-work witness and the query
// indices. Everything is ENQUEUED: `out` is valid after the caller's fetch_flush. d_flags: B words the caller has zeroed.
int fri_prove_impl(cp_ctx *ctx, size_t Bn, int db, const FriCfg &cfg, const std::vector<OracleRef> &oracles,
                   const std::vector<FriBatchDesc> &batches, const gl::Ext *zpow, const gl::Ext *zinv, Transcript &T, tr::Seg opened,
                   const int *use_pow, const uint64_t *pow_ov, unsigned *d_flags, FriHostOut &out) {
  const int rb = cfg.rate_bits, ch = cfg.cap_height;
  const size_t n = (size_t)1 << db, N = n << rb, cap_n = (size_t)1 << ch;
  const unsigned Bu = (unsigned)Bn;
  const size_t nb = batches.size();
  const int n_or = (int)oracles.size();
  if (n_or < 1 || n_or > fri::MAX_ORACLES) return set_error(ctx, CP_ERR_UNSUPPORTED, "1..%d oracles per FRI instance", fri::MAX_ORACLES);
  if (nb < 1) return set_error(ctx, CP_ERR_INVALID_ARG, "no opening batch");
  auto dalloc = [&](size_t bytes, void **p) -> int { return arena_alloc(ctx, bytes, p); };
  out.cfg = cfg;
  out.Bn = Bn;
  out.cap_n = cap_n;

  host_phase(ctx, "fri_batch_poly");
  // ---- batch polynomial: final = sum_b alpha^(k_{b+1} + ...) (F_b - F_b(z_b)) / (X - z_b),  F_b = sum_j alpha^j f_bj ------------
  size_t max_polys = 1;
  for (auto &b : batches) max_polys = b.n_polys > max_polys ? b.n_polys : max_polys;
  const size_t ap_stride = max_polys + 1;  // alpha^0 .. alpha^max_polys: the last entries are the batches' shift factors
  gl::Ext *d_alpha, *d_apow, *d_comp;
  CP_TRY(dalloc(Bn * 16, (void **)&d_alpha));
  CP_TRY(dalloc(Bn * ap_stride * 16, (void **)&d_apow));
  CP_TRY(dalloc(Bn * n * 16, (void **)&d_comp));
  CP_TRY(transcript_step(ctx, T, {opened}, 2, (uint64_t *)d_alpha, 2));
  LAUNCH(ctx, "fri_ext_powers", fri::k_ext_powers, dim3(blocks_for(ap_stride, 256), Bu), dim3(256), d_alpha, ap_stride, d_apow);
  uint64_t *fin, *vals0;
  CP_TRY(dalloc(Bn * 2 * n * 8, (void **)&fin));    // [proof][re | im][n]
  CP_TRY(dalloc(Bn * 2 * N * 8, (void **)&vals0));  // [proof][re | im][N], bit-reversed
  for (size_t b = 0; b < nb; b++) {
    const auto &R = batches[b].ranges;
    size_t done_polys = 0;
    for (size_t r0 = 0; r0 < R.size() || r0 == 0; r0 += fri::MAX_RANGES) {
      fri::BatchRefs refs;
      memset(&refs, 0, sizeof refs);
      refs.n = n;
      for (int o = 0; o < n_or; o++) {
        refs.base[o] = oracles[o].coeffs;
        refs.proof_stride[o] = oracles[o].coeffs_stride;
        refs.table[o] = oracles[o].t_coeffs;
      }
      size_t cnt = 0;
      for (size_t r = r0; r < R.size() && r < r0 + fri::MAX_RANGES; r++) {
        refs.r_oracle[refs.n_ranges] = (int)R[r].oracle;
        refs.r_first[refs.n_ranges] = (int)R[r].first;
        refs.r_count[refs.n_ranges] = (int)R[r].count;
        refs.n_ranges++;
        cnt += R[r].count;
      }
      // a launch that cannot fill the chip and walks a long list: the LIST is cut over more workgroups (fri.h k_combine_split)
      const size_t split = (n * Bn <= ((size_t)1 << 14) && cnt >= 64) ? std::min<size_t>(32, cnt / 16) : 1;
      if (split > 1) {
        gl::Ext *d_parts;
        CP_TRY(dalloc(split * Bn * n * 16, (void **)&d_parts));
        const int per = (int)((cnt + split - 1) / split);
        LAUNCH(ctx, "fri_combine", fri::k_combine_split, dim3(blocks_for(n, 256), Bu, (unsigned)split), dim3(256), refs, d_apow, ap_stride, done_polys,
               per, d_parts);
        LAUNCH(ctx, "fri_combine", fri::k_combine_reduce, dim3(blocks_for(n, 256), Bu), dim3(256), d_parts, (int)split, n, r0 == 0 ? 0 : 1, d_comp);
      } else
        LAUNCH(ctx, "fri_combine", fri::k_combine, dim3(blocks_for(n, 256), Bu), dim3(256), refs, d_apow, ap_stride, done_polys,
               r0 == 0 ? 0 : 1, d_comp);
      done_polys += cnt;
      if (R.empty()) break;
    }
    // ReducingFactor::shift_poly: final = final * alpha^(#polynomials of THIS batch) + quotient
    LAUNCH(ctx, "fri_divide_linear", fri::k_divide_linear_accumulate, dim3(1, Bu), dim3(256), d_comp, zpow + b * n, zinv + b * n, nb * n, n,
           d_apow + batches[b].n_polys, ap_stride, b == 0 ? 1 : 0, fin);
  }
  CP_TRY(cp_lde_dev(ctx, fin, n, db, rb, 2 * Bn, 7, CP_NTT_BITREV_OUT, vals0, N));

  host_phase(ctx, "fri_commit");
  // ---- commit phase (plonky2 `fri_committed_trees`) ---------------------------------------------------------------------
  struct Layer { uint64_t *vals, *dig, *cap; size_t n_vals, n_leaves, dig_stride; int depth; };
  std::vector<Layer> layers(cfg.n_arity);
  out.layer_caps.assign(cfg.n_arity, {});
  uint64_t *coef = fin;
  size_t coef_phys = n, clen = N;  // physical array length / logical length (zero beyond coef_phys)
  uint64_t *vals = vals0;
  uint64_t shift = 7;
  int clog = db + rb;
  gl::Ext *d_betas;
  CP_TRY(dalloc((size_t)(cfg.n_arity ? cfg.n_arity : 1) * Bn * 16, (void **)&d_betas));
  for (int l = 0; l < cfg.n_arity; l++) {
    Layer &L = layers[l];
    const int ab = cfg.arity_bits[l], arity = 1 << ab;
    // k_leaf_hash_fri reads a hashed leaf (more than four words) as whole chunks, without a bound on the last one
    if (2 * arity > 4 && (2 * arity) % poseidon::RATE) return set_error(ctx, CP_ERR_INTERNAL, "FRI leaf of %d words is not whole sponge chunks", 2 * arity);
    L.vals = vals;
    L.n_vals = clen;
    L.n_leaves = clen >> ab;
    L.depth = ilog2(L.n_leaves) - ch;
    if (L.depth < 0) L.depth = 0;
    L.dig_stride = merkle_words_per_tree(L.n_leaves, ch);
    CP_TRY(dalloc(Bn * L.dig_stride * 8, (void **)&L.dig));
    CP_TRY(dalloc(Bn * cap_n * 32, (void **)&L.cap));
    if (L.n_leaves * Bn <= coop_leaf_max(ctx))  // a launch that cannot fill the chip: twelve lanes per leaf (poseidon_coop.h)
      LAUNCH(ctx, "fri_leaf_hash_coop", pcoop::k_leaf_hash_fri_coop, dim3(blocks_for(L.n_leaves, pcoop::STATES_PER_BLOCK), Bu), dim3(256), vals,
             2 * clen, clen, L.n_leaves, arity, L.dig, L.dig_stride);
    else
      LAUNCH(ctx, "fri_leaf_hash", fri::k_leaf_hash_fri, dim3(blocks_for(L.n_leaves, 256), Bu), dim3(256), vals, 2 * clen,
             clen, L.n_leaves, arity, L.dig, L.dig_stride);
    CP_TRY(merkle_levels(ctx, L.dig, L.dig_stride, L.n_leaves, Bn, ch, L.cap));
    out.layer_caps[l].resize(Bn * cap_n * 4);
    CP_TRY(fetch_async(ctx, out.layer_caps[l].data(), L.cap, out.layer_caps[l].size() * 8));
    gl::Ext *beta_l = d_betas + (size_t)l * Bn;
    CP_TRY(transcript_step(ctx, T, {tr::Seg{L.cap, nullptr, cap_n * 4, (uint32_t)(cap_n * 4)}}, 2, (uint64_t *)beta_l, 2));
    // fold the coefficients, then evaluate them on the next coset
    const size_t nlen = clen >> ab;
    uint64_t *ncoef, *nvals;
    CP_TRY(dalloc(Bn * 2 * nlen * 8, (void **)&ncoef));
    CP_TRY(dalloc(Bn * 2 * nlen * 8, (void **)&nvals));
    LAUNCH(ctx, "fri_fold", fri::k_fold, dim3(blocks_for(nlen, 256), Bu), dim3(256), coef, 2 * coef_phys, coef_phys, nlen,
           arity, beta_l, ncoef, 2 * nlen);
    coef = ncoef; coef_phys = nlen; clen = nlen; clog -= ab;
    shift = gl::pow(shift, (uint64_t)arity);
    CP_TRY(cp_d2d(ctx, nvals, ncoef, Bn * 2 * nlen * 8));
    CP_TRY(cp_ntt_dev(ctx, nvals, clog, 2 * Bn, nlen, CP_NTT_COSET | CP_NTT_BITREV_OUT, shift));
    vals = nvals;
  }
  const size_t final_len = clen >> rb;
  // the coefficient array is [proof][re | im][coef_phys]; without any reduction layer coef_phys = n < clen = N
  // (the logical polynomial is zero beyond n), so index by the PHYSICAL length
  if (final_len > coef_phys) return set_error(ctx, CP_ERR_INTERNAL, "final polynomial longer than its coefficient array");
  out.final_len = final_len;
  uint64_t *d_fin;
  CP_TRY(dalloc(Bn * 2 * final_len * 8 + 8, (void **)&d_fin));
  if (final_len)
    LAUNCH(ctx, "fri_pack_final", tr::k_pack_final, dim3(blocks_for(final_len, 64), Bu), dim3(64), coef, coef_phys, final_len, d_fin);
  out.fin.resize(Bn * 2 * final_len);
  CP_TRY(fetch_async(ctx, out.fin.data(), d_fin, out.fin.size() * 8));
  CP_TRY(transcript_step(ctx, T, {tr::Seg{d_fin, nullptr, 2 * final_len, (uint32_t)(2 * final_len)}}, 0, nullptr, 0));

  host_phase(ctx, "pow");
  // ---- proof of work: smallest witness ----------------------------------------------------------------
  // The smallest valid witness is geometric with mean 2^pow_bits; everything below it must be tried anyway. The persistent
  // workgroups of k_pow_grind take the candidates range by range, in increasing order, and stop at each proof's first witness,
  // so what is computed beyond it is only what was in flight at that moment. ONE launch: it offers 2^39 candidates per proof
  // and ends when every proof has its witness (a search that long does not fail).
  fri::PowState *d_ps;
  unsigned long long *d_best, *d_done;
  unsigned *d_next;
  int *d_use = nullptr;
  uint64_t *d_ov = nullptr;
  CP_TRY(dalloc(Bn * sizeof(fri::PowState), (void **)&d_ps));
  CP_TRY(dalloc(Bn * 8, (void **)&d_best));
  CP_TRY(dalloc(Bn * 8, (void **)&d_done));
  CP_TRY(dalloc(Bn * sizeof(unsigned), (void **)&d_next));
  bool any = false;
  for (size_t p = 0; p < Bn; p++) any = any || !(use_pow && use_pow[p]);
  any = any && cfg.pow_bits > 0;
  if (use_pow) {
    CP_TRY(dalloc(Bn * sizeof(int), (void **)&d_use));
    CP_TRY(dalloc(Bn * 8, (void **)&d_ov));
    CP_TRY(push(ctx, d_use, use_pow, Bn * sizeof(int)));
    CP_TRY(push(ctx, d_ov, pow_ov, Bn * 8));
  }
  CP_TRY(T.states_to_device(ctx));
  LAUNCH(ctx, "fri_pow_prepare", tr::k_pow_prepare, dim3(blocks_for(Bn, 64)), dim3(64), T.d_ch, Bu, cfg.pow_bits, d_use, d_ov, d_ps, d_best, d_done);
  if (any) {
    // workgroups in flight = the overshoot (each finishes the range it holds): about one expected search length per
    // proof, at most 8 per CU, at least 64
    uint64_t want = cfg.pow_bits >= 8 ? Bn << (cfg.pow_bits - 8) : Bn;
    want = want < 64 ? 64 : (want > 2048 ? 2048 : want);
    HIP_TRY(ctx, hipMemsetAsync(d_next, 0, Bn * sizeof(unsigned), ctx->stream));
    LAUNCH(ctx, "fri_pow_grind", fri::k_pow_grind, dim3((unsigned)want), dim3(256), d_ps, (uint64_t)0, (uint64_t)1 << 39, cfg.pow_bits, Bu, d_done,
           d_best, d_next);
  }
  out.best.assign(Bn, ~0ull);
  CP_TRY(fetch_async(ctx, out.best.data(), d_best, Bn * 8));
  const int nq = cfg.num_query_rounds;
  uint64_t *d_resp, *d_idx;
  CP_TRY(dalloc(Bn * (size_t)(nq + 1) * 8, (void **)&d_resp));
  CP_TRY(dalloc(Bn * (size_t)nq * 8, (void **)&d_idx));
  CP_TRY(transcript_step(ctx, T, {tr::Seg{(const uint64_t *)d_best, nullptr, 1, 1}}, nq + 1, d_resp, (size_t)nq + 1));
  LAUNCH(ctx, "fri_query_indices", tr::k_query_indices, dim3(blocks_for(Bn * (size_t)(nq + 1), 64)), dim3(64), d_resp, Bu, nq, (uint64_t)N,
         cfg.pow_bits, d_use, d_idx, d_flags);

  host_phase(ctx, "queries");
  // ---- query phase (plonky2 `fri_prover_query_rounds`) -------------------------------------------------------------------
  fri::QueryRefs qr;
  memset(&qr, 0, sizeof qr);
  const int depth0 = db + rb - ch;
  size_t words = 1;
  qr.n_oracles = n_or;
  for (int b = 0; b < n_or; b++) {
    const OracleRef &O = oracles[b];
    qr.lde[b] = O.lde; qr.digests[b] = O.digests; qr.k[b] = (int)O.k;
    qr.lde_table[b] = O.t_lde; qr.dig_table[b] = O.t_dig;
    qr.lde_stride[b] = O.lde_stride; qr.dig_stride[b] = O.dig_stride;
    qr.salt[b] = O.salt; qr.salt_stride[b] = O.salt_stride; qr.n_salt[b] = O.n_salt;
    words += 1 + O.k + (O.salt ? O.n_salt : 0) + 1 + (size_t)depth0 * 4;
  }
  qr.N = N; qr.depth0 = depth0; qr.n_layers = cfg.n_arity; qr.n_queries = nq;
  words += 1;
  for (int l = 0; l < cfg.n_arity; l++) {
    qr.fvals[l] = layers[l].vals; qr.fvals_stride[l] = 2 * layers[l].n_vals; qr.f_nvals[l] = layers[l].n_vals;
    qr.fdig[l] = layers[l].dig; qr.fdig_stride[l] = layers[l].dig_stride;
    qr.f_leaves[l] = layers[l].n_leaves; qr.f_arity_bits[l] = cfg.arity_bits[l]; qr.f_depth[l] = layers[l].depth;
    words += 1 + ((size_t)2 << cfg.arity_bits[l]) + 1 + (size_t)layers[l].depth * 4;
  }
  qr.words_per_query = words;
  out.words = words;
  uint64_t *d_q;
  CP_TRY(dalloc(Bn * nq * words * 8, (void **)&d_q));
  LAUNCH(ctx, "fri_gather_queries", fri::k_gather_queries, dim3(nq, Bu), dim3(256), qr, d_idx, d_q);
  out.qwords.resize(Bn * nq * words);
  CP_TRY(fetch_async(ctx, out.qwords.data(), d_q, out.qwords.size() * 8));
  out.flags.assign(Bn, 0);
  CP_TRY(fetch_async(ctx, out.flags.data(), d_flags, Bn * sizeof(unsigned)));
  return CP_OK;
}

// FriParams sanity shared by the circuit loader, cp_fri_prove and cp_fri_verify
const char *fri_cfg_problem(int db, const FriCfg &c) {
  if (db < 0 || c.rate_bits < 0 || db + c.rate_bits > 30 || db + c.rate_bits < 1) return "degree_bits / rate_bits out of range";
  if (c.n_arity < 0 || c.n_arity > 8) return "0..8 FRI reduction layers";
  if (c.cap_height < 0 || c.cap_height > db + c.rate_bits) return "cap_height out of range";
  if (c.pow_bits < 0 || c.pow_bits > 32) return "proof_of_work_bits out of range [0, 32]";
  if (c.num_query_rounds < 1 || c.num_query_rounds > 255) return "num_query_rounds out of range [1, 255]";
  int bits = db + c.rate_bits;
  for (int l = 0; l < c.n_arity; l++) {
    if (c.arity_bits[l] < 1 || c.arity_bits[l] > 5) return "FRI arity out of range";
    bits -= c.arity_bits[l];
    if (bits < c.cap_height || bits < c.rate_bits) return "FRI reduction schedule too deep for this degree";
  }
  return nullptr;
}

}  // namespace
