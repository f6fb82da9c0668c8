// C ABI of the generic AIR machinery (include/cityprover.h "the STARK's own two steps as GENERIC device machinery"): programs
// (air.h), the quotient of a STARK straight from committed traces, map programs, the two logUp primitives (ext3.h), and the
// prover / verifier strung from them and the two plonky2-level seams (fri_prove.inc). Reference call site of such a prover:
// starkyx `ByteStark::prove`, city_common_circuit/src/hash/accelerator/sha256/smartgadget.rs:518-524 (verified natively at
// :524), called from city_rollup_circuit/src/sighash_circuits/sighash.rs:132-146. Included at the end of cityprover.hip.

struct cp_air_program {
  cp_ctx *ctx = nullptr;
  int device = 0;
  air::Program P;
  air::Compiled single;  // the one-segment form (cp_air_program_get_info; map programs run it)
  struct Variant {
    air::Compiled C;
    DevBuf d_code, d_seg_off;  // uint64_t / uint32_t
  };
  std::mutex m;
  std::map<uint32_t, Variant> variants;  // segments asked for -> the compiled form on the device
};

namespace {

// CITYPROVER_AIR_PREFETCH=1: column operands are loaded into slots in batches ahead of their use instead of at their use. Measured
// on the SHA-256-STARK-shaped quotient (profiles/r04_air_ab.jsonl): no gain at any size - the interpreter is bound by its scalar
// decode work, not by load latency, and a prefetched column is one more interpreted instruction (+28 %). Off by default.
bool air_prefetch() {
  static const bool on = getenv("CITYPROVER_AIR_PREFETCH") && atoi(getenv("CITYPROVER_AIR_PREFETCH")) != 0;
  return on;
}
// slots kept in LDS (the rest in global scratch): 512 B per slot and wave, so this bounds the waves a CU holds
uint32_t air_lds_slots(cp_ctx *ctx) {
  const uint32_t v = (uint32_t)CP_KNOB(ctx, "AIR_LDS_SLOTS", air::MAX_LDS_SLOTS);
  return std::max(1u, std::min(v, 120u));
}

int air_variant(cp_ctx *ctx, cp_air_program *prog, uint32_t want, const cp_air_program::Variant **out) {
  std::lock_guard<std::mutex> l(prog->m);
  auto it = prog->variants.find(want);
  if (it == prog->variants.end()) {
    cp_air_program::Variant v;
    // A segment recomputes whatever it shares with its neighbours. When the constraints share deep subexpressions, cutting finer
    // multiplies the work instead of spreading it: halve the cut until the segments together are at most three times the one-segment form.
    uint32_t cut = want;
    for (;;) {
      v.C = cut == 1 ? prog->single : air::compile(prog->P, cut, air_prefetch());
      if (cut == 1 || v.C.code.size() <= 3 * prog->single.code.size() + 64) break;
      cut >>= 1;
    }
    if (v.C.n_slots >= air::DST_NONE) return set_error(ctx, CP_ERR_UNSUPPORTED, "the program needs %u live temporaries (limit %u)", v.C.n_slots, air::DST_NONE - 1);
    const size_t cb = (v.C.code.size() ? v.C.code.size() : 1) * 8, sb = v.C.seg_off.size() * 4;
    v.d_code = DevBuf(dev_pool(), prog->device);
    v.d_seg_off = DevBuf(dev_pool(), prog->device);
    CP_TRY(alloc_status(ctx, v.d_code.alloc(cb), cb));
    CP_TRY(alloc_status(ctx, v.d_seg_off.alloc(sb), sb));
    HIP_TRY(ctx, hipMemcpyAsync(v.d_code.get(), v.C.code.data(), v.C.code.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(v.d_seg_off.get(), v.C.seg_off.data(), sb, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the host vectors may move when the map grows
    it = prog->variants.emplace(want, std::move(v)).first;
  }
  *out = &it->second;
  return CP_OK;
}

// z_last / L_0 / L_(n-1) on the quotient coset, cached per (degree_bits, q) and context
int air_selectors(cp_ctx *ctx, int db, int q, const uint64_t **out) {
  auto key = std::make_pair(db, q);
  auto it = ctx->air_sel_tables.find(key);
  if (it != ctx->air_sel_tables.end()) { *out = it->second.get<uint64_t>(); return CP_OK; }
  const int log_M = db + q;
  const size_t M = (size_t)1 << log_M, n = (size_t)1 << db;
  uint64_t wM = gl::pow(7, (gl::P - 1) >> 32);
  for (int i = log_M; i < 32; i++) wM = gl::sqr(wM);
  uint64_t g = wM;
  for (int i = 0; i < q; i++) g = gl::sqr(g);
  const uint64_t *otab = nullptr;
  CP_TRY(get_pow_table(ctx, wM, &otab));
  DevBuf tab = ctx->buf();
  CP_TRY(alloc_status(ctx, tab.alloc(3 * M * 8), 3 * M * 8));
  LAUNCH(ctx, "air_selectors", air::k_selectors, dim3(blocks_for(M, 256)), dim3(256), tab.get<uint64_t>(), M, log_M, db, otab, gl::pow(g, n - 1),
         gl::inv((uint64_t)n % gl::P));
  *out = tab.get<uint64_t>();
  ctx->air_sel_tables[key] = std::move(tab);
  return CP_OK;
}

bool all_canonical(const uint64_t *v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (v[i] >= gl::P) return false;
  return true;
}

// consts | publics | globals | challenges | 0
int air_uniform_table(cp_ctx *ctx, const air::Program &P, const uint64_t *publics, const uint64_t *globals, const uint64_t *challenges,
                      std::vector<uint64_t> &uni) {
  if ((P.n_public && !publics) || (P.n_global && !globals) || (P.n_challenge && !challenges)) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL publics / globals / challenges");
  if (!all_canonical(publics, P.n_public) || !all_canonical(globals, P.n_global) || !all_canonical(challenges, P.n_challenge))
    return set_error(ctx, CP_ERR_INVALID_ARG, "a public input / global value / challenge is not canonical");
  uni.assign(P.consts.begin(), P.consts.end());
  uni.insert(uni.end(), publics, publics + P.n_public);
  uni.insert(uni.end(), globals, globals + P.n_global);
  uni.insert(uni.end(), challenges, challenges + P.n_challenge);
  uni.push_back(0);
  return CP_OK;
}

// the tables of Bn instances, [instance][uni_size]; publics / globals / challenges: [instance][n_public / n_global / n_challenge]
int air_uniform_tables(cp_ctx *ctx, const air::Program &P, size_t Bn, const uint64_t *publics, const uint64_t *globals, const uint64_t *challenges,
                       std::vector<uint64_t> &uni) {
  std::vector<uint64_t> one;
  uni.clear();
  for (size_t i = 0; i < Bn; i++) {
    CP_TRY(air_uniform_table(ctx, P, publics ? publics + i * P.n_public : nullptr, globals ? globals + i * P.n_global : nullptr,
                             challenges ? challenges + i * P.n_challenge : nullptr, one));
    uni.insert(uni.end(), one.begin(), one.end());
  }
  return CP_OK;
}

// how many segments a launch over `waves` waves of points is cut into: enough to fill the chip a few times over
uint32_t air_segments_for(cp_ctx *ctx, size_t waves, size_t n_roots) {
  const size_t target = (size_t)CP_KNOB(ctx, "AIR_TARGET_WAVES", 8192);
  size_t s = 1;
  while (s * waves < target && s < 1024) s <<= 1;
  while (s > 1 && s > n_roots) s >>= 1;
  return (uint32_t)s;
}

// points per lane of the interpreter (air.h Vec<K>): one decoded instruction - the scalar work that bounds the kernel - then serves
// K x 64 points. CITYPROVER_AIR_POINTS_PER_LANE = 1, 2 or 4.
int air_points_per_lane(cp_ctx *ctx) {
  const int v = (int)CP_KNOB(ctx, "AIR_POINTS_PER_LANE", 2);
  return v >= 4 ? 4 : v >= 2 ? 2 : 1;
}

// shared memory a workgroup of this context's device may ask for (160 KiB per CU on gfx950, but ask the device)
int device_lds_per_block(cp_ctx *ctx, size_t &out) {
  if (!ctx->lds_per_block) {
    int v = 0;
    HIP_TRY(ctx, hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    if (v <= 0) return set_error(ctx, CP_ERR_HIP, "the device reports no shared memory per workgroup");
    ctx->lds_per_block = (size_t)v;
  }
  out = ctx->lds_per_block;
  return CP_OK;
}

// one launch for Bn instances of the program (grid z; the per-instance strides of ka are the caller's)
int air_run(cp_ctx *ctx, const char *name, bool map_mode, const cp_air_program::Variant &V, air::KArgs &ka, int K, size_t Bn = 1) {
  const uint32_t S = V.C.n_segments();
  const size_t blocks = (ka.M + (size_t)air::WAVE * K - 1) / ((size_t)air::WAVE * K);
  // a slot takes K x 64 x 8 B of the workgroup's (one wave's) LDS: at most as many slots in LDS as the device grants a workgroup
  size_t lds_max = 0;
  CP_TRY(device_lds_per_block(ctx, lds_max));
  const uint32_t lds_fit = (uint32_t)std::min<size_t>(lds_max / ((size_t)K * air::WAVE * 8), air::DST_NONE);
  if (lds_fit < 1) return set_error(ctx, CP_ERR_UNSUPPORTED, "one AIR slot (%zu B) exceeds the device's %zu B of LDS per workgroup", (size_t)K * air::WAVE * 8, lds_max);
  const uint32_t n_lds = std::min({V.C.n_slots, air_lds_slots(ctx), lds_fit}), n_spill = V.C.n_slots - n_lds;
  ka.code = V.d_code.get<uint64_t>();
  ka.seg_off = V.d_seg_off.get<uint32_t>();
  ka.n_lds = (int)n_lds;
  ka.spill_stride = Bn * S * blocks * K * air::WAVE;
  ka.spill = nullptr;
  if (n_spill) CP_TRY(arena_alloc(ctx, (size_t)n_spill * ka.spill_stride * 8, (void **)&ka.spill));
  const size_t lds_bytes = (size_t)(n_lds ? n_lds : 1) * K * air::WAVE * 8;
  if (blocks > 0x7FFFFFFFull || S > 65535 || Bn > 65535) return set_error(ctx, CP_ERR_UNSUPPORTED, "AIR launch too large");
  const dim3 grid((unsigned)blocks, S, (unsigned)Bn), block(air::WAVE);
#define CP_AIR_LAUNCH(MODE, KP) LAUNCH_LDS(ctx, name, (air::k_run<MODE, KP>), grid, block, lds_bytes, ka)
  if (map_mode) {
    if (K == 4) CP_AIR_LAUNCH(1, 4); else if (K == 2) CP_AIR_LAUNCH(1, 2); else CP_AIR_LAUNCH(1, 1);
  } else {
    if (K == 4) CP_AIR_LAUNCH(0, 4); else if (K == 2) CP_AIR_LAUNCH(0, 2); else CP_AIR_LAUNCH(0, 1);
  }
#undef CP_AIR_LAUNCH
  return CP_OK;
}

// The quotient chunks of Bn instances of one constraint program as COEFFICIENTS, d_q [instance][na << q][n]: the interpreter over
// the quotient coset (one launch, the instance a grid dimension), the sum of the segments over Z_H, the coset iNTT. cols:
// [instance][n_columns] device pointers to the committed columns on the LDE coset; uni: [instance][uni_size] (air_uniform_tables);
// alphas: [instance][na], canonical. Enqueued on the context's stream; the tables live in the caller's arena scope.
int air_quotient_coeffs(cp_ctx *ctx, cp_air_program *prog, size_t Bn, const std::vector<const uint64_t *> &cols, int db, int q,
                        const std::vector<uint64_t> &uni, const uint64_t *alphas, uint32_t na, uint64_t *d_q) {
  const air::Program &P = prog->P;
  const int log_M = db + q;
  const size_t n = (size_t)1 << db, M = n << q;
  // a lane takes several points once the traces alone give every SIMD a few waves' worth of them
  int K = air_prefetch() ? 1 : air_points_per_lane(ctx);
  while (K > 1 && Bn * M < (size_t)air::WAVE * K * 64) K >>= 1;
  const uint32_t want = air_segments_for(ctx, Bn * ((M + (size_t)air::WAVE * K - 1) / ((size_t)air::WAVE * K)), P.roots.size());
  const cp_air_program::Variant *V = nullptr;
  CP_TRY(air_variant(ctx, prog, want, &V));
  const uint32_t S = V->C.n_segments();
  // host-side tables: segment weights alpha^(sinks after the segment) per instance, 1 / Z_H on the coset
  std::vector<uint64_t> weights(Bn * S * na), zh_inv((size_t)1 << q);
  for (size_t i = 0; i < Bn; i++)
    for (uint32_t s = 0; s < S; s++)
      for (uint32_t c = 0; c < na; c++) weights[(i * S + s) * na + c] = gl::pow(alphas[i * na + c], V->C.sinks_after[s]);
  {
    uint64_t wq = gl::pow(7, (gl::P - 1) >> 32);  // primitive 2^q-th root: x^n on the coset takes the values 7^n wq^c
    for (int i = q; i < 32; i++) wq = gl::sqr(wq);
    const uint64_t sn = gl::pow(7, n);
    uint64_t w = 1;
    for (size_t c = 0; c < zh_inv.size(); c++) {
      zh_inv[c] = gl::inv(gl::sub(gl::mul(sn, w), 1));
      w = gl::mul(w, wq);
    }
  }
  air::KArgs ka{};
  uint64_t *d_uni, *d_alphas, *d_weights, *d_zh, *d_parts;
  const uint64_t **d_cols;
  CP_TRY(arena_alloc(ctx, uni.size() * 8, (void **)&d_uni));
  CP_TRY(arena_alloc(ctx, cols.size() * 8, (void **)&d_cols));
  CP_TRY(arena_alloc(ctx, Bn * na * 8, (void **)&d_alphas));
  CP_TRY(arena_alloc(ctx, weights.size() * 8, (void **)&d_weights));
  CP_TRY(arena_alloc(ctx, zh_inv.size() * 8, (void **)&d_zh));
  CP_TRY(arena_alloc(ctx, Bn * S * na * M * 8, (void **)&d_parts));
  CP_TRY(push(ctx, d_uni, uni.data(), uni.size() * 8));
  CP_TRY(push(ctx, d_cols, cols.data(), cols.size() * 8));
  CP_TRY(push(ctx, d_alphas, alphas, Bn * na * 8));
  CP_TRY(push(ctx, d_weights, weights.data(), weights.size() * 8));
  CP_TRY(push(ctx, d_zh, zh_inv.data(), zh_inv.size() * 8));
  const uint64_t *sel = nullptr;
  CP_TRY(air_selectors(ctx, db, q, &sel));
  ka.uni = d_uni; ka.cols = d_cols; ka.sel = sel; ka.alphas = d_alphas; ka.weights = d_weights; ka.parts = d_parts; ka.out_cols = nullptr;
  ka.M = M; ka.degree_bits = db; ka.n_alphas = (int)na;
  if (Bn > 1) {
    ka.uni_stride = uni.size() / Bn; ka.cols_stride = P.n_columns; ka.alphas_stride = na; ka.weights_stride = (size_t)S * na;
    ka.parts_stride = (size_t)S * na * M;
  }
  CP_TRY(air_run(ctx, "air_quotient", false, *V, ka, K, Bn));
  LAUNCH(ctx, "air_finish", air::k_finish, dim3(blocks_for(M, air::WAVE), (unsigned)Bn), dim3(256), d_parts, ka.parts_stride, S, (int)na, M, log_M, q,
         d_zh, d_q, (size_t)na * M);
  // values on 7<omega_M>, natural order -> coefficients; the 2^q chunks of n of every challenge are consecutive
  return cp_ntt_dev(ctx, d_q, log_M, Bn * na, M, CP_NTT_INVERSE | CP_NTT_COSET, 7);
}

// One map program on Bn column arrays that lie inst_stride elements apart (in_cols and out_cols alike): one launch. uni as above.
int air_map_launch(cp_ctx *ctx, cp_air_program *prog, size_t Bn, const uint64_t *in_cols, uint64_t *out_cols, size_t inst_stride, size_t n,
                   const std::vector<uint64_t> &uni) {
  const air::Program &P = prog->P;
  // the stores of a map program are independent roots: cut like the constraints of a quotient, so that a short trace (2^10 rows are
  // sixteen waves) still fills the chip - as ONE segment the 912-column map of the SHA-shaped STARK was 1.24 ms of a 7 ms proof
  const cp_air_program::Variant *V = nullptr;
  CP_TRY(air_variant(ctx, prog, air_segments_for(ctx, Bn * ((n + air::WAVE - 1) / air::WAVE), P.roots.size()), &V));
  std::vector<const uint64_t *> cols(Bn * P.n_columns);
  std::vector<uint64_t *> outs(Bn * P.n_out_columns);
  for (size_t i = 0; i < Bn; i++) {
    for (size_t c = 0; c < P.n_columns; c++) cols[i * P.n_columns + c] = in_cols + i * inst_stride + c * n;
    for (size_t c = 0; c < P.n_out_columns; c++) outs[i * P.n_out_columns + c] = out_cols + i * inst_stride + c * n;
  }
  air::KArgs ka{};
  uint64_t *d_uni;
  const uint64_t **d_cols;
  uint64_t **d_outs;
  CP_TRY(arena_alloc(ctx, uni.size() * 8, (void **)&d_uni));
  CP_TRY(arena_alloc(ctx, (cols.size() ? cols.size() : 1) * 8, (void **)&d_cols));
  CP_TRY(arena_alloc(ctx, (outs.size() ? outs.size() : 1) * 8, (void **)&d_outs));
  CP_TRY(push(ctx, d_uni, uni.data(), uni.size() * 8));
  CP_TRY(push(ctx, d_cols, cols.data(), cols.size() * 8));
  CP_TRY(push(ctx, d_outs, outs.data(), outs.size() * 8));
  ka.uni = d_uni; ka.cols = d_cols; ka.out_cols = d_outs; ka.M = n; ka.degree_bits = 0; ka.n_alphas = 0;
  if (Bn > 1) { ka.uni_stride = uni.size() / Bn; ka.cols_stride = P.n_columns; ka.out_cols_stride = P.n_out_columns; }
  return air_run(ctx, "air_map", true, *V, ka, 1, Bn);
}

// the raw program on one row over F_p^2 (a verifier at zeta): values of every op
void air_eval_ext_row(const air::Program &P, const gl::Ext *local, const gl::Ext *next, const gl::Ext *publics, const gl::Ext *globals,
                      const gl::Ext *challenges, std::vector<gl::Ext> &vals) {
  vals.assign(P.ops.size(), gl::Ext{0, 0});
  for (size_t i = 0; i < P.ops.size(); i++) {
    const air::RawOp &o = P.ops[i];
    switch (o.op) {
      case air::R_LOCAL: vals[i] = local[o.a]; break;
      case air::R_NEXT: vals[i] = next[o.a]; break;
      case air::R_PUBLIC: vals[i] = publics[o.a]; break;
      case air::R_GLOBAL: vals[i] = globals[o.a]; break;
      case air::R_CHALLENGE: vals[i] = challenges[o.a]; break;
      case air::R_CONST: vals[i] = gl::Ext{P.consts[o.a], 0}; break;
      case air::R_ADD: vals[i] = gl::ext_add(vals[o.a], vals[o.b]); break;
      case air::R_SUB: vals[i] = gl::ext_sub(vals[o.a], vals[o.b]); break;
      case air::R_MUL: vals[i] = gl::ext_mul(vals[o.a], vals[o.b]); break;
      case air::R_NEG: vals[i] = gl::ext_sub(gl::Ext{0, 0}, vals[o.a]); break;
      case air::R_INV: vals[i] = (vals[o.a].a | vals[o.a].b) ? host_ext_inv(vals[o.a]) : gl::Ext{0, 0}; break;
      default: break;
    }
  }
}

// A map program must not load a column it also stores (air.h map_self_read: the stores run as concurrent segments). in / out: byte
// addresses of the first input / output column, or indices scaled by n * 8; step < 0: a call of cp_air_map_dev, not a STARK step.
int map_self_read_refused(cp_ctx *ctx, const air::Program &P, uint64_t in, uint64_t out, size_t n, long step) {
  uint32_t in_col = 0, out_col = 0;
  if (!air::map_self_read(P, in, out, n, &in_col, &out_col)) return CP_OK;
  if (step < 0) return set_error(ctx, CP_ERR_INVALID_ARG, "the map program loads extended column %u, which it also stores", out_col);
  return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: the map program loads extended column %u, which it also stores", (size_t)step, out_col);
}

struct StarkShape {
  int db, rb, ch, q;
  size_t n, k0, k1, kt, kq;
  uint32_t na;
};
// everything about a cp_stark_desc that prover and verifier check alike
int stark_shape(cp_ctx *ctx, const cp_stark_desc *d, bool prover, StarkShape &s) {
  if (!d) return set_error(ctx, CP_ERR_INVALID_ARG, "desc is NULL");
  FriCfg cfg;
  CP_TRY(load_fri_cfg(ctx, &d->fri, cfg));
  if (d->fri.degree_bits != d->degree_bits) return set_error(ctx, CP_ERR_INVALID_ARG, "fri.degree_bits %d != degree_bits %d", d->fri.degree_bits, d->degree_bits);
  s.db = d->degree_bits; s.rb = d->fri.rate_bits; s.ch = d->fri.cap_height; s.q = d->quotient_degree_bits;
  if (s.q < 0 || s.q > s.rb) return set_error(ctx, CP_ERR_INVALID_ARG, "quotient_degree_bits %d out of range [0, rate_bits %d]", s.q, s.rb);
  if (d->num_challenges < 1 || d->num_challenges > (uint32_t)air::MAX_ALPHAS) return set_error(ctx, CP_ERR_INVALID_ARG, "num_challenges must be 1..%d", air::MAX_ALPHAS);
  s.n = (size_t)1 << s.db; s.k0 = d->n_trace_columns; s.k1 = d->n_extended_columns; s.kt = s.k0 + s.k1; s.na = d->num_challenges;
  s.kq = (size_t)s.na << s.q;
  if (s.k0 < 1 || s.kt > 65535) return set_error(ctx, CP_ERR_INVALID_ARG, "trace width out of range");
  if (!s.k1 && (d->n_round_challenges || d->n_steps)) return set_error(ctx, CP_ERR_INVALID_ARG, "round challenges / steps without extended columns");
  const cp_air_program *c = d->constraints;
  if (!c) return set_error(ctx, CP_ERR_INVALID_ARG, "constraints program is NULL");
  if (c->P.kind != CP_AIR_CONSTRAINTS) return set_error(ctx, CP_ERR_INVALID_ARG, "constraints is not a CP_AIR_CONSTRAINTS program");
  if (c->P.n_columns != s.kt || c->P.n_public != d->n_public || c->P.n_global != d->n_global || c->P.n_challenge != d->n_round_challenges)
    return set_error(ctx, CP_ERR_INVALID_ARG, "constraints program: columns / publics / globals / challenges differ from the description");
  if (c->P.max_degree > (1u << s.q) + 1) return set_error(ctx, CP_ERR_INVALID_ARG, "constraint degree %u exceeds 2^quotient_degree_bits + 1 = %u", c->P.max_degree, (1u << s.q) + 1);
  if (prover) {
    if (d->n_steps && !d->steps) return set_error(ctx, CP_ERR_INVALID_ARG, "steps are NULL");
    for (size_t i = 0; i < d->n_steps; i++) {
      const cp_stark_step &st = d->steps[i];
      if (st.kind == CP_STARK_STEP_MAP) {
        const cp_air_program *m = st.program;
        if (!m || m->P.kind != CP_AIR_MAP) return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: not a CP_AIR_MAP program", i);
        if (m->P.n_columns != s.kt || m->P.n_out_columns != s.k1 || m->P.n_public != d->n_public || m->P.n_global != d->n_global ||
            m->P.n_challenge != d->n_round_challenges)
          return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: the map program's columns / outputs / publics / globals / challenges differ from the description", i);
        CP_TRY(map_self_read_refused(ctx, m->P, 0, (uint64_t)s.k0 * s.n * 8, s.n, (long)i));  // extended column e is input column k0 + e
      } else if (st.kind == CP_STARK_STEP_CUBIC_INVERSE) {
        if (st.first > s.k1 || (uint64_t)st.count * 3 > s.k1 - st.first) return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: columns out of range", i);
        if (st.modulus[0] >= gl::P || st.modulus[1] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: modulus is not canonical", i);
      } else if (st.kind == CP_STARK_STEP_PREFIX_SUM) {
        if (st.first > s.k1 || st.count > s.k1 - st.first) return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: columns out of range", i);
      } else return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: unknown kind %d", i, st.kind);
    }
  }
  return CP_OK;
}

void put_u64(std::vector<uint8_t> &b, uint64_t v) {
  const uint8_t *p = (const uint8_t *)&v;
  b.insert(b.end(), p, p + 8);
}
void put_words(std::vector<uint8_t> &b, const uint64_t *w, size_t n) {
  const uint8_t *p = (const uint8_t *)w;
  b.insert(b.end(), p, p + 8 * n);
}

// selector values at zeta and the folded constraint check of one challenge
struct ZetaSelectors { gl::Ext zn, zh, z_last, l_first, l_last; };
ZetaSelectors zeta_selectors(gl::Ext zeta, int db) {
  const size_t n = (size_t)1 << db;
  uint64_t g = gl::pow(7, (gl::P - 1) >> 32);
  for (int i = db; i < 32; i++) g = gl::sqr(g);
  const uint64_t g_last = gl::pow(g, n - 1), n_inv = gl::inv((uint64_t)n % gl::P);
  ZetaSelectors z;
  z.zn = host_ext_pow(zeta, n);
  z.zh = gl::ext_sub(z.zn, gl::Ext{1, 0});
  z.z_last = gl::ext_sub(zeta, gl::Ext{g_last, 0});
  z.l_first = gl::ext_mul(gl::ext_scale(z.zh, n_inv), host_ext_inv(gl::ext_sub(zeta, gl::Ext{1, 0})));
  z.l_last = gl::ext_mul(gl::ext_scale(z.zh, gl::mul(n_inv, g_last)), host_ext_inv(z.z_last));
  return z;
}

// ---- cp_stark_prove_batch: Bn instances of one description through shared launches ----
struct StarkBatchOut {
  std::vector<ByteBuf> proofs;
  std::vector<cp_challenger_state> challengers;
};

// The sequence of cp_stark_prove with the instance as the outer dimension of every array and a grid dimension of every launch. The
// transcripts up to the openings are host sponges (as in cp_stark_prove: one download per round serves all of them), the FRI part
// follows the context's transcript mode. vals: [instance][k0 + k1][n], the traces in place. Arguments are validated by the caller.
int stark_prove_batch_impl(cp_ctx *ctx, const cp_stark_desc *desc, const StarkShape &s, size_t Bn, uint64_t *vals, const uint64_t *publics,
                           const uint64_t *globals, const cp_challenger_state *ch_in, const int *use_pow, const uint64_t *pow_ov, StarkBatchOut &out) {
  const size_t n = s.n, N = n << s.rb, cap_w = (size_t)4 << s.ch, inst = s.kt * n;
  const unsigned Bu = (unsigned)Bn;
  std::vector<HostChallenger> C(Bn);
  for (size_t i = 0; i < Bn; i++) challenger_load(C[i], ch_in[i]);
  // one commitment round: the k columns of every instance -> internal arrays [instance][k][...], one iNTT, one LDE, Bn trees in one
  // Merkle call, one download of the Bn caps, which every instance's sponge then observes
  auto commit = [&](DevBatch &O, size_t k, const uint64_t *values /* first instance's columns inside vals, or null: O.coeffs is filled */) -> int {
    if (values) {
      for (size_t i = 0; i < Bn; i++) CP_TRY(cp_d2d(ctx, O.coeffs + i * O.coeffs_stride, values + i * inst, k * n * 8));
      CP_TRY(cp_ntt_dev(ctx, O.coeffs, s.db, Bn * k, n, CP_NTT_INVERSE, 0));
    }
    CP_TRY(cp_lde_dev(ctx, O.coeffs, n, s.db, s.rb, Bn * k, 7, CP_NTT_BITREV_OUT, O.lde, N));
    CP_TRY(merkle_cols_batch(ctx, O.lde, N, k, N, Bn, k * N, s.ch, O.digests, O.cap));
    CP_TRY(batch_fetch_caps(ctx, O, Bn, s.ch));
    for (uint64_t v : O.cap_host)
      if (v >= gl::P) return set_error(ctx, CP_ERR_INTERNAL, "non-canonical cap element");
    for (size_t i = 0; i < Bn; i++) C[i].observe(O.cap_host.data() + i * cap_w, cap_w);
    return CP_OK;
  };
  host_phase(ctx, "stark_trace");
  DevBatch t0, t1, qb;
  CP_TRY(batch_alloc(ctx, t0, Bn, s.k0, n, N, s.ch));
  CP_TRY(commit(t0, s.k0, vals));
  if (canonical_check_failed(ctx)) return CP_ERR_INVALID_ARG;  // the caller names the instance
  std::vector<uint64_t> rch(Bn * desc->n_round_challenges);
  if (s.k1) {
    host_phase(ctx, "stark_extended");
    for (size_t i = 0; i < rch.size(); i++) rch[i] = C[i / desc->n_round_challenges].challenge();
    uint64_t *ext = vals + s.k0 * n;
    for (size_t i = 0; i < desc->n_steps; i++) {
      const cp_stark_step &st = desc->steps[i];
      if (st.kind == CP_STARK_STEP_MAP) {
        cp_air_program *prog = const_cast<cp_air_program *>(st.program);
        if (prog->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: the program belongs to another device", i);
        std::vector<uint64_t> uni;
        CP_TRY(air_uniform_tables(ctx, prog->P, Bn, publics, globals, rch.data(), uni));
        CP_TRY(air_map_launch(ctx, prog, Bn, vals, ext, inst, n, uni));
      } else if (st.kind == CP_STARK_STEP_CUBIC_INVERSE) {
        const size_t groups = ((size_t)st.count + ext3::GROUP - 1) / ext3::GROUP;
        if (groups > 65535 || n > ((size_t)1 << 32)) return set_error(ctx, CP_ERR_INVALID_ARG, "step %zu: too many elements per call", i);
        if (st.count)
          LAUNCH(ctx, "cubic_batch_inverse", ext3::k_batch_inverse, dim3(blocks_for(n, 256), (unsigned)groups, Bu), dim3(256), ext + (size_t)st.first * n,
                 (size_t)st.count, n, st.modulus[0], st.modulus[1], inst);
      } else if (st.count) {
        LAUNCH(ctx, "column_prefix_sum", ext3::k_prefix_sum, dim3(st.count, Bu), dim3(256), ext + (size_t)st.first * n, n, (int)(st.flags & 1), inst);
      }
    }
    CP_TRY(batch_alloc(ctx, t1, Bn, s.k1, n, N, s.ch));
    CP_TRY(commit(t1, s.k1, ext));
  }
  host_phase(ctx, "stark_quotient");
  std::vector<uint64_t> alphas(Bn * s.na);
  for (size_t i = 0; i < alphas.size(); i++) alphas[i] = C[i / s.na].challenge();
  {
    cp_air_program *prog = const_cast<cp_air_program *>(desc->constraints);  // the cache of compiled forms is behind its mutex
    if (prog->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the constraints program belongs to another device");
    std::vector<uint64_t> uni;
    CP_TRY(air_uniform_tables(ctx, prog->P, Bn, publics, globals, rch.data(), uni));
    std::vector<const uint64_t *> cols;
    for (size_t i = 0; i < Bn; i++) {
      for (size_t j = 0; j < s.k0; j++) cols.push_back(t0.lde + i * t0.lde_stride + j * N);
      for (size_t j = 0; j < s.k1; j++) cols.push_back(t1.lde + i * t1.lde_stride + j * N);
    }
    CP_TRY(batch_alloc(ctx, qb, Bn, s.kq, n, N, s.ch));
    CP_TRY(air_quotient_coeffs(ctx, prog, Bn, cols, s.db, s.q, uni, alphas.data(), s.na, qb.coeffs));
    CP_TRY(commit(qb, s.kq, nullptr));
  }
  host_phase(ctx, "stark_openings");
  // zeta and g zeta of every instance, then their inverses: [2 Bn points | 2 Bn inverses], the order fri_prove_impl reads them in
  uint64_t g = gl::pow(7, (gl::P - 1) >> 32);
  for (int i = s.db; i < 32; i++) g = gl::sqr(g);
  std::vector<gl::Ext> pts(4 * Bn);
  for (size_t i = 0; i < Bn; i++) {
    const uint64_t za = C[i].challenge(), zb = C[i].challenge();
    const gl::Ext z{za, zb}, zn = host_ext_pow(z, n);
    if (zn.a == 1 && zn.b == 0)
      return set_error(ctx, CP_ERR_INTERNAL, "instance %zu: zeta fell into the trace domain (probability 2^-%d): retry with another transcript", i, 128 - s.db);
    // what cp_fri_prove refuses of an opening point: zero, or a point of the LDE coset (z^n != 1 leaves only these)
    if ((z.a == 0 && z.b == 0) || (z.b == 0 && gl::pow(gl::mul(z.a, gl::inv(7)), (uint64_t)N) == 1))
      return set_error(ctx, CP_ERR_INVALID_ARG, "instance %zu: the opening point is zero or lies on the LDE coset", i);
    pts[2 * i] = z;
    pts[2 * i + 1] = gl::Ext{gl::mul(z.a, g), gl::mul(z.b, g)};
    pts[2 * Bn + 2 * i] = host_ext_inv(pts[2 * i]);
    pts[2 * Bn + 2 * i + 1] = host_ext_inv(pts[2 * i + 1]);
  }
  // per instance [trace, extended, quotient at zeta | trace, extended at g zeta]: the order the transcript observes and the proof lists
  const size_t open_stride = 2 * s.kt + s.kq;
  gl::Ext *d_pts, *zpow, *d_open;
  unsigned *d_flags;
  CP_TRY(arena_alloc(ctx, pts.size() * 16, (void **)&d_pts));
  CP_TRY(arena_alloc(ctx, pts.size() * n * 16, (void **)&zpow));
  CP_TRY(arena_alloc(ctx, Bn * open_stride * 16, (void **)&d_open));
  CP_TRY(arena_alloc(ctx, Bn * sizeof(unsigned), (void **)&d_flags));
  CP_TRY(push(ctx, d_pts, pts.data(), pts.size() * 16));
  HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, Bn * sizeof(unsigned), ctx->stream));
  LAUNCH(ctx, "fri_ext_powers", fri::k_ext_powers, dim3(blocks_for(n, 256), 4 * Bu), dim3(256), d_pts, n, zpow);
  auto open_at = [&](const DevBatch &O, const gl::Ext *zp, size_t at) -> int {
    if (!O.k) return CP_OK;
    LAUNCH(ctx, "eval_at_point", fri::k_eval_at_point, dim3((unsigned)O.k, Bu), dim3(256), O.coeffs, O.coeffs_stride, (const uint64_t *const *)nullptr, n, zp,
           2 * n, d_open, open_stride, at);
    return CP_OK;
  };
  CP_TRY(open_at(t0, zpow, 0));
  CP_TRY(open_at(t1, zpow, s.k0));
  CP_TRY(open_at(qb, zpow, s.kt));
  CP_TRY(open_at(t0, zpow + n, s.kt + s.kq));
  CP_TRY(open_at(t1, zpow + n, s.kt + s.kq + s.k0));
  std::vector<uint64_t> open(Bn * open_stride * 2);
  CP_TRY(fetch(ctx, open.data(), d_open, open.size() * 8));
  for (size_t i = 0; i < Bn; i++) C[i].observe(open.data() + i * open_stride * 2, open_stride * 2);
  // ---- prove_openings: the zeta batch over every oracle, the g zeta batch over the trace rounds ----
  std::vector<OracleRef> oracles;
  for (const DevBatch *O : {&t0, &t1, &qb}) {
    if (!O->k) continue;
    OracleRef R;
    R.k = O->k;
    R.coeffs = O->coeffs; R.lde = O->lde; R.digests = O->digests;
    R.coeffs_stride = O->coeffs_stride; R.lde_stride = O->lde_stride; R.dig_stride = O->dig_stride;
    oracles.push_back(R);
  }
  std::vector<FriBatchDesc> fb(2);
  for (uint32_t o = 0; o < oracles.size(); o++) {
    fb[0].ranges.push_back({o, 0, (uint32_t)oracles[o].k});
    fb[0].n_polys += oracles[o].k;
    if (o + 1 < oracles.size()) {
      fb[1].ranges.push_back({o, 0, (uint32_t)oracles[o].k});
      fb[1].n_polys += oracles[o].k;
    }
  }
  FriCfg cfg;
  CP_TRY(load_fri_cfg(ctx, &desc->fri, cfg));
  Transcript T;
  CP_TRY(T.init_from(ctx, C.data(), Bn));
  FriHostOut fo;
  CP_TRY(fri_prove_impl(ctx, Bn, s.db, cfg, oracles, fb, zpow, zpow + 2 * Bn * n, T, tr::Seg{nullptr, nullptr, 0, 0}, use_pow, pow_ov, d_flags, fo));
  std::vector<tr::DevCh> hch(Bn);
  if (T.device) CP_TRY(fetch_async(ctx, hch.data(), T.d_ch, Bn * sizeof(tr::DevCh)));
  host_phase(ctx, "drain");
  CP_TRY(fetch_flush(ctx));
  CP_TRY(fo.check(ctx));
  host_phase(ctx, "copy_out");
  out.proofs.assign(Bn, ByteBuf());
  out.challengers.assign(Bn, cp_challenger_state());
  const size_t n_tr = s.k1 ? 2 : 1;
  for (size_t i = 0; i < Bn; i++) {
    ByteBuf &b = out.proofs[i];
    const uint64_t *o = open.data() + i * open_stride * 2;
    b.u64(n_tr);
    b.u64((uint64_t)1 << s.ch); b.felts(t0.cap_host.data() + i * cap_w, cap_w);
    if (s.k1) { b.u64((uint64_t)1 << s.ch); b.felts(t1.cap_host.data() + i * cap_w, cap_w); }
    b.u64((uint64_t)1 << s.ch); b.felts(qb.cap_host.data() + i * cap_w, cap_w);
    b.u64(s.kt); b.felts(o, 2 * s.kt);
    b.u64(s.kt); b.felts(o + 2 * (s.kt + s.kq), 2 * s.kt);
    b.u64(s.kq); b.felts(o + 2 * s.kt, 2 * s.kq);
    fo.bytes(i, b);
    if (!T.device) hch[i] = Transcript::pack(T.C[i]);
    cp_challenger_state &c = out.challengers[i];
    memset(&c, 0, sizeof c);
    memcpy(c.sponge_state, hch[i].state, sizeof hch[i].state);
    memcpy(c.input_buffer, hch[i].in, (size_t)hch[i].n_in * 8);
    memcpy(c.output_buffer, hch[i].state, (size_t)hch[i].n_out * 8);
    c.n_input = (uint32_t)hch[i].n_in;
    c.n_output = (uint32_t)hch[i].n_out;
  }
  host_phase(ctx, nullptr);
  return CP_OK;
}

// ---- the verifier's two halves: everything before `verify_fri_proof` (cp_stark_verify, and per proof cp_stark_verify_batch) ----
struct StarkFront {
  std::vector<uint64_t> caps[3], lq, nxt;  // the caps; the openings as the transcript takes them: local | quotient, next
  gl::Ext zeta;
  cp_challenger_state ch;  // after the openings
  size_t o = 0;            // where the FriProof starts
  int status = 0, detail = -1;  // the class of a refusal in cp_verify_verdict's terms
};
// Parse of everything before the FriProof, transcript, round challenges, alphas, zeta, the constraints at zeta against the
// quotient, the openings into the transcript. desc, publics, globals and `in` are validated by the caller. Errors go to the
// thread's own message, with cp_stark_verify's words.
int stark_verify_front(const cp_stark_desc *desc, const StarkShape &s, const uint64_t *publics, const uint64_t *globals, const cp_challenger_state &in,
                       const uint8_t *proof, size_t proof_len, StarkFront &f) {
  const size_t n_tr = s.k1 ? 2 : 1, cap_w = (size_t)4 << s.ch;
  // ---- parse ----
  size_t o = 0;
  bool bad = false, noncanonical = false;
  auto u64 = [&]() -> uint64_t {
    if (proof_len - o < 8) { bad = true; return 0; }
    uint64_t v;
    memcpy(&v, proof + o, 8);
    o += 8;
    return v;
  };
  auto words = [&](size_t cnt, std::vector<uint64_t> &out) {
    if (bad || cnt > (proof_len - o) / 8) { bad = true; return; }
    out.resize(cnt);
    memcpy(out.data(), proof + o, cnt * 8);
    o += cnt * 8;
    if (!all_canonical(out.data(), cnt)) noncanonical = true;
  };
  std::vector<uint64_t> loc, qz;
  std::vector<uint64_t> *caps = f.caps, &nxt = f.nxt;
  if (u64() != n_tr) bad = true;
  for (size_t i = 0; i < n_tr + 1 && !bad; i++) {
    if (u64() != ((uint64_t)1 << s.ch)) bad = true;
    words(cap_w, caps[i]);
  }
  if (!bad && u64() != s.kt) bad = true;
  words(2 * s.kt, loc);
  if (!bad && u64() != s.kt) bad = true;
  words(2 * s.kt, nxt);
  if (!bad && u64() != s.kq) bad = true;
  words(2 * s.kq, qz);
  f.status = 1;
  if (bad) return set_error(nullptr, CP_ERR_VERIFY, "malformed STARK proof");
  f.status = 2;
  if (noncanonical) return set_error(nullptr, CP_ERR_VERIFY, "a field element of the proof is not canonical (>= p)");
  hostu::alloc_checkpoint();
  // ---- transcript ----
  cp_challenger_state &ch = f.ch;
  ch = in;
  CP_TRY(cp_challenger_observe(&ch, caps[0].data(), cap_w));
  std::vector<uint64_t> rch(2 * (size_t)desc->n_round_challenges, 0);
  if (s.k1) {
    for (uint32_t i = 0; i < desc->n_round_challenges; i++) CP_TRY(cp_challenger_challenges(&ch, &rch[2 * i], 1));
    CP_TRY(cp_challenger_observe(&ch, caps[1].data(), cap_w));
  }
  uint64_t alphas[air::MAX_ALPHAS];
  CP_TRY(cp_challenger_challenges(&ch, alphas, s.na));
  CP_TRY(cp_challenger_observe(&ch, caps[n_tr].data(), cap_w));
  uint64_t zw[2];
  CP_TRY(cp_challenger_challenges(&ch, zw, 2));
  const gl::Ext zeta{zw[0], zw[1]};
  f.zeta = zeta;
  // ---- the constraints at zeta against Z_H(zeta) * sum_i zeta^(n i) t_i(zeta) ----
  const air::Program &P = desc->constraints->P;
  std::vector<gl::Ext> pe(desc->n_public), ge(desc->n_global), vals;
  for (uint32_t i = 0; i < desc->n_public; i++) pe[i] = gl::Ext{publics[i], 0};
  for (uint32_t i = 0; i < desc->n_global; i++) ge[i] = gl::Ext{globals[i], 0};
  air_eval_ext_row(P, (const gl::Ext *)loc.data(), (const gl::Ext *)nxt.data(), pe.data(), ge.data(), (const gl::Ext *)rch.data(), vals);
  const ZetaSelectors zs = zeta_selectors(zeta, s.db);
  f.status = 4;
  if (zs.zh.a == 0 && zs.zh.b == 0) return set_error(nullptr, CP_ERR_VERIFY, "zeta lies in the trace domain");
  f.status = 5;
  for (uint32_t a = 0; a < s.na; a++) {
    gl::Ext acc{0, 0};
    for (uint32_t r : P.roots) {
      gl::Ext v = vals[P.ops[r].a];
      if (P.ops[r].op == air::R_ASSERT_TRANSITION) v = gl::ext_mul(v, zs.z_last);
      else if (P.ops[r].op == air::R_ASSERT_FIRST) v = gl::ext_mul(v, zs.l_first);
      else if (P.ops[r].op == air::R_ASSERT_LAST) v = gl::ext_mul(v, zs.l_last);
      acc = gl::ext_add(gl::ext_scale(acc, alphas[a]), v);
    }
    gl::Ext t{0, 0};
    for (size_t k = (size_t)1 << s.q; k-- > 0;) t = gl::ext_add(gl::ext_mul(t, zs.zn), gl::Ext{qz[2 * (((size_t)a << s.q) + k)], qz[2 * (((size_t)a << s.q) + k) + 1]});
    const gl::Ext lhs = gl::ext_mul(t, zs.zh);
    f.detail = (int)a;
    if (lhs.a != acc.a || lhs.b != acc.b) return set_error(nullptr, CP_ERR_VERIFY, "the constraints do not vanish: quotient identity fails at zeta for challenge %u", a);
  }
  f.status = 0;
  f.detail = -1;
  // ---- the openings into the transcript ----
  f.lq = loc;
  f.lq.insert(f.lq.end(), qz.begin(), qz.end());
  CP_TRY(cp_challenger_observe(&ch, f.lq.data(), f.lq.size()));
  CP_TRY(cp_challenger_observe(&ch, nxt.data(), nxt.size()));
  f.o = o;
  return CP_OK;
}

// The FRI instance of a STARK proof in cp_fri_verify's terms: 2 or 3 oracles (trace, [extended,] quotient), everything at zeta,
// the trace rounds at g zeta. Points, caps and opened values are the front's; without one the table alone (points 0).
struct StarkFriInstance {
  size_t n_or;
  cp_fri_oracle_info infos[3];
  const uint64_t *cap_ptrs[3] = {nullptr, nullptr, nullptr};
  cp_fri_poly_range r0[3], r1[2];
  cp_fri_batch fb[2];
  const uint64_t *opened[2] = {nullptr, nullptr};
  StarkFriInstance(const StarkFriInstance &) = delete;  // fb points into r0 / r1
  StarkFriInstance(const StarkShape &s, const StarkFront *f) {
    const gl::Ext zeta = f ? f->zeta : gl::Ext{0, 0};
    if (f) {
      for (int i = 0; i < 3; i++) cap_ptrs[i] = f->caps[i].data();
      opened[0] = f->lq.data();
      opened[1] = f->nxt.data();
    }
    uint64_t g = gl::pow(7, (gl::P - 1) >> 32);
    for (int i = s.db; i < 32; i++) g = gl::sqr(g);
    const size_t n_tr = s.k1 ? 2 : 1;
    n_or = n_tr + 1;
    const uint32_t qi = (uint32_t)n_tr;
    infos[0] = {(uint32_t)s.k0, 0}; infos[1] = {(uint32_t)(s.k1 ? s.k1 : s.kq), 0}; infos[2] = {(uint32_t)s.kq, 0};
    r0[0] = {0, 0, (uint32_t)s.k0}; r0[1] = {1, 0, (uint32_t)s.k1}; r0[2] = {qi, 0, (uint32_t)s.kq};
    r1[0] = {0, 0, (uint32_t)s.k0}; r1[1] = {1, 0, (uint32_t)s.k1};
    if (!s.k1) r0[1] = r0[2];
    fb[0] = {{zeta.a, zeta.b}, r0, s.k1 ? (size_t)3 : (size_t)2};
    fb[1] = {{gl::mul(zeta.a, g), gl::mul(zeta.b, g)}, r1, s.k1 ? (size_t)2 : (size_t)1};
  }
};

// the same instance as verify.inc's structures (what cp_fri_verify builds from its arguments); f == nullptr: no caps, points, values
void stark_fri_instance(const cp_stark_desc *desc, const StarkShape &s, const StarkFront *f, FriVerifyInstance &I) {
  const StarkFriInstance fi(s, f);
  load_fri_cfg(nullptr, &desc->fri, I.cfg);  // stark_shape accepted it
  I.db = s.db;
  I.n_oracles = (int)fi.n_or;
  for (size_t o = 0; o < fi.n_or; o++) {
    I.kk[o] = I.leaf_len[o] = fi.infos[o].num_polys;
    I.caps[o] = fi.cap_ptrs[o];
  }
  I.points.resize(2);
  I.ranges.assign(2, {});
  I.opened.assign(2, {});
  for (size_t b = 0; b < 2; b++) {
    I.points[b] = gl::Ext{fi.fb[b].point[0], fi.fb[b].point[1]};
    size_t cnt = 0;
    for (size_t r = 0; r < fi.fb[b].n_ranges; r++) {
      I.ranges[b].push_back(fi.fb[b].ranges[r]);
      cnt += fi.fb[b].ranges[r].count;
    }
    if (!f) continue;
    I.opened[b].resize(cnt);
    for (size_t j = 0; j < cnt; j++) I.opened[b][j] = gl::Ext{fi.opened[b][2 * j], fi.opened[b][2 * j + 1]};
  }
}

// The STARK proof format as the kernels of fri_verify.h read it: trace_caps | quotient_cap | local | next | quotient openings |
// FriProof, every oracle's cap in the proof itself. Refuses what the instance table cannot hold.
int stark_layout(cp_ctx *ctx, const cp_stark_desc *desc, const StarkShape &s, FriVerifyInstance &I, friv::Instance &D, size_t &proof_words) {
  if (desc->fri.num_query_rounds > 255) return set_error(ctx, CP_ERR_INVALID_ARG, "more than 255 query rounds");  // the failure key: query << 8 | ordinal
  if (s.kq < 1 || s.kq > 65535) return set_error(ctx, CP_ERR_INVALID_ARG, "quotient width out of range");
  stark_fri_instance(desc, s, nullptr, I);
  if (I.n_oracles > friv::MAX_ORACLES || I.cfg.n_arity > friv::MAX_LAYERS) return set_error(ctx, CP_ERR_INVALID_ARG, "too many oracles / FRI layers");
  memset(&D, 0, sizeof D);
  const size_t cap_n = (size_t)1 << s.ch;
  size_t o = 1;
  for (int b = 0; b < I.n_oracles; b++) { o += 1; D.cap_src[b] = 1; D.cap_off[b] = (uint32_t)o; o += cap_n * 4; }
  o += 3 + 4 * s.kt + 2 * s.kq;
  proof_words = friv_layout(I, o, D);
  D.n_batches = 2;
  uint32_t nr = 0;
  for (size_t b = 0; b < 2; b++) {
    D.batch_first[b] = nr;
    for (const cp_fri_poly_range &R : I.ranges[b]) {
      if (nr >= (uint32_t)friv::MAX_RANGES) return set_error(ctx, CP_ERR_INVALID_ARG, "too many opening ranges");
      D.r_oracle[nr] = R.oracle; D.r_first[nr] = R.first; D.r_count[nr] = R.count;
      nr++;
    }
  }
  D.batch_first[2] = nr;
  D.n_ranges = nr;
  if (proof_words > ((size_t)1 << 31)) return set_error(ctx, CP_ERR_INVALID_ARG, "description out of range: a proof of more than 2^31 words");
  return CP_OK;
}

// Everything cp_stark_verify does before its query phase, for one proof of a batch, on whatever thread: the front above, then what
// cp_fri_verify does before verify_fri_queries (shape-directed parse of the FriProof, FRI challenges, proof of work) - the same
// functions in the same order. Status 0: `rec` holds the challenge record, ch_out the challenger as cp_stark_verify leaves it.
cp_verify_verdict stark_verify_host_phase(const cp_stark_desc *desc, const StarkShape &s, const uint64_t *publics,
                                          const uint64_t *globals, const cp_challenger_state &ch_in, const uint8_t *proof, size_t len,
                                          cp_challenger_state &ch_out, uint64_t *rec) {
  StarkFront f;
  if (stark_verify_front(desc, s, publics, globals, ch_in, proof, len, f) != CP_OK) return verdict(f.status, -1, f.detail);
  FriVerifyInstance I;
  stark_fri_instance(desc, s, &f, I);
  Rd r{proof + f.o, len - f.o};
  ParsedFri pf;
  if (parse_fri_proof(nullptr, I, r, pf) != CP_OK || r.o != len - f.o) return verdict(1);
  if (r.noncanonical) return verdict(2);
  HostChallenger C;
  challenger_load(C, f.ch);
  gl::Ext alpha;
  std::vector<gl::Ext> fbetas;
  std::vector<uint64_t> x_indices;
  if (fri_challenges(nullptr, C, I, pf, alpha, fbetas, x_indices) != CP_OK) return verdict(6);
  fill_record(I, alpha, fbetas.data(), x_indices.data(), rec);
  challenger_store(C, ch_out);
  return verdict(0);
}

}  // namespace

extern "C" {

cp_air_program *cp_air_program_create(cp_ctx *ctx, const cp_air_program_desc *desc) try {
  if (!ctx || !desc) { set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  if ((desc->n_ops && !desc->ops) || (desc->n_consts && !desc->consts)) { set_error(ctx, CP_ERR_INVALID_ARG, "NULL ops / consts"); return nullptr; }
  if (desc->n_ops > ((size_t)1 << 24) || desc->n_consts >= air::MAX_INDEX) { set_error(ctx, CP_ERR_INVALID_ARG, "program too large (2^24 ops, 2^20 constants)"); return nullptr; }
  std::unique_ptr<cp_air_program> p(new cp_air_program());
  p->ctx = ctx;
  p->device = ctx->device;
  p->P.kind = desc->kind;
  p->P.ops.resize(desc->n_ops);
  static_assert(sizeof(air::RawOp) == sizeof(cp_air_op), "op layout");
  if (desc->n_ops) memcpy(p->P.ops.data(), desc->ops, desc->n_ops * sizeof(cp_air_op));
  p->P.consts.assign(desc->consts, desc->consts + desc->n_consts);
  p->P.n_columns = desc->n_columns; p->P.n_public = desc->n_public; p->P.n_global = desc->n_global; p->P.n_challenge = desc->n_challenge;
  p->P.n_out_columns = desc->n_out_columns;
  const std::string why = air::analyse(p->P);
  if (!why.empty()) { set_error(ctx, CP_ERR_INVALID_ARG, "AIR program: %s", why.c_str()); return nullptr; }
  p->single = air::compile(p->P, 1, air_prefetch());
  if (p->single.n_slots >= air::DST_NONE) { set_error(ctx, CP_ERR_UNSUPPORTED, "the program needs %u live temporaries (limit %u)", p->single.n_slots, air::DST_NONE - 1); return nullptr; }
  return p.release();
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

void cp_air_program_destroy(cp_air_program *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  delete p;
}

int cp_air_program_get_info(const cp_air_program *p, cp_air_program_info *out) try {
  if (!p || !out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  out->n_ops = p->P.ops.size();
  out->n_live_ops = p->P.n_live;
  out->n_constraints = p->P.kind == CP_AIR_CONSTRAINTS ? p->P.roots.size() : 0;
  out->max_constraint_degree = p->P.max_degree;
  out->n_segments_max = (uint32_t)std::min<size_t>(p->P.roots.size() ? p->P.roots.size() : 1, 1024);
  out->n_slots = p->single.n_slots;
  out->n_instructions = p->single.code.size();
  return CP_OK;
} CP_CATCH(nullptr)

int cp_air_program_eval_ext(const cp_air_program *p, const uint64_t *local, const uint64_t *next, const uint64_t *publics, const uint64_t *globals,
                            const uint64_t *challenges, uint64_t *out, uint32_t *sink_kinds_out) try {
  if (!p || !out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  const air::Program &P = p->P;
  if (P.kind != CP_AIR_CONSTRAINTS) return set_error(nullptr, CP_ERR_INVALID_ARG, "not a CP_AIR_CONSTRAINTS program");
  if ((P.n_columns && (!local || !next)) || (P.n_public && !publics) || (P.n_global && !globals) || (P.n_challenge && !challenges))
    return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  if (!all_canonical(local, 2 * (size_t)P.n_columns) || !all_canonical(next, 2 * (size_t)P.n_columns) || !all_canonical(publics, 2 * (size_t)P.n_public) ||
      !all_canonical(globals, 2 * (size_t)P.n_global) || !all_canonical(challenges, 2 * (size_t)P.n_challenge))
    return set_error(nullptr, CP_ERR_INVALID_ARG, "an input element is not canonical");
  std::vector<gl::Ext> vals;
  air_eval_ext_row(P, (const gl::Ext *)local, (const gl::Ext *)next, (const gl::Ext *)publics, (const gl::Ext *)globals, (const gl::Ext *)challenges, vals);
  size_t k = 0;
  for (uint32_t r : P.roots) {
    out[2 * k] = vals[P.ops[r].a].a;
    out[2 * k + 1] = vals[P.ops[r].a].b;
    if (sink_kinds_out) sink_kinds_out[k] = P.ops[r].op;
    k++;
  }
  return CP_OK;
} CP_CATCH(nullptr)

int cp_air_quotient_commit(cp_ctx *ctx, const cp_air_program *program, cp_poly_batch *const *oracles, size_t n_oracles, int q,
                           const uint64_t *publics, const uint64_t *globals, const uint64_t *challenges, const uint64_t *alphas, size_t n_alphas,
                           cp_poly_batch **quotient_out) try {
  CHECK_CTX(ctx);
  if (!program || !oracles || !alphas || !quotient_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  *quotient_out = nullptr;
  cp_air_program *prog = const_cast<cp_air_program *>(program);  // the cache of compiled forms is behind its mutex
  const air::Program &P = prog->P;
  if (P.kind != CP_AIR_CONSTRAINTS) return set_error(ctx, CP_ERR_INVALID_ARG, "not a CP_AIR_CONSTRAINTS program");
  if (prog->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the program belongs to another device");
  if (n_oracles < 1 || n_oracles > 64) return set_error(ctx, CP_ERR_INVALID_ARG, "1..64 trace oracles");
  if (n_alphas < 1 || n_alphas > (size_t)air::MAX_ALPHAS) return set_error(ctx, CP_ERR_INVALID_ARG, "1..%d alphas", air::MAX_ALPHAS);
  if (!all_canonical(alphas, n_alphas)) return set_error(ctx, CP_ERR_INVALID_ARG, "an alpha is not canonical");
  size_t width = 0;
  int db = 0, rb = 0, ch = 0;
  for (size_t o = 0; o < n_oracles; o++) {
    const cp_poly_batch *b = oracles[o];
    if (!b) return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu is NULL", o);
    if (!b->ctx) return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu: the context of this batch was destroyed", o);
    if (!(b->ctx == ctx || (ctx->parent && b->ctx == ctx->parent))) return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu belongs to another context", o);
    if (o == 0) { db = b->degree_bits; rb = b->rate_bits; ch = b->cap_height; }
    else if (b->degree_bits != db || b->rate_bits != rb || b->cap_height != ch) return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu: degree / rate / cap height differ from oracle 0", o);
    width += b->k;
  }
  if (width != P.n_columns) return set_error(ctx, CP_ERR_INVALID_ARG, "the oracles have %zu columns, the program reads rows of %u", width, P.n_columns);
  if (q < 0 || q > rb) return set_error(ctx, CP_ERR_INVALID_ARG, "quotient_degree_bits %d out of range [0, rate_bits %d]", q, rb);
  if (P.max_degree > (1u << q) + 1) return set_error(ctx, CP_ERR_INVALID_ARG, "constraint degree %u exceeds 2^quotient_degree_bits + 1 = %u", P.max_degree, (1u << q) + 1);
  std::vector<uint64_t> uni;
  CP_TRY(air_uniform_table(ctx, P, publics, globals, challenges, uni));
  const size_t n = (size_t)1 << db, N = n << rb;
  std::vector<const uint64_t *> cols;
  for (size_t o = 0; o < n_oracles; o++)
    for (size_t j = 0; j < oracles[o]->k; j++) cols.push_back(oracles[o]->lde + j * N);
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);
  host_phase(ctx, "air_quotient");
  uint64_t *d_q;
  CP_TRY(arena_alloc(ctx, (n_alphas << q) * n * 8, (void **)&d_q));
  CP_TRY(air_quotient_coeffs(ctx, prog, 1, cols, db, q, uni, alphas, (uint32_t)n_alphas, d_q));
  host_phase(ctx, nullptr);
  return poly_batch_commit(ctx, d_q, true, n_alphas << q, db, rb, ch, CP_BATCH_FROM_COEFFS, nullptr, quotient_out);
} CP_CATCH(ctx)

int cp_air_map_dev(cp_ctx *ctx, const cp_air_program *program, const uint64_t *in_cols_dev, uint64_t *out_cols_dev, size_t n, const uint64_t *publics,
                   const uint64_t *globals, const uint64_t *challenges) try {
  CHECK_CTX(ctx);
  if (!program) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  cp_air_program *prog = const_cast<cp_air_program *>(program);
  const air::Program &P = prog->P;
  if (P.kind != CP_AIR_MAP) return set_error(ctx, CP_ERR_INVALID_ARG, "not a CP_AIR_MAP program");
  if (prog->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the program belongs to another device");
  if (n == 0) return CP_OK;
  if ((P.n_columns && !in_cols_dev) || (P.n_out_columns && !out_cols_dev)) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL column arrays");
  CP_TRY(map_self_read_refused(ctx, P, (uint64_t)(uintptr_t)in_cols_dev, (uint64_t)(uintptr_t)out_cols_dev, n, -1));
  std::vector<uint64_t> uni;
  CP_TRY(air_uniform_table(ctx, P, publics, globals, challenges, uni));
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);
  CP_TRY(air_map_launch(ctx, prog, 1, in_cols_dev, out_cols_dev, 0, n, uni));
  HIP_TRY(ctx, sync_stream(ctx));
  return CP_OK;
} CP_CATCH(ctx)

int cp_cubic_batch_inverse_dev(cp_ctx *ctx, const uint64_t modulus[2], uint64_t *cols_dev, size_t count, size_t n) try {
  CHECK_CTX(ctx);
  if (count == 0 || n == 0) return CP_OK;
  if (!modulus || !cols_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (modulus[0] >= gl::P || modulus[1] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "modulus is not canonical");
  const size_t groups = (count + ext3::GROUP - 1) / ext3::GROUP;
  if (groups > 65535 || n > ((size_t)1 << 32)) return set_error(ctx, CP_ERR_INVALID_ARG, "too many elements per call");
  LAUNCH(ctx, "cubic_batch_inverse", ext3::k_batch_inverse, dim3(blocks_for(n, 256), (unsigned)groups), dim3(256), cols_dev, count, n, modulus[0], modulus[1], (size_t)0);
  HIP_TRY(ctx, sync_stream(ctx));
  return CP_OK;
} CP_CATCH(ctx)

int cp_column_prefix_sum_dev(cp_ctx *ctx, uint64_t *cols_dev, size_t k, size_t n, int exclusive) try {
  CHECK_CTX(ctx);
  if (k == 0 || n == 0) return CP_OK;
  if (!cols_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (k > 0x7FFFFFFFull) return set_error(ctx, CP_ERR_INVALID_ARG, "too many columns per call");
  LAUNCH(ctx, "column_prefix_sum", ext3::k_prefix_sum, dim3((unsigned)k), dim3(256), cols_dev, n, exclusive ? 1 : 0, (size_t)0);
  HIP_TRY(ctx, sync_stream(ctx));
  return CP_OK;
} CP_CATCH(ctx)

int cp_stark_prove(cp_ctx *ctx, const cp_stark_desc *desc, const uint64_t *trace_values, int trace_on_device, const uint64_t *publics,
                   const uint64_t *globals, cp_challenger_state *challenger, int use_pow_override, uint64_t pow_override, uint8_t **proof_out,
                   size_t *proof_len) try {
  CHECK_CTX(ctx);
  if (!trace_values || !challenger || !proof_out || !proof_len) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  *proof_out = nullptr;
  *proof_len = 0;
  StarkShape s;
  CP_TRY(stark_shape(ctx, desc, true, s));
  if ((desc->n_public && !publics) || (desc->n_global && !globals)) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL publics / globals");
  if (!all_canonical(publics, desc->n_public) || !all_canonical(globals, desc->n_global)) return set_error(ctx, CP_ERR_INVALID_ARG, "a public input / global value is not canonical");
  if (const char *why = challenger_problem(challenger)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s", why);
  cp_challenger_state ch = *challenger;  // a refused call leaves the caller's transcript alone
  const size_t cap_w = (size_t)4 << s.ch;
  // every handle and buffer of the call, released on every exit path
  struct Owned {
    DevBuf vals_buf;  // from the pool; goes back as reusable only once the stream is known to be idle (after the handles below)
    cp_poly_batch *t0 = nullptr, *t1 = nullptr, *qb = nullptr;
    uint64_t *vals = nullptr;
    uint8_t *fri = nullptr;
    ~Owned() {
      cp_batch_destroy(t0);
      cp_batch_destroy(t1);
      cp_batch_destroy(qb);
      free(fri);
    }
  } own{ctx->buf(DevOwn::POOLED)};
  // the value columns of both trace rounds in one array: a row of a map step = execution trace, then the extended columns
  CP_TRY(alloc_status(ctx, own.vals_buf.alloc(s.kt * s.n * 8), s.kt * s.n * 8));
  own.vals = own.vals_buf.get<uint64_t>();
  if (trace_on_device) CP_TRY(cp_d2d(ctx, own.vals, trace_values, s.k0 * s.n * 8));
  else {
    CP_TRY(cp_h2d(ctx, own.vals, trace_values, s.k0 * s.n * 8));
    CP_TRY(canonical_check_enqueue(ctx, own.vals, s.k0 * s.n, true));  // a host trace is scanned on the device, behind the upload
  }
  CP_TRY(poly_batch_commit(ctx, own.vals, true, s.k0, s.db, s.rb, s.ch, 0, nullptr, &own.t0));  // ends in a synchronising cap download
  if (!trace_on_device && canonical_check_failed(ctx)) return set_error(ctx, CP_ERR_INVALID_ARG, "a trace value is not canonical");
  CP_TRY(cp_challenger_observe(&ch, own.t0->cap_host.data(), cap_w));
  std::vector<uint64_t> rch(desc->n_round_challenges);
  if (s.k1) {
    CP_TRY(cp_challenger_challenges(&ch, rch.data(), rch.size()));
    uint64_t *ext = own.vals + s.k0 * s.n;
    HIP_TRY(ctx, hipMemsetAsync(ext, 0, s.k1 * s.n * 8, ctx->stream));
    for (size_t i = 0; i < desc->n_steps; i++) {
      const cp_stark_step &st = desc->steps[i];
      if (st.kind == CP_STARK_STEP_MAP) CP_TRY(cp_air_map_dev(ctx, st.program, own.vals, ext, s.n, publics, globals, rch.data()));
      else if (st.kind == CP_STARK_STEP_CUBIC_INVERSE) CP_TRY(cp_cubic_batch_inverse_dev(ctx, st.modulus, ext + (size_t)st.first * s.n, st.count, s.n));
      else CP_TRY(cp_column_prefix_sum_dev(ctx, ext + (size_t)st.first * s.n, st.count, s.n, (int)(st.flags & 1)));
    }
    CP_TRY(poly_batch_commit(ctx, ext, true, s.k1, s.db, s.rb, s.ch, 0, nullptr, &own.t1));
    CP_TRY(cp_challenger_observe(&ch, own.t1->cap_host.data(), cap_w));
  }
  uint64_t alphas[air::MAX_ALPHAS];
  CP_TRY(cp_challenger_challenges(&ch, alphas, s.na));
  cp_poly_batch *traces[2] = {own.t0, own.t1};
  const size_t n_tr = s.k1 ? 2 : 1;
  CP_TRY(cp_air_quotient_commit(ctx, desc->constraints, traces, n_tr, s.q, publics, globals, rch.data(), alphas, s.na, &own.qb));
  CP_TRY(cp_challenger_observe(&ch, own.qb->cap_host.data(), cap_w));
  uint64_t zeta[2], zeta_next[2];
  CP_TRY(cp_challenger_challenges(&ch, zeta, 2));
  uint64_t g = gl::pow(7, (gl::P - 1) >> 32);
  for (int i = s.db; i < 32; i++) g = gl::sqr(g);
  zeta_next[0] = gl::mul(zeta[0], g);
  zeta_next[1] = gl::mul(zeta[1], g);
  if (host_ext_pow(gl::Ext{zeta[0], zeta[1]}, s.n).a == 1 && host_ext_pow(gl::Ext{zeta[0], zeta[1]}, s.n).b == 0)
    return set_error(ctx, CP_ERR_INTERNAL, "zeta fell into the trace domain (probability 2^-%d): retry with another transcript", 128 - s.db);
  std::vector<uint64_t> loc(2 * (s.kt + s.kq)), nxt(2 * s.kt);
  CP_TRY(cp_batch_eval_ext(own.t0, 0, s.k0, zeta, loc.data()));
  if (s.k1) CP_TRY(cp_batch_eval_ext(own.t1, 0, s.k1, zeta, loc.data() + 2 * s.k0));
  CP_TRY(cp_batch_eval_ext(own.qb, 0, s.kq, zeta, loc.data() + 2 * s.kt));
  CP_TRY(cp_batch_eval_ext(own.t0, 0, s.k0, zeta_next, nxt.data()));
  if (s.k1) CP_TRY(cp_batch_eval_ext(own.t1, 0, s.k1, zeta_next, nxt.data() + 2 * s.k0));
  CP_TRY(cp_challenger_observe(&ch, loc.data(), loc.size()));
  CP_TRY(cp_challenger_observe(&ch, nxt.data(), nxt.size()));
  cp_poly_batch *oracles[3] = {own.t0, s.k1 ? own.t1 : own.qb, own.qb};
  const size_t n_or = n_tr + 1;
  const uint32_t qi = (uint32_t)n_tr;
  cp_fri_poly_range r0[3] = {{0, 0, (uint32_t)s.k0}, {1, 0, (uint32_t)s.k1}, {qi, 0, (uint32_t)s.kq}}, r1[2] = {{0, 0, (uint32_t)s.k0}, {1, 0, (uint32_t)s.k1}};
  if (!s.k1) r0[1] = r0[2];
  cp_fri_batch fb[2] = {{{zeta[0], zeta[1]}, r0, s.k1 ? (size_t)3 : (size_t)2}, {{zeta_next[0], zeta_next[1]}, r1, s.k1 ? (size_t)2 : (size_t)1}};
  size_t fri_len = 0;
  CP_TRY(cp_fri_prove(ctx, oracles, n_or, fb, 2, &desc->fri, &ch, use_pow_override, pow_override, &own.fri, &fri_len));
  std::vector<uint8_t> b;
  put_u64(b, n_tr);
  put_u64(b, (uint64_t)1 << s.ch); put_words(b, own.t0->cap_host.data(), cap_w);
  if (s.k1) { put_u64(b, (uint64_t)1 << s.ch); put_words(b, own.t1->cap_host.data(), cap_w); }
  put_u64(b, (uint64_t)1 << s.ch); put_words(b, own.qb->cap_host.data(), cap_w);
  put_u64(b, s.kt); put_words(b, loc.data(), 2 * s.kt);
  put_u64(b, s.kt); put_words(b, nxt.data(), 2 * s.kt);
  put_u64(b, s.kq); put_words(b, loc.data() + 2 * s.kt, 2 * s.kq);
  b.insert(b.end(), own.fri, own.fri + fri_len);
  uint8_t *buf = (uint8_t *)malloc(b.size());
  if (!buf) return set_error(ctx, CP_ERR_OOM, "out of host memory");
  memcpy(buf, b.data(), b.size());
  *proof_out = buf;
  *proof_len = b.size();
  *challenger = ch;
  own.vals_buf.mark_idle();  // cp_fri_prove drained the stream and nothing was enqueued since
  return CP_OK;
} CP_CATCH(ctx)

int cp_stark_prove_batch(cp_ctx *ctx, const cp_stark_desc *desc, size_t n_traces, const uint64_t *const *trace_values, int trace_on_device,
                         const uint64_t *publics, const uint64_t *globals, cp_challenger_state *challengers, const int *use_pow_override,
                         const uint64_t *pow_override, uint8_t **proofs_out, size_t *proof_lens) try {
  // every argument of every instance is checked before anything is staged; nothing of the caller's is written before the last step
  if (n_traces < 1 || n_traces > CP_STARK_BATCH_MAX) return set_error(ctx, CP_ERR_INVALID_ARG, "n_traces %zu out of range [1, %d]", n_traces, CP_STARK_BATCH_MAX);
  if (!trace_values || !challengers || !proofs_out || !proof_lens) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  CHECK_CTX(ctx);
  StarkShape s;
  CP_TRY(stark_shape(ctx, desc, true, s));
  const size_t Bn = n_traces;
  if (Bn * std::max({s.k0, s.k1, s.kq}) > 65535)
    return set_error(ctx, CP_ERR_INVALID_ARG, "%zu traces of %zu columns: more than 65535 polynomials in one launch", Bn, std::max({s.k0, s.k1, s.kq}));
  if ((desc->n_public && !publics) || (desc->n_global && !globals)) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL publics / globals");
  std::vector<int> up(Bn, 0);
  std::vector<uint64_t> ov(Bn, 0);
  for (size_t i = 0; i < Bn; i++) {
    if (!trace_values[i]) return set_error(ctx, CP_ERR_INVALID_ARG, "instance %zu: trace_values is NULL", i);
    if (!all_canonical(publics ? publics + i * desc->n_public : nullptr, desc->n_public) ||
        !all_canonical(globals ? globals + i * desc->n_global : nullptr, desc->n_global))
      return set_error(ctx, CP_ERR_INVALID_ARG, "instance %zu: a public input / global value is not canonical", i);
    if (const char *why = challenger_problem(&challengers[i])) return set_error(ctx, CP_ERR_INVALID_ARG, "instance %zu: %s", i, why);
    if (use_pow_override && use_pow_override[i]) {
      if (!pow_override || pow_override[i] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "instance %zu: pow witness is not canonical", i);
      up[i] = 1;
      ov[i] = pow_override[i];
    }
  }
  StarkBatchOut out;
  {
    // the value columns of both trace rounds of every instance in one array: [instance][execution trace, then the extended columns][n]
    DevBuf vals_buf = ctx->buf(DevOwn::POOLED);  // goes back as reusable only once the stream is known to be idle
    const size_t inst = s.kt * s.n;
    CP_TRY(alloc_status(ctx, vals_buf.alloc(Bn * inst * 8), Bn * inst * 8));
    uint64_t *vals = vals_buf.get<uint64_t>();
    ArenaScope arena_scope(ctx, ctx->arena.used == 0);  // drains the stream and rewinds the arena on every exit, before vals_buf goes back
    if (s.k1) HIP_TRY(ctx, hipMemsetAsync(vals, 0, Bn * inst * 8, ctx->stream));
    for (size_t i = 0; i < Bn; i++)
      HIP_TRY(ctx, hipMemcpyAsync(vals + i * inst, trace_values[i], s.k0 * s.n * 8, trace_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    // host traces are scanned on the device, behind the uploads: one scan of the whole array (the extended columns are zero)
    CP_TRY(canonical_check_enqueue(ctx, vals, trace_on_device ? 0 : Bn * inst, true));
    const int rc = stark_prove_batch_impl(ctx, desc, s, Bn, vals, publics, globals, challengers, up.data(), ov.data(), out);
    if (rc != CP_OK) {
      if (!trace_on_device && canonical_check_failed(ctx)) {  // rare: find the instance and the index for the message on the host
        for (size_t i = 0; i < Bn; i++)
          for (size_t j = 0; j < s.k0 * s.n; j++)
            if (trace_values[i][j] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "instance %zu: trace value %zu is not canonical", i, j);
        return set_error(ctx, CP_ERR_INVALID_ARG, "a trace value was not canonical when it was uploaded (the host array changed during the call)");
      }
      return rc;
    }
    vals_buf.mark_idle();  // the last fetch_flush drained the stream and nothing was enqueued since
  }
  // all or nothing: every buffer first, then the caller's arrays
  std::vector<std::unique_ptr<uint8_t, decltype(&free)>> bufs;
  for (size_t i = 0; i < Bn; i++) {
    const size_t len = out.proofs[i].v.size();
    bufs.emplace_back((uint8_t *)malloc(len ? len : 1), &free);
    if (!bufs.back()) return set_error(ctx, CP_ERR_OOM, "out of host memory");
    memcpy(bufs.back().get(), out.proofs[i].v.data(), len);
  }
  for (size_t i = 0; i < Bn; i++) {
    proofs_out[i] = bufs[i].release();
    proof_lens[i] = out.proofs[i].v.size();
    challengers[i] = out.challengers[i];
  }
  return CP_OK;
} CP_CATCH(ctx)

int cp_stark_verify(const cp_stark_desc *desc, const uint64_t *publics, const uint64_t *globals, cp_challenger_state *challenger, const uint8_t *proof,
                    size_t proof_len) try {
  if (!challenger || !proof) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  StarkShape s;
  CP_TRY(stark_shape(nullptr, desc, false, s));
  if ((desc->n_public && !publics) || (desc->n_global && !globals)) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL publics / globals");
  if (!all_canonical(publics, desc->n_public) || !all_canonical(globals, desc->n_global)) return set_error(nullptr, CP_ERR_INVALID_ARG, "a public input / global value is not canonical");
  if (const char *why = challenger_problem(challenger)) return set_error(nullptr, CP_ERR_INVALID_ARG, "%s", why);
  StarkFront f;
  CP_TRY(stark_verify_front(desc, s, publics, globals, *challenger, proof, proof_len, f));
  StarkFriInstance fi(s, &f);
  CP_TRY(cp_fri_verify(&desc->fri, fi.infos, fi.n_or, fi.cap_ptrs, fi.fb, 2, fi.opened, &f.ch, proof + f.o, proof_len - f.o));
  *challenger = f.ch;
  return CP_OK;
} CP_CATCH(nullptr)

int cp_stark_verify_batch(cp_ctx *ctx, const cp_stark_desc *desc, size_t n_proofs, const uint64_t *publics, const uint64_t *globals,
                          cp_challenger_state *challengers, const uint8_t *const *proofs, const size_t *proof_lens, size_t chunk_proofs,
                          unsigned path_form, cp_verify_verdict *verdicts_out) try {
  // the arguments first, the context last, and nothing of the caller's is written before the last step
  if (!challengers || !proofs || !proof_lens || !verdicts_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (n_proofs == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "no proofs");
  if (path_form > PATHS_COOP) return set_error(ctx, CP_ERR_INVALID_ARG, "path_form %u: 0 (chosen by the library), 1 (one lane per path) or 2 (twelve lanes per path)", path_form);
  StarkShape s;
  CP_TRY(stark_shape(ctx, desc, false, s));
  if ((desc->n_public && !publics) || (desc->n_global && !globals)) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL publics / globals");
  for (size_t i = 0; i < n_proofs; i++) {
    if (!proofs[i] && proof_lens[i]) return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu is NULL", i);
    if (!all_canonical(publics ? publics + i * desc->n_public : nullptr, desc->n_public) ||
        !all_canonical(globals ? globals + i * desc->n_global : nullptr, desc->n_global))
      return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu: a public input / global value is not canonical", i);
    if (const char *why = challenger_problem(&challengers[i])) return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu: %s", i, why);
  }
  friv::Instance D;
  FriVerifyInstance I0;
  size_t proof_words;
  CP_TRY(stark_layout(ctx, desc, s, I0, D, proof_words));
  CHECK_CTX(ctx);
  hostu::alloc_checkpoint();
  std::vector<cp_challenger_state> ch_out(n_proofs);
  std::vector<cp_verify_verdict> verdicts(n_proofs);
  CP_TRY(verify_batch_passes(ctx, D, proof_words, nullptr, proofs, proof_lens, n_proofs, chunk_proofs, (PathForm)path_form, verdicts.data(),
                             [&](size_t p, uint64_t *rec) {
                               return stark_verify_host_phase(desc, s, publics ? publics + p * desc->n_public : nullptr,
                                                              globals ? globals + p * desc->n_global : nullptr, challengers[p], proofs[p], proof_lens[p],
                                                              ch_out[p], rec);
                             }));
  for (size_t i = 0; i < n_proofs; i++) {
    verdicts_out[i] = verdicts[i];
    if (verdicts[i].status == 0) challengers[i] = ch_out[i];
  }
  return CP_OK;
} CP_CATCH(ctx)

}  // extern "C"
