// C ABI of the witness checks (check.h; include/cityprover.h "Does the witness satisfy the circuit, and where not?"): the plonky2
// wire matrix against gates and copy constraints, a STARK trace against the sinks of its AIR. Included at the end of cityprover.hip:
// the circuits, the argument checks and the staging are the provers' own (prover_tail.inc, stark.inc).

namespace {

int64_t key_or_minus_one(unsigned long long key, int shift) { return key == check::NONE ? -1 : (int64_t)(key >> shift); }

// the circuits have passed validate_batch (one shape, one gate set); wires_dev: [proof][num_wires][n]
int check_witness_impl(cp_ctx *ctx, size_t Bn, cp_circuit *const *circuits, const uint64_t *const *pis, const size_t *n_pis, const uint64_t *wires_dev,
                       cp_witness_report *reports, uint64_t *per_gate_out) {
  const cp_circuit &c0 = *circuits[0];
  const cp_shape &sh = c0.sh;
  const size_t n = (size_t)1 << sh.degree_bits, n_gates = c0.gates.size();
  const int R = sh.num_routed_wires;
  ArenaScope arena_scope(ctx);  // drains the stream and rewinds the arena on every exit path
  const uint64_t *omega_tab;
  CP_TRY(get_pow_table(ctx, GL_ROOTS[sh.degree_bits], &omega_tab));
  const uint64_t **d_cs;
  uint64_t *d_pih;
  unsigned long long *d_ctr;
  CP_TRY(arena_alloc(ctx, Bn * sizeof(void *), (void **)&d_cs));
  CP_TRY(arena_alloc(ctx, Bn * 32, (void **)&d_pih));
  CP_TRY(arena_alloc(ctx, Bn * check::C_STRIDE * 8, (void **)&d_ctr));
  std::vector<unsigned long long> ctr(Bn * check::C_STRIDE, 0);
  {
    std::vector<const uint64_t *> h(Bn);
    std::vector<uint64_t> pih(4 * Bn);
    for (size_t p = 0; p < Bn; p++) h[p] = circuits[p]->cs_values;
    host_for(Bn, [&](size_t p) {  // public_inputs_hash, as tail_setup computes it
      uint64_t st[12] = {0};
      for (size_t off = 0; off < n_pis[p]; off += 8) {
        const size_t c = n_pis[p] - off < 8 ? n_pis[p] - off : 8;
        memcpy(st, pis[p] + off, c * 8);
        poseidon::permute_host(st);
      }
      memcpy(&pih[4 * p], st, 32);
    });
    for (size_t p = 0; p < Bn; p++)
      for (int k : {check::C_GATE_KEY, check::C_COPY_KEY, check::C_SIGMA_KEY, check::C_NONCANON_KEY}) ctr[p * check::C_STRIDE + k] = check::NONE;
    CP_TRY(push(ctx, d_cs, h.data(), Bn * sizeof(void *)));
    CP_TRY(push(ctx, d_pih, pih.data(), pih.size() * 8));
    CP_TRY(push(ctx, d_ctr, ctr.data(), ctr.size() * 8));
  }
  check::GateArgs ga{};
  ga.cs = d_cs; ga.wires = wires_dev; ga.wires_stride = (size_t)sh.num_wires * n; ga.pi_hash = d_pih; ga.counters = d_ctr; ga.n = n;
  ga.num_selectors = c0.num_selectors; ga.n_gates = (int)n_gates;
  for (size_t g = 0; g < n_gates; g++) ga.gates[g] = c0.gates[g];
  check::CellArgs ca{};
  ca.cs = d_cs; ca.wires = wires_dev; ca.wires_stride = ga.wires_stride; ca.k_is = c0.k_is; ca.omega_tab = omega_tab; ca.counters = d_ctr; ca.n = n;
  ca.degree_bits = sh.degree_bits; ca.ncst = sh.num_constants; ca.R = R; ca.W = sh.num_wires;
  {
    uint64_t w = gl::inv(GL_ROOTS[sh.degree_bits]);
    for (int b = 0; b < sh.degree_bits; b++) { ca.omega_inv_pow2[b] = w; w = gl::sqr(w); }
  }
  const dim3 grid(blocks_for(n, check::THREADS), (unsigned)Bn), block(check::THREADS);
  for (size_t g = 0; g < n_gates; g++) {  // one instantiation per gate type, as the quotient has: light gates keep their occupancy
    const int gi = (int)g;
    switch (c0.gates[g].type) {
#define CITY_CHECK_CASE(T) case gates::T: LAUNCH(ctx, "check_gate", check::k_gate<gates::T>, grid, block, ga, gi); break;
      CITY_CHECK_GATE_TYPES(CITY_CHECK_CASE)
#undef CITY_CHECK_CASE
      default: break;  // Noop: no constraints
    }
  }
  LAUNCH_LDS(ctx, "check_cells", check::k_cells, grid, block, (size_t)(R > 0 ? R : 1) * 8, ca);
  LAUNCH(ctx, "check_firsts", check::k_firsts, dim3((unsigned)Bn), dim3(64), ga, ca);
  CP_TRY(fetch(ctx, ctr.data(), d_ctr, ctr.size() * 8));  // the one readback of the call
  for (size_t p = 0; p < Bn; p++) {
    const unsigned long long *c = &ctr[p * check::C_STRIDE];
    cp_witness_report r;
    memset(&r, 0, sizeof r);
    for (size_t g = 0; g < n_gates; g++) {
      r.n_gate_violations += c[check::C_PER_GATE + g];
      if (per_gate_out) per_gate_out[p * n_gates + g] = c[check::C_PER_GATE + g];
    }
    r.n_copy_violations = c[check::C_N_COPY];
    r.n_sigma_undecodable = c[check::C_N_SIGMA];
    r.n_noncanonical = c[check::C_N_NONCANON];
    r.gate_row = key_or_minus_one(c[check::C_GATE_KEY], check::GATE_ROW_SHIFT);
    r.gate_index = r.gate_type = r.constraint = -1;
    if (r.gate_row >= 0) {
      r.gate_index = (int32_t)((c[check::C_GATE_KEY] >> check::GATE_INDEX_SHIFT) & ((1u << (check::GATE_ROW_SHIFT - check::GATE_INDEX_SHIFT)) - 1));
      r.gate_type = c0.gates[r.gate_index].type;
      r.constraint = (int32_t)(c[check::C_GATE_KEY] & ((1u << check::GATE_INDEX_SHIFT) - 1));
      r.constraint_value = c[check::C_GATE_VALUE];
    }
    const unsigned cell_mask = (1u << check::CELL_ROW_SHIFT) - 1;
    r.copy_row = key_or_minus_one(c[check::C_COPY_KEY], check::CELL_ROW_SHIFT);
    r.copy_column = r.copy_row >= 0 ? (int32_t)(c[check::C_COPY_KEY] & cell_mask) : -1;
    r.copy_to_row = r.copy_row >= 0 ? (int64_t)c[check::C_COPY_TO_ROW] : -1;
    r.copy_to_column = r.copy_row >= 0 ? (int32_t)c[check::C_COPY_TO_COL] : -1;
    if (r.copy_row >= 0) { r.copy_value = c[check::C_COPY_VALUE]; r.copy_to_value = c[check::C_COPY_TO_VALUE]; }
    r.sigma_row = key_or_minus_one(c[check::C_SIGMA_KEY], check::CELL_ROW_SHIFT);
    r.sigma_column = r.sigma_row >= 0 ? (int32_t)(c[check::C_SIGMA_KEY] & cell_mask) : -1;
    r.noncanonical_row = key_or_minus_one(c[check::C_NONCANON_KEY], check::CELL_ROW_SHIFT);
    r.noncanonical_column = r.noncanonical_row >= 0 ? (int32_t)(c[check::C_NONCANON_KEY] & cell_mask) : -1;
    reports[p] = r;
  }
  return CP_OK;
}

// the sinks of `prog` over n natural rows of cols_dev (n_columns x n); uni: air_uniform_table. Launch geometry as air_run's.
int air_check_impl(cp_ctx *ctx, cp_air_program *prog, const uint64_t *cols_dev, size_t n, const std::vector<uint64_t> &uni, cp_air_check_report *report,
                   uint64_t *per_sink_out) {
  const air::Program &P = prog->P;
  const size_t n_sinks = P.roots.size();
  int K = air_prefetch() ? 1 : air_points_per_lane(ctx);
  while (K > 1 && n < (size_t)air::WAVE * K) K >>= 1;
  const size_t blocks = (n + (size_t)air::WAVE * K - 1) / ((size_t)air::WAVE * K);
  const cp_air_program::Variant *V = nullptr;
  CP_TRY(air_variant(ctx, prog, air_segments_for(ctx, blocks, n_sinks), &V));
  const uint32_t S = V->C.n_segments();
  if (blocks > 0x7FFFFFFFull || S > 65535) return set_error(ctx, CP_ERR_UNSUPPORTED, "AIR launch too large");
  // every segment is a block of its own: the number of its first sink (a segment's sinks are consecutive, in program order)
  std::vector<uint32_t> first_sink(S + 1, 0);
  for (uint32_t s = 0; s < S; s++) {
    uint32_t k = 0;
    for (uint32_t pc = V->C.seg_off[s]; pc < V->C.seg_off[s + 1]; pc++) k += ((uint32_t)V->C.code[pc] & 15) == air::I_SINK;
    first_sink[s + 1] = first_sink[s] + k;
  }
  if (first_sink[S] != n_sinks) return set_error(ctx, CP_ERR_INTERNAL, "the segments hold %u sinks, the program has %zu", first_sink[S], n_sinks);
  size_t lds_max = 0;
  CP_TRY(device_lds_per_block(ctx, lds_max));
  const uint32_t lds_fit = (uint32_t)std::min<size_t>(lds_max / ((size_t)K * air::WAVE * 8), air::DST_NONE);
  if (lds_fit < 1) return set_error(ctx, CP_ERR_UNSUPPORTED, "one AIR slot (%zu B) exceeds the device's %zu B of LDS per workgroup", (size_t)K * air::WAVE * 8, lds_max);
  const uint32_t n_lds = std::min({V->C.n_slots, air_lds_slots(ctx), lds_fit}), n_spill = V->C.n_slots - n_lds;
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);
  std::vector<const uint64_t *> cols(P.n_columns ? P.n_columns : 1, nullptr);
  for (size_t c = 0; c < P.n_columns; c++) cols[c] = cols_dev + c * n;
  std::vector<unsigned long long> ctr(check::A_PER_SINK + n_sinks, 0);
  ctr[check::A_KEY] = check::NONE;
  check::AirArgs a{};
  uint64_t *d_uni;
  const uint64_t **d_cols;
  uint32_t *d_first;
  unsigned long long *d_ctr;
  CP_TRY(arena_alloc(ctx, uni.size() * 8, (void **)&d_uni));
  CP_TRY(arena_alloc(ctx, cols.size() * 8, (void **)&d_cols));
  CP_TRY(arena_alloc(ctx, first_sink.size() * 4, (void **)&d_first));
  CP_TRY(arena_alloc(ctx, ctr.size() * 8, (void **)&d_ctr));
  a.k.spill_stride = (size_t)S * blocks * K * air::WAVE;
  if (n_spill) CP_TRY(arena_alloc(ctx, (size_t)n_spill * a.k.spill_stride * 8, (void **)&a.k.spill));
  CP_TRY(push(ctx, d_uni, uni.data(), uni.size() * 8));
  CP_TRY(push(ctx, d_cols, cols.data(), cols.size() * 8));
  CP_TRY(push(ctx, d_first, first_sink.data(), first_sink.size() * 4));
  CP_TRY(push(ctx, d_ctr, ctr.data(), ctr.size() * 8));
  a.k.code = V->d_code.get<uint64_t>();
  a.k.seg_off = V->d_seg_off.get<uint32_t>();
  a.k.uni = d_uni; a.k.cols = d_cols; a.k.M = n; a.k.n_lds = (int)n_lds;
  a.first_sink = d_first; a.counters = d_ctr; a.n_segments = S;
  const size_t lds_bytes = (size_t)(n_lds ? n_lds : 1) * K * air::WAVE * 8;
  const dim3 grid((unsigned)blocks, S), block(air::WAVE);
  if (K == 4) LAUNCH_LDS(ctx, "air_check", (check::k_air_check<4, false>), grid, block, lds_bytes, a);
  else if (K == 2) LAUNCH_LDS(ctx, "air_check", (check::k_air_check<2, false>), grid, block, lds_bytes, a);
  else LAUNCH_LDS(ctx, "air_check", (check::k_air_check<1, false>), grid, block, lds_bytes, a);
  LAUNCH_LDS(ctx, "air_check_first", (check::k_air_check<1, true>), dim3(1), block, lds_bytes, a);
  CP_TRY(fetch(ctx, ctr.data(), d_ctr, ctr.size() * 8));
  cp_air_check_report r;
  memset(&r, 0, sizeof r);
  for (size_t k = 0; k < n_sinks; k++) {
    r.n_violations += ctr[check::A_PER_SINK + k];
    if (per_sink_out) per_sink_out[k] = ctr[check::A_PER_SINK + k];
  }
  r.row = key_or_minus_one(ctr[check::A_KEY], check::AIR_ROW_SHIFT);
  r.sink = -1;
  r.sink_kind = -1;
  if (r.row >= 0) {
    r.sink = (int64_t)(ctr[check::A_KEY] & ((1u << check::AIR_ROW_SHIFT) - 1));
    r.sink_kind = (int32_t)P.ops[P.roots[(size_t)r.sink]].op;
    r.value = ctr[check::A_VALUE];
  }
  *report = r;
  return CP_OK;
}

}  // namespace

extern "C" {

int cp_circuit_check_witness_dev(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs_host,
                                 const size_t *n_public_inputs, const uint64_t *wires_values_dev, cp_witness_report *reports_out,
                                 uint64_t *per_gate_out) try {
  CHECK_CTX(ctx);
  if (!circuits || !public_inputs_host || !n_public_inputs || !wires_values_dev || !reports_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (n_proofs == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "n_proofs is 0");
  CP_TRY(validate_batch(ctx, n_proofs, circuits, public_inputs_host, n_public_inputs, true, nullptr, nullptr, nullptr, nullptr));
  return check_witness_impl(ctx, n_proofs, circuits, public_inputs_host, n_public_inputs, wires_values_dev, reports_out, per_gate_out);
} CP_CATCH(ctx)

int cp_circuit_check_witness(cp_circuit *circuit, const uint64_t *wires_values_host, const uint64_t *public_inputs_host, size_t n_public_inputs,
                             cp_witness_report *report_out, uint64_t *per_gate_out) try {
  if (!circuit) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_ctx *ctx = circuit->ctx;
  CHECK_CTX(ctx);
  if (!wires_values_host || !report_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  cp_circuit *cs[1] = {circuit};
  const uint64_t *pis[1] = {public_inputs_host}, *ws[1] = {wires_values_host};
  CP_TRY(validate_batch(ctx, 1, cs, pis, &n_public_inputs, true, nullptr, nullptr, nullptr, nullptr));
  const uint64_t *wd, *sd;
  CP_TRY(stage_host_inputs(ctx, 1, cs, ws, nullptr, &wd, &sd));
  return check_witness_impl(ctx, 1, cs, pis, &n_public_inputs, wd, report_out, per_gate_out);
} CP_CATCH(circuit ? circuit->ctx : nullptr)

int cp_air_check_rows_dev(cp_ctx *ctx, const cp_air_program *constraints, const uint64_t *cols_dev, size_t n, const uint64_t *publics,
                          const uint64_t *globals, const uint64_t *challenges, cp_air_check_report *report_out, uint64_t *per_sink_out) try {
  CHECK_CTX(ctx);
  if (!constraints || !report_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  cp_air_program *prog = const_cast<cp_air_program *>(constraints);  // the cache of compiled forms is behind its mutex
  const air::Program &P = prog->P;
  if (P.kind != CP_AIR_CONSTRAINTS) return set_error(ctx, CP_ERR_INVALID_ARG, "not a CP_AIR_CONSTRAINTS program");
  if (prog->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the program belongs to another device");
  if (n == 0 || (n & (n - 1)) || n > ((size_t)1 << 32)) return set_error(ctx, CP_ERR_INVALID_ARG, "n = %zu is not a power of two in [1, 2^32]", n);
  if (P.n_columns && !cols_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL column array");
  std::vector<uint64_t> uni;
  CP_TRY(air_uniform_table(ctx, P, publics, globals, challenges, uni));
  return air_check_impl(ctx, prog, cols_dev, n, uni, report_out, per_sink_out);
} CP_CATCH(ctx)

int cp_stark_check_trace(cp_ctx *ctx, const cp_stark_desc *desc, const uint64_t *trace_values, int trace_on_device, const uint64_t *publics,
                         const uint64_t *globals, const uint64_t *round_challenges, cp_air_check_report *report_out, uint64_t *per_sink_out) try {
  CHECK_CTX(ctx);
  if (!trace_values || !report_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  StarkShape s;
  CP_TRY(stark_shape(ctx, desc, true, s));
  if ((desc->n_public && !publics) || (desc->n_global && !globals) || (desc->n_round_challenges && !round_challenges))
    return set_error(ctx, CP_ERR_INVALID_ARG, "NULL publics / globals / round challenges");
  if (!all_canonical(publics, desc->n_public) || !all_canonical(globals, desc->n_global) || !all_canonical(round_challenges, desc->n_round_challenges))
    return set_error(ctx, CP_ERR_INVALID_ARG, "a public input / global value / round challenge is not canonical");
  // the value columns of both trace rounds in one array, as cp_stark_prove lays them out: execution trace, then the extended columns
  DevBuf vals_buf = ctx->buf();
  CP_TRY(alloc_status(ctx, vals_buf.alloc(s.kt * s.n * 8), s.kt * s.n * 8));
  uint64_t *vals = vals_buf.get<uint64_t>();
  if (trace_on_device) CP_TRY(cp_d2d(ctx, vals, trace_values, s.k0 * s.n * 8));
  else {
    CP_TRY(cp_h2d(ctx, vals, trace_values, s.k0 * s.n * 8));
    CP_TRY(canonical_check_enqueue(ctx, vals, s.k0 * s.n, true));
    HIP_TRY(ctx, sync_stream(ctx));
    if (canonical_check_failed(ctx)) return set_error(ctx, CP_ERR_INVALID_ARG, "a trace value is not canonical");
  }
  if (s.k1) {
    uint64_t *ext = vals + s.k0 * s.n;
    HIP_TRY(ctx, hipMemsetAsync(ext, 0, s.k1 * s.n * 8, ctx->stream));
    for (size_t i = 0; i < desc->n_steps; i++) {
      const cp_stark_step &st = desc->steps[i];
      if (st.kind == CP_STARK_STEP_MAP) CP_TRY(cp_air_map_dev(ctx, st.program, vals, ext, s.n, publics, globals, round_challenges));
      else if (st.kind == CP_STARK_STEP_CUBIC_INVERSE) CP_TRY(cp_cubic_batch_inverse_dev(ctx, st.modulus, ext + (size_t)st.first * s.n, st.count, s.n));
      else CP_TRY(cp_column_prefix_sum_dev(ctx, ext + (size_t)st.first * s.n, st.count, s.n, (int)(st.flags & 1)));
    }
  }
  cp_air_program *prog = const_cast<cp_air_program *>(desc->constraints);
  if (prog->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the constraints program belongs to another device");
  std::vector<uint64_t> uni;
  CP_TRY(air_uniform_table(ctx, prog->P, publics, globals, round_challenges, uni));
  return air_check_impl(ctx, prog, vals, s.n, uni, report_out, per_sink_out);
} CP_CATCH(ctx)

}  // extern "C"
