// Host driver of quotient.h (A8): quotient values on the LDE coset -> coefficients, for a batch of proofs of one shape.
// Included by cityprover.hip in front of prover_tail.inc, whose prove_tail_batch_impl calls quot_launch between the second and the
// third commitment. The quotient has four forms (one grid of slices, a workgroup per tile, a launch per gate, the arithmetic family
// as one launch); quot_launch chooses among them, the functions above it are the pieces of that choice.

namespace {

int arena_alloc(cp_ctx *ctx, size_t bytes, void **out);                  // prover_tail.inc
int push(cp_ctx *ctx, void *dev, const void *host, size_t bytes);        // prover_tail.inc

// The gates that read the same first wires of a row and run as ONE piece (quotient.h k_quot_arith_group): the first gate of each of
// the five types; a second gate of a type (same type, other parameters) stays on its own. Returns false, with nothing marked,
// when fewer than two gates qualify. The tile planner and the per-gate path must agree on this for the proof bytes to agree.
bool quot_arith_group(const quot::Gate *gates, int n_gates, quot::ArithGroup &G, bool grouped[quot::MAX_GATES]) {
  G = quot::ArithGroup{-1, -1, -1, -1, -1};
  std::fill(grouped, grouped + quot::MAX_GATES, false);
  int members = 0;
  for (int gi = 0; gi < n_gates; gi++) {
    int *slot = nullptr;
    switch (gates[gi].type) {
      case gates::CONSTANT: slot = &G.constant; break;
      case gates::PUBLIC_INPUT: slot = &G.public_input; break;
      case gates::ARITHMETIC: slot = &G.arithmetic; break;
      case gates::ARITHMETIC_EXT: slot = &G.arithmetic_ext; break;
      case gates::MUL_EXT: slot = &G.mul_ext; break;
      default: break;
    }
    if (slot && *slot < 0) { *slot = gi; grouped[gi] = true; members++; }
  }
  if (members >= 2) return true;
  G = quot::ArithGroup{-1, -1, -1, -1, -1};
  std::fill(grouped, grouped + quot::MAX_GATES, false);
  return false;
}

// what a gate's piece costs (M VALU instructions per proof at the product shape, profiles/r04_pmc_qbench.json: only the
// proportions matter)
double quot_piece_weight(int gate_type) {
  switch (gate_type) {
    case gates::POSEIDON: return 9.7;
    case gates::REDUCING: return 4.5;
    case gates::COMPARISON: return 4.2;
    case gates::REDUCING_EXT: return 3.5;
    case gates::COSET_INTERPOLATION: return 3.2;
    case gates::BASE_SUM: return 2.9;
    case gates::RANDOM_ACCESS: return 1.8;
    case gates::POSEIDON_MDS: return 1.1;
    case gates::ARITHMETIC: case gates::ARITHMETIC_EXT: case gates::MUL_EXT: return 1.5;
    case gates::CONSTANT: case gates::PUBLIC_INPUT: return 0.2;
    default: return 3.0;
  }
}

// The tile form's plan (quotient.h k_quot_tile): which piece each wave of a workgroup evaluates, and the workgroup's LDS. A pure
// function of the gate list and the wire count. Returns false when the form does not fit: more than four pieces per SIMD, or more
// LDS than a workgroup has - the caller then takes the per-gate form.
bool quot_tile_plan(const quot::Gate *gates, int n_gates, int num_wires, quot::TilePieces &P, size_t &lds_bytes) {
  struct Piece { int kind, gi; double w; };
  std::vector<Piece> pieces{{0, -1, 7.1}};  // the permutation argument
  bool grouped[quot::MAX_GATES];
  P = quot::TilePieces{};
  if (quot_arith_group(gates, n_gates, P.G, grouped)) pieces.push_back({2, -1, 4.5});
  for (int gi = 0; gi < n_gates; gi++)
    if (!grouped[gi] && gates[gi].type != gates::NOOP) pieces.push_back({1, gi, quot_piece_weight(gates[gi].type)});
  // longest piece first onto the lightest of four bins; wave w of a workgroup runs on SIMD w mod 4, so slot w takes from bin w mod 4
  std::stable_sort(pieces.begin(), pieces.end(), [](const Piece &x, const Piece &y) { return x.w > y.w; });
  std::vector<Piece> bins[4];
  double load[4] = {0, 0, 0, 0};
  for (const Piece &pc : pieces) {
    int b = 0;
    for (int k = 1; k < 4; k++)
      if (load[k] < load[b]) b = k;
    bins[b].push_back(pc);
    load[b] += pc.w;
  }
  size_t depth = 0;
  for (auto &b : bins) depth = std::max(depth, b.size());
  lds_bytes = std::max((size_t)num_wires, 4 * depth * quot::MAXC) * quot::TILE * 8;
  if (depth > 4 || lds_bytes > 160 * 1024) return false;
  P.n = (int)(4 * depth);
  for (size_t d = 0; d < depth; d++)
    for (int b = 0; b < 4; b++) {
      const size_t slot = 4 * d + b;
      if (d < bins[b].size()) { P.kind[slot] = bins[b][d].kind; P.gi[slot] = bins[b][d].gi; }
      else { P.kind[slot] = 1; P.gi[slot] = -1; }  // an empty slot: a "gate" without constraints
    }
  return true;
}

// a launch per gate that is not in the arithmetic group
int quot_launch_gates(cp_ctx *ctx, const quot::Args &a, const bool *grouped, dim3 qgrid, dim3 qblock) {
  const int t0 = a.t0_gates;
  for (int gi = 0; gi < a.n_gates; gi++) {
    if (grouped[gi]) continue;
    switch (a.gates[gi].type) {
#define CITY_QUOT_GATE(T, NAME) \
  case gates::T: LAUNCH(ctx, "quotient_" NAME, quot::k_quot_gate<gates::T>, qgrid, qblock, a, gi, t0); break;
      CITY_QUOT_GATE(CONSTANT, "constant") CITY_QUOT_GATE(PUBLIC_INPUT, "public_input") CITY_QUOT_GATE(ARITHMETIC, "arithmetic")
      CITY_QUOT_GATE(POSEIDON, "poseidon") CITY_QUOT_GATE(COMPARISON, "comparison") CITY_QUOT_GATE(U32_ARITHMETIC, "u32_arithmetic")
      CITY_QUOT_GATE(U32_RANGE_CHECK, "u32_range_check") CITY_QUOT_GATE(U32_ADD_MANY, "u32_add_many")
      CITY_QUOT_GATE(U32_SUBTRACTION, "u32_subtraction") CITY_QUOT_GATE(U32_INTERLEAVE, "u32_interleave")
      CITY_QUOT_GATE(UNINTERLEAVE_TO_U32, "uninterleave_to_u32") CITY_QUOT_GATE(UNINTERLEAVE_TO_B32, "uninterleave_to_b32")
      CITY_QUOT_GATE(ARITHMETIC_EXT, "arithmetic_ext") CITY_QUOT_GATE(MUL_EXT, "mul_ext") CITY_QUOT_GATE(BASE_SUM, "base_sum")
      CITY_QUOT_GATE(RANDOM_ACCESS, "random_access") CITY_QUOT_GATE(REDUCING, "reducing") CITY_QUOT_GATE(REDUCING_EXT, "reducing_ext")
      CITY_QUOT_GATE(POSEIDON_MDS, "poseidon_mds") CITY_QUOT_GATE(COSET_INTERPOLATION, "coset_interpolation")
      CITY_QUOT_GATE(EXPONENTIATION, "exponentiation")
#undef CITY_QUOT_GATE
      default: break;  // Noop: no constraints
    }
  }
  return CP_OK;
}

// A8 for Bn proofs of shape `sh` with the gate set `gates`: cs_lde = per-proof pointers to the constants / sigmas LDE, wires_lde and
// zs_lde = the two committed oracles [proof][k][N] (bit-reversed), chal = [proof][betas (nc) | gammas (nc)], alphas = [proof][nc],
// head = [proof][circuit_digest (4) | public_inputs_hash (4)]. *out: [proof][nc][N] quotient coefficients, natural order (arena
// memory); chunk j of challenge c = out[c][j*n .. (j+1)*n)
int quot_launch(cp_ctx *ctx, const cp_shape &sh, size_t Bn, const std::vector<quot::Gate> &gates, int num_selectors, const uint64_t *k_is,
                const uint64_t *const *cs_lde, const uint64_t *wires_lde, size_t wires_stride, const uint64_t *zs_lde, size_t zs_stride,
                const uint64_t *chal, const uint64_t *alphas, const uint64_t *head, uint64_t **out) {
  const int db = sh.degree_bits, rb = sh.rate_bits, nc = sh.num_challenges;
  const size_t n = (size_t)1 << db, N = n << rb;
  const unsigned Bu = (unsigned)Bn;
  if (nc > quot::MAXC) return set_error(ctx, CP_ERR_UNSUPPORTED, "more than %d challenges", quot::MAXC);
  if ((1 << rb) != sh.quotient_degree_factor)
    return set_error(ctx, CP_ERR_UNSUPPORTED, "quotient_degree_factor must equal 2^rate_bits");
  quot::Args a;
  memset(&a, 0, sizeof a);
  int ngc = 0;
  for (size_t gi = 0; gi < gates.size(); gi++) {
    a.gates[gi] = gates[gi];
    ngc = std::max(ngc, quot::gate_num_constraints(gates[gi]));
  }
  a.n_gates = (int)gates.size();
  a.num_selectors = num_selectors;
  a.t0_gates = nc + nc * (sh.num_partial_products + 1);
  a.n_terms = a.t0_gates + ngc;
  // small tables: alpha powers (on the device, from the challenges), Z_H on the coset and its inverses (shape constants)
  std::vector<uint64_t> zh(2u << rb);
  const uint64_t gpn = gl::pow(7, n), w8 = GL_ROOTS[rb];
  for (int i = 0; i < (1 << rb); i++) {
    zh[i] = gl::sub(gl::mul(gpn, gl::pow(w8, i)), 1);
    zh[(1 << rb) + i] = gl::inv(zh[i]);
  }
  uint64_t *d_ap, *d_zh, *qv;
  CP_TRY(arena_alloc(ctx, Bn * nc * (size_t)a.n_terms * 8, (void **)&d_ap));
  CP_TRY(arena_alloc(ctx, zh.size() * 8, (void **)&d_zh));
  CP_TRY(arena_alloc(ctx, Bn * nc * N * 8, (void **)&qv));
  LAUNCH(ctx, "quotient_alpha_powers", tr::k_alpha_powers, dim3(blocks_for((size_t)a.n_terms, 64), Bu * (unsigned)nc), dim3(64), alphas, a.n_terms, d_ap);
  CP_TRY(push(ctx, d_zh, zh.data(), zh.size() * 8));
  CP_TRY(get_pow_table(ctx, GL_ROOTS[db + rb], &a.omega_tab));
  CP_TRY(get_l0_table(ctx, db, rb, a.omega_tab, d_zh, &a.l0_tab));
  a.cs_lde = cs_lde;
  a.wires_lde = wires_lde; a.wires_stride = wires_stride;
  a.zs_lde = zs_lde; a.zs_stride = zs_stride;
  a.k_is = k_is;
  a.chal = chal;  // [proof][2][nc]
  a.apow = d_ap;
  a.pi_hash = head + 4;  // [proof] at stride 8: see pi_stride
  a.pi_stride = 8;
  a.zh = d_zh; a.zh_inv = d_zh + (1 << rb);
  a.out = qv; a.out_stride = (size_t)nc * N;
  a.n_field = (uint64_t)n % gl::P;
  a.N = N; a.log_N = db + rb; a.rb = rb;
  a.ncst = sh.num_constants; a.R = sh.num_routed_wires; a.W = sh.num_wires; a.nc = nc; a.npp = sh.num_partial_products;
  a.chunk = sh.quotient_degree_factor;
  a.flip = (int)CP_KNOB(ctx, "QUOT_FLIP", 1);  // 1: odd gate launches walk the batch backwards (quotient.h k_quot_gate)

  // ---- the form ----
  const dim3 qgrid(blocks_for(N, 256), Bu), qblock(256);
  quot::TilePieces P;
  size_t tile_lds = 0;
  quot::ArithGroup G;
  bool grouped[quot::MAX_GATES] = {false};
  if (Bn <= (size_t)CP_KNOB(ctx, "QUOT_ALL_MAX", 4)) {
    // up to four proofs cannot fill the chip with a launch per gate: every piece of the quotient as a slice of ONE grid
    // (quotient.h k_quot_all; CITYPROVER_QUOT_ALL_MAX = largest batch that takes this form, 0 = never)
    a.n_parts = a.n_gates + 1;
    CP_TRY(arena_alloc(ctx, (size_t)a.n_parts * Bn * nc * N * 8, (void **)&a.parts));
    LAUNCH(ctx, "quotient_all", quot::k_quot_all, dim3(blocks_for(N, 256), Bu, (unsigned)a.n_parts), qblock, a);
    LAUNCH(ctx, "quotient_finish", quot::k_quot_finish, qgrid, qblock, a);
  } else if (CP_KNOB(ctx, "QUOT_TILE", 0) && N % quot::TILE == 0 && quot_tile_plan(a.gates, a.n_gates, a.W, P, tile_lds)) {
    // CITYPROVER_QUOT_TILE=1: the whole quotient of a 64-point tile in one workgroup, wires staged in LDS once, one wave per piece
    // (quotient.h k_quot_tile). It reads every wire column ONCE - and it is OFF by default because it measured 20 % slower end to
    // end (profiles/r04_quot_tile_ab.jsonl: 2 075-2 091 -> 1 659-1 675 proofs/s at 64 blocks in flight, one block alone 58.6 -> 61.4-62.1 ms):
    // a workgroup is twelve to sixteen waves of DIFFERENT lengths on one CU, three or four per SIMD at 126 registers, and ends
    // with its PoseidonGate wave, which then runs nearly alone - where a launch per gate keeps eight like waves on every SIMD.
    // The quotient is bound by the latency of its chains, not by HBM (the proof moves 0.5 GB at 1.1 TB/s): trading traffic for
    // occupancy was the wrong trade. Kept for the record and for shapes where it could pay (bytes equal: the GPU suite ran on it).
    // Nothing else to launch: the tile kernel divides by Z_H and writes the natural order itself.
    if (tile_lds > 64 * 1024)  // per device: asked for whenever it is needed (a host-side table lookup)
      HIP_TRY(ctx, hipFuncSetAttribute((const void *)quot::k_quot_tile, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    LAUNCH_LDS(ctx, "quotient_tile", quot::k_quot_tile, dim3((unsigned)(N / quot::TILE), Bu), dim3((unsigned)(P.n * quot::TILE)), tile_lds, a, P);
  } else {
    // a launch per piece, adding into one accumulator; gates that read the same first wires of a row as ONE launch
    // (quotient.h k_quot_arith_group; CITYPROVER_QUOT_GROUP=0: a launch each)
    CP_TRY(arena_alloc(ctx, Bn * nc * N * 8, (void **)&a.acc));
    LAUNCH(ctx, "quotient_perm", quot::k_quot_perm, qgrid, qblock, a);
    if (CP_KNOB(ctx, "QUOT_GROUP", 1) && quot_arith_group(a.gates, a.n_gates, G, grouped)) {
      if (nc <= 2) LAUNCH(ctx, "quotient_arith_group", quot::k_quot_arith_group<2>, qgrid, qblock, a, G, a.t0_gates);
      else LAUNCH(ctx, "quotient_arith_group", quot::k_quot_arith_group<quot::MAXC>, qgrid, qblock, a, G, a.t0_gates);
    }
    CP_TRY(quot_launch_gates(ctx, a, grouped, qgrid, qblock));
    LAUNCH(ctx, "quotient_finish", quot::k_quot_finish, qgrid, qblock, a);
  }
  // coset iFFT (natural in, natural out): coefficients
  CP_TRY(cp_ntt_dev(ctx, qv, db + rb, Bn * nc, N, CP_NTT_INVERSE | CP_NTT_COSET, 7));
  *out = qv;
  return CP_OK;
}

}  // namespace
