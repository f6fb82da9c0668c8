// Groth16 keys that nobody holds a trapdoor for (kernels: groth16_srs.h, point_ntt.h; DESIGN.md section 4.6):
//   cp_groth16_srs_*                      a phase-1 powers-of-tau SRS on the device, every point checked
//   cp_groth16_setup_srs_bls12381         the setup of groth16_setup.inc done on points: [L_j] by the inverse point transform of
//                                         the SRS powers, the query points as column sums of the transposed matrices over them,
//                                         Z_j = [tau^(j+N)] - [tau^j]; the key has gamma = delta = 1
//   cp_groth16_key_contribute_bls12381    delta <- d delta, K and Z <- K / d and Z / d, into a new key
//   cp_groth16_key_check_contribution_*   that step checked from the two keys: two MSMs per key, two products of two pairings
//   cp_groth16_srs_unit / _contribute     phase 1 itself: the SRS of tau = alpha = beta = 1, and every point times its own c t^k
//   cp_groth16_srs_points / _check        the SRS back on the host; that its arrays belong together: eight MSMs over adjacent
//                                         pairs under the caller's weights, five products of two pairings in one call
// Included by bls.hip after groth16_setup.inc and point_ntt.inc.
struct cp_groth16_srs {
  explicit cp_groth16_srs(int dev) : device(dev), mem(dev_pool(), dev) {}
  const int device;
  int log_size = 0;
  void *tau_g1 = nullptr, *tau_g2 = nullptr, *alpha_tau_g1 = nullptr, *beta_tau_g1 = nullptr;  // the internal affine form
  uint64_t alpha_g1[12] = {}, beta_g1[12] = {}, beta_g2[24] = {};                              // affine canonical
  DevBag mem;
};

namespace {

void groth16_srs_free(cp_groth16_srs *s) {
  if (!s) return;
  if (s->mem.size()) (void)hipSetDevice(s->device);
  delete s;
}

pointntt::Scalar group_order() {
  pointntt::Scalar r;
  memcpy(r.w, BLS_FR_P32, sizeof r.w);
  return r;
}
template <class F>
bool host_in_torsion(const bls::JacT<F> &p) {
  uint64_t r[4];
  memcpy(r, BLS_FR_P32, sizeof r);
  return bls::jac_is_inf(jac_mul_scalar(p, r));
}

// one array of the descriptor: canonical coordinates (host), conversion, the curve and torsion checks (device)
template <class F>
int srs_array(cp_ctx *ctx, cp_groth16_srs *srs, const uint64_t *xy, size_t n, const char *name, bool torsion, void **out) {
  constexpr size_t W64 = bls::Field<F>::WORDS;  // u64 per point: 2 coordinates of WORDS 32-bit words
  for (size_t i = 0; i < n; i++)
    for (size_t h = 0; h < W64 / 6; h++)
      if (!canonical_words((const uint32_t *)(xy + W64 * i) + 12 * h)) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: %s[%zu]: coordinate is not canonical (>= p)", name, i);
  DevBag tmp = ctx->bag();
  uint64_t *raw = nullptr;
  unsigned long long *first_bad = nullptr;
  const size_t raw_bytes = n * W64 * 8, bytes = n * sizeof(bls::AffineT<F>);
  CP_TRY(alloc_status(ctx, tmp.alloc(&raw, raw_bytes), raw_bytes));
  CP_TRY(alloc_status(ctx, tmp.alloc(&first_bad, 16), 16));
  CP_TRY(alloc_status(ctx, srs->mem.alloc(out, bytes), bytes));
  HIP_TRY(ctx, hipMemcpyAsync(raw, xy, raw_bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(first_bad, 0xff, 16, ctx->stream));
  CP_TRY(msm_prepare_dev<F>(ctx, raw, n, *out));
  LAUNCH(ctx, IS_G1<F> ? "srs_check_g1" : "srs_check_g2", g16srs::k_check_points<F>, dim3(blocks_for(n, fixedbase::LANES<F>)), dim3(fixedbase::LANES<F>),
         (const bls::AffineT<F> *)*out, n, torsion ? 1 : 0, group_order(), first_bad);
  unsigned long long bad[2];
  HIP_TRY(ctx, hipMemcpyAsync(bad, first_bad, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (bad[0] <= bad[1] && bad[0] != ~0ull) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: %s[%llu] is not on the curve", name, bad[0]);
  if (bad[1] != ~0ull) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: %s[%llu] is outside the r-torsion ([r]P is not the point at infinity)", name, bad[1]);
  return CP_OK;
}

int groth16_srs_build(cp_ctx *ctx, const cp_groth16_srs_desc *d, unsigned flags, cp_groth16_srs *srs) {
  if (flags & ~CP_GROTH16_SRS_CHECK_TORSION) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: unknown flags 0x%x", flags);
  if (d->log_size < 1 || d->log_size > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: log_size %d out of range (1 .. 28)", d->log_size);
  if (!d->tau_g1 || !d->tau_g2 || !d->alpha_tau_g1 || !d->beta_tau_g1) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: NULL point array");
  const bool torsion = flags & CP_GROTH16_SRS_CHECK_TORSION;
  const size_t n = (size_t)1 << d->log_size;
  // the key's single points and the trapdoor setup's generators depend on it
  if (memcmp(d->tau_g1, BLS_G1_GEN, sizeof BLS_G1_GEN) != 0) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: tau_g1[0] is not the standard generator of G1");
  if (memcmp(d->tau_g2, BLS_G2_GEN, sizeof BLS_G2_GEN) != 0) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: tau_g2[0] is not the standard generator of G2");
  bls::Jac2 b2;
  CP_TRY(point_in<bls::Fp2>(ctx, d->beta_g2, "SRS: beta_g2", &b2));
  if (torsion && !host_in_torsion(b2)) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: beta_g2 is outside the r-torsion ([r]P is not the point at infinity)");
  srs->log_size = d->log_size;
  CP_TRY(srs_array<bls::Fp>(ctx, srs, d->tau_g1, 2 * n - 1, "tau_g1", torsion, &srs->tau_g1));
  CP_TRY(srs_array<bls::Fp2>(ctx, srs, d->tau_g2, n, "tau_g2", torsion, &srs->tau_g2));
  CP_TRY(srs_array<bls::Fp>(ctx, srs, d->alpha_tau_g1, n, "alpha_tau_g1", torsion, &srs->alpha_tau_g1));
  CP_TRY(srs_array<bls::Fp>(ctx, srs, d->beta_tau_g1, n, "beta_tau_g1", torsion, &srs->beta_tau_g1));
  memcpy(srs->alpha_g1, d->alpha_tau_g1, sizeof srs->alpha_g1);
  memcpy(srs->beta_g1, d->beta_tau_g1, sizeof srs->beta_g1);
  memcpy(srs->beta_g2, d->beta_g2, sizeof srs->beta_g2);
  return CP_OK;
}

// ---- the transposed system as the column kernels read it ----
struct ColumnMatrix {
  std::vector<uint64_t> row_ptr;  // n_wires + 1, kept terms
  std::vector<r1cs::Term> terms;
  const uint64_t *d_row_ptr = nullptr;
  const r1cs::Term *d_terms = nullptr;
};
// rows of T (wires) with their terms sorted by class, zero coefficients dropped (r1cs_build does the same to the rows of a system)
void column_matrix(const g16setup::Csr &T, size_t m, const std::vector<uint32_t> &cls, const std::vector<uint32_t> &small, ColumnMatrix &out) {
  out.row_ptr.resize(m + 1);
  out.terms.reserve(T.col.size());
  for (size_t i = 0; i < m; i++) {
    out.row_ptr[i] = out.terms.size();
    for (uint32_t pass = 0; pass < r1cs::N_CLS; pass++)
      for (size_t t = T.row_ptr[i]; t < T.row_ptr[i + 1]; t++) {
        const uint32_t k = T.coeff[t];
        if (cls[k] != pass) continue;
        out.terms.push_back(r1cs::Term{T.col[t], pass | ((pass == r1cs::CLS_GENERAL ? k : small[k]) << r1cs::TAG_BITS)});
      }
  }
  out.row_ptr[m] = out.terms.size();
}
template <class T>
int upload_vector(cp_ctx *ctx, DevBag &bag, const std::vector<T> &v, const T **out) {
  T *d = nullptr;
  const size_t bytes = v.size() * sizeof(T);
  CP_TRY(alloc_status(ctx, bag.alloc(&d, bytes ? bytes : 1), bytes));
  if (bytes) HIP_TRY(ctx, hipMemcpyAsync(d, v.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  *out = d;
  return CP_OK;
}

// the long wires of a job, cut into chunks (g16srs::k_columns_chunk)
struct LongWires {
  std::vector<uint32_t> wires, chunk_ptr;  // chunk_ptr: wires.size() + 1
  std::vector<g16srs::Chunk> chunks;
  const uint32_t *d_wires = nullptr, *d_chunk_ptr = nullptr;
  const g16srs::Chunk *d_chunks = nullptr;
  void add(uint32_t wire, size_t kept) {
    wires.push_back(wire);
    chunk_ptr.push_back((uint32_t)chunks.size());
    for (size_t first = 0; first < kept; first += g16srs::CHUNK_TERMS) chunks.push_back(g16srs::Chunk{wire, (uint32_t)first});
  }
  int upload(cp_ctx *ctx, DevBag &bag) {
    chunk_ptr.push_back((uint32_t)chunks.size());
    CP_TRY(upload_vector(ctx, bag, wires, &d_wires));
    CP_TRY(upload_vector(ctx, bag, chunk_ptr, &d_chunk_ptr));
    return upload_vector(ctx, bag, chunks, &d_chunks);
  }
};

// work[i] = the job's sum for every wire i; partial: room for one point per chunk
template <class F>
int columns_run(cp_ctx *ctx, const g16srs::Job<F> &J, const LongWires &lw, void *partial, bls::JacT<F> *work) {
  LAUNCH(ctx, IS_G1<F> ? "srs_columns_g1" : "srs_columns_g2", g16srs::k_columns_short<F>, dim3(blocks_for(J.n_wires, fixedbase::LANES<F>)), dim3(fixedbase::LANES<F>), J, work);
  if (lw.wires.empty()) return CP_OK;
  LAUNCH(ctx, IS_G1<F> ? "srs_columns_chunk_g1" : "srs_columns_chunk_g2", g16srs::k_columns_chunk<F>, dim3((unsigned)lw.chunks.size()), dim3(g16srs::CHUNK_TERMS), J, lw.d_chunks,
         (bls::JacT<F> *)partial);
  LAUNCH(ctx, IS_G1<F> ? "srs_columns_combine_g1" : "srs_columns_combine_g2", g16srs::k_columns_combine<F>, dim3((unsigned)lw.wires.size()), dim3(g16srs::CHUNK_TERMS), lw.d_wires,
         lw.d_chunk_ptr, (const bls::JacT<F> *)partial, work);
  return CP_OK;
}

int first_flag(cp_ctx *ctx, const uint8_t *inf, size_t n, unsigned long long *slot_dev, unsigned long long *out) {
  HIP_TRY(ctx, hipMemsetAsync(slot_dev, 0xff, 8, ctx->stream));
  if (n) LAUNCH(ctx, "srs_first_flag", g16srs::k_first_flag, dim3(blocks_for(n, 256)), dim3(256), inf, n, slot_dev);
  HIP_TRY(ctx, hipMemcpyAsync(out, slot_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CP_OK;
}

// the seven device arrays of a key, in the order and the sizes of groth16_setup_run
struct KeyArrays { void *a_g1, *b_g1, *b_g2, *k_g1, *z_g1, *a_inf, *b_inf; };
size_t flag_bytes(size_t m) { return (m + 7) & ~(size_t)7; }  // whole u64: callers copy words
int key_arrays(cp_ctx *ctx, cp_groth16_key *key, size_t m, size_t n_private, size_t N, KeyArrays *a) {
  struct Want { void **p; size_t bytes; } wants[] = {{&a->a_g1, m * CP_G1_AFFINE_BYTES}, {&a->b_g1, m * CP_G1_AFFINE_BYTES}, {&a->b_g2, m * CP_G2_AFFINE_BYTES},
                                                     {&a->k_g1, (n_private ? n_private : 1) * CP_G1_AFFINE_BYTES}, {&a->z_g1, (N - 1) * CP_G1_AFFINE_BYTES},
                                                     {&a->a_inf, flag_bytes(m)}, {&a->b_inf, flag_bytes(m)}};
  for (const Want &w : wants) CP_TRY(alloc_status(ctx, key->mem.alloc(w.p, w.bytes), w.bytes));
  cp_groth16_pk &pk = key->pk;
  pk.a_g1 = a->a_g1; pk.b_g1 = a->b_g1; pk.b_g2 = a->b_g2; pk.k_g1 = a->k_g1; pk.z_g1 = a->z_g1;
  pk.a_inf = (const uint8_t *)a->a_inf; pk.b_inf = (const uint8_t *)a->b_inf;
  return CP_OK;
}

int groth16_setup_srs_run(cp_ctx *ctx, const cp_r1cs_desc *sys, size_t n_public, const cp_groth16_srs *srs, cp_groth16_key *key) {
  using J1 = bls::Jac;
  using J2 = bls::Jac2;
  // ---- every refusal that needs no device: those of groth16_setup_run, in its words ----
  host_phase(ctx, "srs_setup_validate");
  if (srs->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the SRS lives on device %d, the context on device %d", srs->device, ctx->device);
  CP_TRY(r1cs_validate(ctx, sys));
  const size_t n = sys->n_constraints, m = sys->n_wires;
  if (n_public == 0 || n_public > m) return set_error(ctx, CP_ERR_INVALID_ARG, "setup: n_public %zu out of range (1 .. n_wires = %zu; it counts wire 0)", n_public, m);
  if (n < 2) return set_error(ctx, CP_ERR_INVALID_ARG, "setup: a system of one constraint has a domain of one point (log_domain 0), which the prover does not take");
  if (m > ((size_t)1 << 28)) return set_error(ctx, CP_ERR_INVALID_ARG, "setup: n_wires %zu out of range (1 .. 2^28)", m);
  int log_domain = 0;
  while (((size_t)1 << log_domain) < n) log_domain++;
  if (log_domain > srs->log_size)
    return set_error(ctx, CP_ERR_INVALID_ARG, "setup: the system's log_domain %d exceeds the SRS's log_size %d", log_domain, srs->log_size);
  const size_t N = (size_t)1 << log_domain, n_private = m - n_public;
  // ---- the three matrices transposed, their terms classified ----
  host_phase(ctx, "srs_setup_transpose");
  const bool classes = !(sys->flags & CP_R1CS_NO_TERM_CLASSES);
  std::vector<uint32_t> cls(sys->n_coeffs), small(sys->n_coeffs);
  for (size_t k = 0; k < sys->n_coeffs; k++) {
    cls[k] = r1cs::classify(sys->coeffs + 4 * k, &small[k]);
    if (!classes) cls[k] = r1cs::CLS_GENERAL;
  }
  ColumnMatrix M[3];
  const cp_r1cs_matrix *mats[3] = {&sys->a, &sys->b, &sys->c};
  {
    g16setup::Csr T[3];
    for (int k = 0; k < 3; k++) g16setup::transpose_csr(mats[k]->row_ptr, mats[k]->col, mats[k]->coeff, n, m, T[k]);
    for (size_t i = n_public; i < m; i++)
      if (T[0].row_ptr[i] == T[0].row_ptr[i + 1] && T[1].row_ptr[i] == T[1].row_ptr[i + 1] && T[2].row_ptr[i] == T[2].row_ptr[i + 1])
        return set_error(ctx, CP_ERR_INVALID_ARG, "setup: private wire %zu occurs in no constraint: its key point would be the point at infinity", i);
    for (int k = 0; k < 3; k++) {
      column_matrix(T[k], m, cls, small, M[k]);
      T[k] = g16setup::Csr();
    }
  }
  // wires that take workgroups, per job: A alone, B alone, the K / IC combination of the three
  LongWires lw[3];
  for (size_t i = 0; i < m; i++) {
    const size_t la = M[0].row_ptr[i + 1] - M[0].row_ptr[i], lb = M[1].row_ptr[i + 1] - M[1].row_ptr[i], lc = M[2].row_ptr[i + 1] - M[2].row_ptr[i];
    if (la > r1cs::LONG_ROW_THRESHOLD) lw[0].add((uint32_t)i, la);
    if (lb > r1cs::LONG_ROW_THRESHOLD) lw[1].add((uint32_t)i, lb);
    if (la + lb + lc > r1cs::LONG_ROW_THRESHOLD) lw[2].add((uint32_t)i, la + lb + lc);
  }
  // ---- temporaries of this call: the system, the Lagrange points ----
  host_phase(ctx, "srs_setup_lagrange");
  DevBag tmp = ctx->bag();
  for (auto &mat : M) {
    CP_TRY(upload_vector(ctx, tmp, mat.row_ptr, &mat.d_row_ptr));
    CP_TRY(upload_vector(ctx, tmp, mat.terms, &mat.d_terms));
  }
  const uint32_t *d_coeffs = nullptr;
  size_t max_chunks = 1;
  for (auto &l : lw) {
    CP_TRY(l.upload(ctx, tmp));
    if (l.chunks.size() > max_chunks) max_chunks = l.chunks.size();
  }
  void *partial = nullptr;  // the chunk sums of one job at a time
  CP_TRY(alloc_status(ctx, tmp.alloc(&partial, max_chunks * sizeof(J2)), max_chunks * sizeof(J2)));
  {
    uint32_t *c = nullptr;
    const size_t bytes = sys->n_coeffs * 32;
    CP_TRY(alloc_status(ctx, tmp.alloc(&c, bytes ? bytes : 1), bytes));
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(c, sys->coeffs, bytes, hipMemcpyHostToDevice, ctx->stream));
    d_coeffs = c;
  }
  // [L_j]_1, [alpha L_j]_1, [beta L_j]_1, [L_j]_2: the inverse transforms of the first N powers of each array
  void *lag[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t *lag_inf[4] = {nullptr, nullptr, nullptr, nullptr};
  const void *src[4] = {srs->tau_g1, srs->alpha_tau_g1, srs->beta_tau_g1, srs->tau_g2};
  for (int k = 0; k < 4; k++) {
    const size_t bytes = N * (k < 3 ? CP_G1_AFFINE_BYTES : CP_G2_AFFINE_BYTES);
    CP_TRY(alloc_status(ctx, tmp.alloc(&lag[k], bytes), bytes));
    CP_TRY(alloc_status(ctx, tmp.alloc(&lag_inf[k], N), N));
    HIP_TRY(ctx, hipMemcpyAsync(lag[k], src[k], bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(lag_inf[k], 0, N, ctx->stream));
    if (k < 3) CP_TRY(point_ntt_run<bls::Fp>(ctx, lag[k], lag_inf[k], log_domain, CP_NTT_INVERSE));
    else CP_TRY(point_ntt_run<bls::Fp2>(ctx, lag[k], lag_inf[k], log_domain, CP_NTT_INVERSE));
  }
  HIP_TRY(ctx, sync_stream(ctx));  // a profiled call clocks the transforms apart from the columns
  // ---- the point sets: buffers of the key ----
  host_phase(ctx, "srs_setup_columns");
  KeyArrays ka;
  CP_TRY(key_arrays(ctx, key, m, n_private, N, &ka));
  void *kic = nullptr;
  uint8_t *kic_inf = nullptr, *z_inf = nullptr;
  unsigned long long *slot = nullptr;
  CP_TRY(alloc_status(ctx, tmp.alloc(&kic, m * CP_G1_AFFINE_BYTES), m * CP_G1_AFFINE_BYTES));
  CP_TRY(alloc_status(ctx, tmp.alloc(&kic_inf, m), m));
  CP_TRY(alloc_status(ctx, tmp.alloc(&z_inf, N), N));
  CP_TRY(alloc_status(ctx, tmp.alloc(&slot, 8), 8));
  HIP_TRY(ctx, hipMemsetAsync(ka.a_inf, 0, flag_bytes(m), ctx->stream));  // the padding of the last word
  HIP_TRY(ctx, hipMemsetAsync(ka.b_inf, 0, flag_bytes(m), ctx->stream));
  void *w = nullptr;
  CP_TRY(point_work(ctx, m * sizeof(J2) > (N - 1) * sizeof(J1) ? m * sizeof(J2) : (N - 1) * sizeof(J1), &w));
  auto product1 = [&](int mat, int l) { return g16srs::Product<bls::Fp>{M[mat].d_row_ptr, M[mat].d_terms, (const bls::Affine *)lag[l], lag_inf[l]}; };
  {
    g16srs::Job<bls::Fp> J{};
    J.n_products = 1; J.coeffs = d_coeffs; J.n_wires = m;
    J.p[0] = product1(0, 0);
    CP_TRY(columns_run<bls::Fp>(ctx, J, lw[0], partial, (J1 *)w));
    CP_TRY(point_finish<bls::Fp>(ctx, (J1 *)w, m, nullptr, ka.a_g1, (uint8_t *)ka.a_inf));
    J.p[0] = product1(1, 0);
    CP_TRY(columns_run<bls::Fp>(ctx, J, lw[1], partial, (J1 *)w));
    CP_TRY(point_finish<bls::Fp>(ctx, (J1 *)w, m, nullptr, ka.b_g1, (uint8_t *)ka.b_inf));
  }
  {
    g16srs::Job<bls::Fp2> J{};
    J.n_products = 1; J.coeffs = d_coeffs; J.n_wires = m;
    J.p[0] = g16srs::Product<bls::Fp2>{M[1].d_row_ptr, M[1].d_terms, (const bls::Affine2 *)lag[3], lag_inf[3]};
    CP_TRY(columns_run<bls::Fp2>(ctx, J, lw[1], partial, (J2 *)w));
    CP_TRY(point_finish<bls::Fp2>(ctx, (J2 *)w, m, nullptr, ka.b_g2, (uint8_t *)ka.b_inf));  // the same flags again
  }
  {
    g16srs::Job<bls::Fp> J{};  // beta u_i + alpha v_i + w_i, on points
    J.n_products = 3; J.coeffs = d_coeffs; J.n_wires = m;
    J.p[0] = product1(0, 2);
    J.p[1] = product1(1, 1);
    J.p[2] = product1(2, 0);
    CP_TRY(columns_run<bls::Fp>(ctx, J, lw[2], partial, (J1 *)w));
    CP_TRY(point_finish<bls::Fp>(ctx, (J1 *)w, m, nullptr, kic, kic_inf));
  }
  unsigned long long first = 0;
  CP_TRY(first_flag(ctx, kic_inf + n_public, n_private, slot, &first));
  if (first != ~0ull)
    return set_error(ctx, CP_ERR_INVALID_ARG, "setup: private wire %llu has beta u + alpha v + w = 0 at tau: its key point would be the point at infinity",
                     first + (unsigned long long)n_public);
  if (n_private)
    HIP_TRY(ctx, hipMemcpyAsync(ka.k_g1, (const char *)kic + n_public * CP_G1_AFFINE_BYTES, n_private * CP_G1_AFFINE_BYTES, hipMemcpyDeviceToDevice, ctx->stream));
  host_phase(ctx, "srs_setup_z");
  LAUNCH(ctx, "srs_z", g16srs::k_z<bls::Fp>, dim3(blocks_for(N - 1, fixedbase::LANES<bls::Fp>)), dim3(fixedbase::LANES<bls::Fp>), (const bls::Affine *)srs->tau_g1, N, N - 1, (J1 *)w);
  CP_TRY(point_finish<bls::Fp>(ctx, (J1 *)w, N - 1, nullptr, ka.z_g1, z_inf));
  CP_TRY(first_flag(ctx, z_inf, N - 1, slot, &first));
  if (first != ~0ull) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: [tau^(2^%d)]_1 is the generator: tau lies in the evaluation domain", log_domain);
  // ---- the single points: from the SRS, and the generators for gamma = delta = 1 ----
  host_phase(ctx, "srs_setup_rest");
  cp_groth16_pk &pk = key->pk;
  cp_groth16_vk &vk = key->vk;
  memcpy(pk.alpha_g1, srs->alpha_g1, sizeof pk.alpha_g1);
  memcpy(pk.beta_g1, srs->beta_g1, sizeof pk.beta_g1);
  memcpy(pk.beta_g2, srs->beta_g2, sizeof pk.beta_g2);
  memcpy(pk.delta_g1, BLS_G1_GEN, sizeof pk.delta_g1);
  memcpy(pk.delta_g2, BLS_G2_GEN, sizeof pk.delta_g2);
  memcpy(vk.gamma_g2, BLS_G2_GEN, sizeof vk.gamma_g2);
  memcpy(vk.alpha_g1, pk.alpha_g1, sizeof vk.alpha_g1);
  memcpy(vk.beta_g2, pk.beta_g2, sizeof vk.beta_g2);
  memcpy(vk.delta_g2, pk.delta_g2, sizeof vk.delta_g2);
  vk.n_public = n_public;
  pk.n_wires = m;
  pk.n_private = n_private;
  pk.log_domain = log_domain;
  std::vector<bls::Affine> ic(n_public);
  key->ic_inf.resize(n_public);
  key->ic_xy.resize(12 * n_public);
  HIP_TRY(ctx, hipMemcpyAsync(ic.data(), kic, n_public * sizeof(bls::Affine), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(key->ic_inf.data(), kic_inf, n_public, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n_public; i++) {
    uint32_t cw[24];
    bls::fp_to_canonical(ic[i].x, cw);
    bls::fp_to_canonical(ic[i].y, cw + 12);
    memcpy(&key->ic_xy[12 * i], cw, sizeof cw);
  }
  host_phase(ctx, nullptr);
  return CP_OK;
}

// ---- a contribution: delta <- d delta, K <- K / d, Z <- Z / d ----
int contribution_scalar(cp_ctx *ctx, const uint64_t d[4], blsfr::Fr *out) {
  if (!(d[0] | d[1] | d[2] | d[3])) return set_error(ctx, CP_ERR_INVALID_ARG, "contribution: d is zero");
  if (!blsfr::fr_is_canonical((const uint32_t *)d)) return set_error(ctx, CP_ERR_INVALID_ARG, "contribution: d is not canonical (>= r)");
  *out = blsfr::fr_from_canonical((const uint32_t *)d);
  return CP_OK;
}
int key_on_ctx_device(cp_ctx *ctx, const cp_groth16_key *key, const char *what) {
  if (key->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "%s lives on device %d, the context on device %d", what, key->device, ctx->device);
  return CP_OK;
}
// out[i] = scale * in[i] for a set without infinity flags
int scale_set(cp_ctx *ctx, const void *in, size_t n, const uint64_t scale[4], void *out, uint8_t *flags_scratch) {
  void *w = nullptr;
  CP_TRY(point_work(ctx, n * sizeof(bls::Jac), &w));
  LAUNCH(ctx, "point_load", (pointntt::k_load<bls::Fp, false>), dim3(blocks_for(n, 256)), dim3(256), (const bls::Affine *)in, (const uint8_t *)nullptr, n, 0, (bls::Jac *)w);
  return point_finish<bls::Fp>(ctx, (bls::Jac *)w, n, scale, out, flags_scratch);
}

int groth16_contribute_run(cp_ctx *ctx, const cp_groth16_key *key, const uint64_t d[4], cp_groth16_key *out) {
  blsfr::Fr df;
  CP_TRY(contribution_scalar(ctx, d, &df));
  CP_TRY(key_on_ctx_device(ctx, key, "the key"));
  uint64_t d_inv[4];
  blsfr::fr_to_canonical(blsfr::fr_inv(df), (uint32_t *)d_inv);
  const cp_groth16_pk &pk = key->pk;
  const size_t m = pk.n_wires, n_private = pk.n_private, N = (size_t)1 << pk.log_domain;
  KeyArrays ka;
  CP_TRY(key_arrays(ctx, out, m, n_private, N, &ka));
  DevBag tmp = ctx->bag();
  uint8_t *flags = nullptr;
  const size_t flags_bytes = n_private > N ? n_private : N;
  CP_TRY(alloc_status(ctx, tmp.alloc(&flags, flags_bytes), flags_bytes));
  struct Copy { void *dst; const void *src; size_t bytes; } copies[] = {{ka.a_g1, pk.a_g1, m * CP_G1_AFFINE_BYTES}, {ka.b_g1, pk.b_g1, m * CP_G1_AFFINE_BYTES},
                                                                        {ka.b_g2, pk.b_g2, m * CP_G2_AFFINE_BYTES}, {ka.a_inf, pk.a_inf, flag_bytes(m)},
                                                                        {ka.b_inf, pk.b_inf, flag_bytes(m)}};
  for (const Copy &c : copies) HIP_TRY(ctx, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if (n_private) CP_TRY(scale_set(ctx, pk.k_g1, n_private, d_inv, ka.k_g1, flags));
  CP_TRY(scale_set(ctx, pk.z_g1, N - 1, d_inv, ka.z_g1, flags));
  // the two delta points on the host, under the kernels
  bls::Jac d1;
  bls::Jac2 d2;
  CP_TRY(point_in<bls::Fp>(ctx, pk.delta_g1, "the key's delta_g1", &d1));
  CP_TRY(point_in<bls::Fp2>(ctx, pk.delta_g2, "the key's delta_g2", &d2));
  const KeyArrays keep = ka;
  out->pk = pk;
  out->vk = key->vk;
  out->ic_xy = key->ic_xy;
  out->ic_inf = key->ic_inf;
  cp_groth16_pk &opk = out->pk;
  opk.a_g1 = keep.a_g1; opk.b_g1 = keep.b_g1; opk.b_g2 = keep.b_g2; opk.k_g1 = keep.k_g1; opk.z_g1 = keep.z_g1;
  opk.a_inf = (const uint8_t *)keep.a_inf; opk.b_inf = (const uint8_t *)keep.b_inf;
  int inf1, inf2;
  jac_out<bls::Fp>(jac_mul_scalar(d1, d), opk.delta_g1, &inf1);
  jac_out<bls::Fp2>(jac_mul_scalar(d2, d), opk.delta_g2, &inf2);
  if (inf1 || inf2) return set_error(ctx, CP_ERR_INVALID_ARG, "contribution: d times the key's delta is the point at infinity (a delta outside the r-torsion)");
  memcpy(out->vk.delta_g2, opk.delta_g2, sizeof opk.delta_g2);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CP_OK;
}

// ---- the check of a contribution from the two keys alone ----
int device_arrays_differ(cp_ctx *ctx, const void *a, const void *b, size_t bytes, uint32_t *slot_dev, bool *out) {
  HIP_TRY(ctx, hipMemsetAsync(slot_dev, 0, 4, ctx->stream));
  if (bytes) LAUNCH(ctx, "srs_differs", g16srs::k_differs, dim3(blocks_for(bytes, 256)), dim3(256), (const uint8_t *)a, (const uint8_t *)b, bytes, slot_dev);
  uint32_t v = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&v, slot_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *out = v != 0;
  return CP_OK;
}
// a verdict with its reason in the context's message; the call itself succeeds
int contribution_verdict(cp_ctx *ctx, int verdict, int *out, const char *why) {
  (void)set_error(ctx, CP_OK, "contribution check: verdict %d: %s", verdict, why);
  *out = verdict;
  return CP_OK;
}

int groth16_check_contribution_run(cp_ctx *ctx, const cp_groth16_key *before, const cp_groth16_key *after, const uint64_t *weights, int *verdict) {
  CP_TRY(key_on_ctx_device(ctx, before, "the key before"));
  CP_TRY(key_on_ctx_device(ctx, after, "the key after"));
  const cp_groth16_pk &p0 = before->pk, &p1 = after->pk;
  if (p0.n_wires != p1.n_wires || p0.n_private != p1.n_private || p0.log_domain != p1.log_domain || before->vk.n_public != after->vk.n_public)
    return contribution_verdict(ctx, 1, verdict, "the sizes (n_wires, n_private, log_domain, n_public) differ");
  const size_t m = p0.n_wires, n_private = p0.n_private, nz = ((size_t)1 << p0.log_domain) - 1, count = n_private + nz;
  for (size_t i = 0; i < count; i++)
    if (!(weights[2 * i] | weights[2 * i + 1])) return set_error(ctx, CP_ERR_INVALID_ARG, "contribution check: weight %zu is zero", i);
  // ---- what a contribution must not change ----
  struct Single { const void *a, *b; size_t bytes; const char *name; } singles[] = {
      {p0.alpha_g1, p1.alpha_g1, sizeof p0.alpha_g1, "alpha_g1"}, {p0.beta_g1, p1.beta_g1, sizeof p0.beta_g1, "beta_g1"}, {p0.beta_g2, p1.beta_g2, sizeof p0.beta_g2, "beta_g2"},
      {before->vk.alpha_g1, after->vk.alpha_g1, sizeof p0.alpha_g1, "the verifying key's alpha_g1"}, {before->vk.beta_g2, after->vk.beta_g2, sizeof p0.beta_g2, "the verifying key's beta_g2"},
      {before->vk.gamma_g2, after->vk.gamma_g2, sizeof p0.beta_g2, "gamma_g2"}};
  for (const Single &s : singles)
    if (memcmp(s.a, s.b, s.bytes) != 0) {
      char why[96];
      snprintf(why, sizeof why, "%s differs", s.name);
      return contribution_verdict(ctx, 1, verdict, why);
    }
  if (before->ic_xy != after->ic_xy || before->ic_inf != after->ic_inf) return contribution_verdict(ctx, 1, verdict, "an IC point differs");
  if (memcmp(after->vk.delta_g2, p1.delta_g2, sizeof p1.delta_g2) != 0)
    return contribution_verdict(ctx, 1, verdict, "the verifying key's delta_g2 is not the proving key's");
  DevBag tmp = ctx->bag();
  uint32_t *slot = nullptr;
  CP_TRY(alloc_status(ctx, tmp.alloc(&slot, 4), 4));
  struct Set { const void *a, *b; size_t bytes; const char *name; } sets[] = {{p0.a_g1, p1.a_g1, m * CP_G1_AFFINE_BYTES, "a_g1"}, {p0.b_g1, p1.b_g1, m * CP_G1_AFFINE_BYTES, "b_g1"},
                                                                              {p0.b_g2, p1.b_g2, m * CP_G2_AFFINE_BYTES, "b_g2"}, {p0.a_inf, p1.a_inf, m, "a_inf"}, {p0.b_inf, p1.b_inf, m, "b_inf"}};
  for (const Set &s : sets) {
    bool differ = false;
    CP_TRY(device_arrays_differ(ctx, s.a, s.b, s.bytes, slot, &differ));
    if (differ) {
      char why[96];
      snprintf(why, sizeof why, "%s differs", s.name);
      return contribution_verdict(ctx, 1, verdict, why);
    }
  }
  // ---- the new delta points: on the curve and in the r-torsion ----
  bls::Jac d1[2];
  bls::Jac2 d2[2];
  CP_TRY(point_in<bls::Fp>(ctx, p0.delta_g1, "the key before: delta_g1", &d1[0]));
  CP_TRY(point_in<bls::Fp2>(ctx, p0.delta_g2, "the key before: delta_g2", &d2[0]));
  {
    const uint32_t *w1 = (const uint32_t *)p1.delta_g1, *w2 = (const uint32_t *)p1.delta_g2;
    bool ok = canonical_words(w1) && canonical_words(w1 + 12);
    for (int h = 0; h < 4; h++) ok = ok && canonical_words(w2 + 12 * h);
    if (!ok) return contribution_verdict(ctx, 4, verdict, "a delta coordinate of the key after is not canonical (>= p)");
    const bls::Affine a1 = bls::affine_from_canonical<bls::Fp>(w1);
    const bls::Affine2 a2 = bls::affine_from_canonical<bls::Fp2>(w2);
    if (!bls::affine_on_curve(a1)) return contribution_verdict(ctx, 4, verdict, "delta_g1 of the key after is not on the curve");
    if (!bls::affine_on_curve(a2)) return contribution_verdict(ctx, 4, verdict, "delta_g2 of the key after is not on the twist");
    d1[1] = {a1.x, a1.y, bls::fp_one()};
    d2[1] = {a2.x, a2.y, bls::Field<bls::Fp2>::one()};
    if (!host_in_torsion(d1[1])) return contribution_verdict(ctx, 4, verdict, "delta_g1 of the key after is outside the r-torsion");
    if (!host_in_torsion(d2[1])) return contribution_verdict(ctx, 4, verdict, "delta_g2 of the key after is outside the r-torsion");
  }
  // ---- S = sum rho_i K_i + sum sigma_j Z_j over both keys ----
  std::vector<uint64_t> scalars(4 * count, 0);
  for (size_t i = 0; i < count; i++) {
    scalars[4 * i] = weights[2 * i];
    scalars[4 * i + 1] = weights[2 * i + 1];
  }
  uint64_t *d_scalars = nullptr;
  CP_TRY(alloc_status(ctx, tmp.alloc(&d_scalars, count * 32), count * 32));
  HIP_TRY(ctx, hipMemcpyAsync(d_scalars, scalars.data(), count * 32, hipMemcpyHostToDevice, ctx->stream));
  bls::Jac S[2];
  const cp_groth16_pk *pks[2] = {&p0, &p1};
  for (int k = 0; k < 2; k++) {
    bls::Jac sk, sz;
    CP_TRY(msm_run<bls::Fp>(ctx, (const uint32_t *)d_scalars, (const bls::Affine *)pks[k]->k_g1, nullptr, n_private, &sk));
    CP_TRY(msm_run<bls::Fp>(ctx, (const uint32_t *)(d_scalars + 4 * n_private), (const bls::Affine *)pks[k]->z_g1, nullptr, nz, &sz));
    S[k] = bls::jac_add(sk, sz);
  }
  // ---- e(delta_1', delta_2) = e(delta_1, delta_2') and e(S', delta_2') = e(S, delta_2): two products of two pairs ----
  uint64_t g1[4][12], g2[4][24];
  uint8_t g1_inf[4] = {0, 0, 0, 0}, g2_inf[4] = {0, 0, 0, 0}, is_one[2] = {0, 0}, status[2] = {0, 0};
  int inf = 0;
  jac_out<bls::Fp>(d1[1], g1[0], &inf);
  jac_out<bls::Fp>(bls::jac_neg(d1[0]), g1[1], &inf);
  jac_out<bls::Fp>(S[1], g1[2], &inf);
  g1_inf[2] = (uint8_t)inf;
  jac_out<bls::Fp>(bls::jac_neg(S[0]), g1[3], &inf);
  g1_inf[3] = (uint8_t)inf;
  memcpy(g2[0], p0.delta_g2, sizeof g2[0]);
  memcpy(g2[1], p1.delta_g2, sizeof g2[1]);
  memcpy(g2[2], p1.delta_g2, sizeof g2[2]);
  memcpy(g2[3], p0.delta_g2, sizeof g2[3]);
  CP_TRY(cp_pairing_product_bls12381(ctx, &g1[0][0], g1_inf, &g2[0][0], g2_inf, 2, 2, 0, nullptr, is_one, status));
  if (!is_one[0]) return contribution_verdict(ctx, 2, verdict, "e(delta_1', delta_2) != e(delta_1, delta_2')");
  if (!is_one[1]) return contribution_verdict(ctx, 3, verdict, "e(S', delta_2') != e(S, delta_2): K or Z is not the old set under the inverse multiplier");
  return contribution_verdict(ctx, 0, verdict, "the key after is the key before under a non-zero multiplier of delta");
}

// ---- phase 1: the unit SRS, a contribution, the read-back, the consistency check ----
int srs_on_ctx_device(cp_ctx *ctx, const cp_groth16_srs *srs) {
  if (srs->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the SRS lives on device %d, the context on device %d", srs->device, ctx->device);
  return CP_OK;
}

template <class F>
int srs_fill(cp_ctx *ctx, cp_groth16_srs *srs, size_t n, void **out) {
  bls::AffineT<F> gen;
  CP_TRY(generator_mont<F>(ctx, &gen));
  const size_t bytes = n * sizeof(bls::AffineT<F>);
  CP_TRY(alloc_status(ctx, srs->mem.alloc(out, bytes), bytes));
  LAUNCH(ctx, IS_G1<F> ? "srs_fill_g1" : "srs_fill_g2", g16srs::k_fill<F>, dim3(blocks_for(n, 256)), dim3(256), gen, n, (bls::AffineT<F> *)*out);
  return CP_OK;
}

int groth16_srs_unit_run(cp_ctx *ctx, int log_size, cp_groth16_srs *srs) {
  if (log_size < 1 || log_size > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS: log_size %d out of range (1 .. 28)", log_size);
  const size_t n = (size_t)1 << log_size;
  srs->log_size = log_size;
  CP_TRY(srs_fill<bls::Fp>(ctx, srs, 2 * n - 1, &srs->tau_g1));
  CP_TRY(srs_fill<bls::Fp2>(ctx, srs, n, &srs->tau_g2));
  CP_TRY(srs_fill<bls::Fp>(ctx, srs, n, &srs->alpha_tau_g1));
  CP_TRY(srs_fill<bls::Fp>(ctx, srs, n, &srs->beta_tau_g1));
  memcpy(srs->alpha_g1, BLS_G1_GEN, sizeof srs->alpha_g1);
  memcpy(srs->beta_g1, BLS_G1_GEN, sizeof srs->beta_g1);
  memcpy(srs->beta_g2, BLS_G2_GEN, sizeof srs->beta_g2);
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CP_OK;
}

int srs_scalar(cp_ctx *ctx, const uint64_t v[4], const char *name, blsfr::Fr *out) {
  if (!(v[0] | v[1] | v[2] | v[3])) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS contribution: %s is zero", name);
  if (!blsfr::fr_is_canonical((const uint32_t *)v)) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS contribution: %s is not canonical (>= r)", name);
  *out = blsfr::fr_from_canonical((const uint32_t *)v);
  return CP_OK;
}

// *dst (a new array of `out`) [k] = scalar(k) * in[k] for k < n; a result at infinity is refused by array and lowest index
template <class F>
int scale_each_set(cp_ctx *ctx, cp_groth16_srs *out, const void *in, size_t n, const g16srs::EachScalar &S, const char *name, bls::JacT<F> *work, uint8_t *flags,
                   unsigned long long *slot, void **dst) {
  const size_t bytes = n * sizeof(bls::AffineT<F>);
  CP_TRY(alloc_status(ctx, out->mem.alloc(dst, bytes), bytes));
  LAUNCH(ctx, IS_G1<F> ? "srs_scale_each_g1" : "srs_scale_each_g2", g16srs::k_scale_each<F>, dim3(blocks_for(n, fixedbase::LANES<F>)), dim3(fixedbase::LANES<F>),
         (const bls::AffineT<F> *)in, n, S, work);
  CP_TRY(point_finish<F>(ctx, work, n, nullptr, *dst, flags));
  unsigned long long first = 0;
  CP_TRY(first_flag(ctx, flags, n, slot, &first));
  if (first != ~0ull)
    return set_error(ctx, CP_ERR_INVALID_ARG, "SRS contribution: %s[%llu] times its scalar is the point at infinity (a point outside the r-torsion)", name, first);
  return CP_OK;
}

// one entry of a G1 array of the SRS as affine canonical words
int srs_g1_entry(cp_ctx *ctx, const void *arr, size_t index, uint64_t out[12]) {
  bls::Affine p;
  HIP_TRY(ctx, hipMemcpyAsync(&p, (const bls::Affine *)arr + index, sizeof p, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t cw[24];
  bls::fp_to_canonical(p.x, cw);
  bls::fp_to_canonical(p.y, cw + 12);
  memcpy(out, cw, sizeof cw);
  return CP_OK;
}

int groth16_srs_contribute_run(cp_ctx *ctx, const cp_groth16_srs *srs, const uint64_t t[4], const uint64_t a[4], const uint64_t b[4], cp_groth16_srs *out) {
  blsfr::Fr tf, af, bf;
  CP_TRY(srs_scalar(ctx, t, "t", &tf));
  CP_TRY(srs_scalar(ctx, a, "a", &af));
  CP_TRY(srs_scalar(ctx, b, "b", &bf));
  CP_TRY(srs_on_ctx_device(ctx, srs));
  const size_t n = (size_t)1 << srs->log_size, n1 = 2 * n - 1;
  out->log_size = srs->log_size;
  // [b] beta_g2 on the host, under the kernels
  bls::Jac2 b2;
  CP_TRY(point_in<bls::Fp2>(ctx, srs->beta_g2, "the SRS's beta_g2", &b2));
  int inf2 = 0;
  jac_out<bls::Fp2>(jac_mul_scalar(b2, b), out->beta_g2, &inf2);
  if (inf2) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS contribution: beta_g2 times b is the point at infinity (a point outside the r-torsion)");
  DevBag tmp = ctx->bag();
  blsfr::Fr *powers = nullptr;
  uint8_t *flags = nullptr;
  unsigned long long *slot = nullptr;
  CP_TRY(alloc_status(ctx, tmp.alloc(&powers, n1 * sizeof(blsfr::Fr)), n1 * sizeof(blsfr::Fr)));
  CP_TRY(alloc_status(ctx, tmp.alloc(&flags, n1), n1));
  CP_TRY(alloc_status(ctx, tmp.alloc(&slot, 8), 8));
  void *w = nullptr;  // one work array for the four sets, sized for the largest: n points of G2
  CP_TRY(point_work(ctx, n * sizeof(bls::Jac2) > n1 * sizeof(bls::Jac) ? n * sizeof(bls::Jac2) : n1 * sizeof(bls::Jac), &w));
  LAUNCH(ctx, "fr_powers", frntt::k_powers, dim3(blocks_for(n1, 256)), dim3(256), tf, n1, powers);
  const g16srs::EachScalar plain{powers, tf, 0}, with_a{powers, af, 1}, with_b{powers, bf, 1};
  CP_TRY(scale_each_set<bls::Fp>(ctx, out, srs->tau_g1, n1, plain, "tau_g1", (bls::Jac *)w, flags, slot, &out->tau_g1));
  CP_TRY(scale_each_set<bls::Fp2>(ctx, out, srs->tau_g2, n, plain, "tau_g2", (bls::Jac2 *)w, flags, slot, &out->tau_g2));
  CP_TRY(scale_each_set<bls::Fp>(ctx, out, srs->alpha_tau_g1, n, with_a, "alpha_tau_g1", (bls::Jac *)w, flags, slot, &out->alpha_tau_g1));
  CP_TRY(scale_each_set<bls::Fp>(ctx, out, srs->beta_tau_g1, n, with_b, "beta_tau_g1", (bls::Jac *)w, flags, slot, &out->beta_tau_g1));
  CP_TRY(srs_g1_entry(ctx, out->alpha_tau_g1, 0, out->alpha_g1));
  CP_TRY(srs_g1_entry(ctx, out->beta_tau_g1, 0, out->beta_g1));
  return CP_OK;
}

template <class F>
int srs_read(cp_ctx *ctx, const void *pts, size_t n, uint64_t *out_host) {
  if (!out_host) return CP_OK;
  DevBag tmp = ctx->bag();
  uint32_t *raw = nullptr;
  const size_t bytes = n * 2 * bls::Field<F>::WORDS * 4;
  CP_TRY(alloc_status(ctx, tmp.alloc(&raw, bytes), bytes));
  LAUNCH(ctx, IS_G1<F> ? "srs_canonical_g1" : "srs_canonical_g2", g16srs::k_canonical<F>, dim3(blocks_for(n, 256)), dim3(256), (const bls::AffineT<F> *)pts, n, raw);
  HIP_TRY(ctx, hipMemcpyAsync(out_host, raw, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CP_OK;
}

int groth16_srs_points_run(cp_ctx *ctx, const cp_groth16_srs *srs, int *log_size_out, uint64_t *tau_g1, uint64_t *tau_g2, uint64_t *alpha_tau_g1, uint64_t *beta_tau_g1,
                           uint64_t *beta_g2) {
  CP_TRY(srs_on_ctx_device(ctx, srs));
  const size_t n = (size_t)1 << srs->log_size;
  CP_TRY(srs_read<bls::Fp>(ctx, srs->tau_g1, 2 * n - 1, tau_g1));
  CP_TRY(srs_read<bls::Fp2>(ctx, srs->tau_g2, n, tau_g2));
  CP_TRY(srs_read<bls::Fp>(ctx, srs->alpha_tau_g1, n, alpha_tau_g1));
  CP_TRY(srs_read<bls::Fp>(ctx, srs->beta_tau_g1, n, beta_tau_g1));
  if (beta_g2) memcpy(beta_g2, srs->beta_g2, sizeof srs->beta_g2);
  if (log_size_out) *log_size_out = srs->log_size;
  return CP_OK;
}

int srs_verdict(cp_ctx *ctx, int verdict, int *out, const char *why) {
  (void)set_error(ctx, CP_OK, "SRS check: verdict %d: %s", verdict, why);
  *out = verdict;
  return CP_OK;
}

// L = sum w_k P[k], H = sum w_k P[k + 1] over count adjacent pairs: the same scalars over the array and over the array shifted
// by one entry; both as affine canonical words with an infinity flag
template <class F>
int srs_pair_sums(cp_ctx *ctx, const uint64_t *scalars_dev, const void *pts, size_t count, uint64_t *lo_xy, uint8_t *lo_inf, bool negate_lo, uint64_t *hi_xy, uint8_t *hi_inf,
                  bool negate_hi) {
  bls::JacT<F> lo, hi;
  CP_TRY(msm_run<F>(ctx, (const uint32_t *)scalars_dev, (const bls::AffineT<F> *)pts, nullptr, count, &lo));
  CP_TRY(msm_run<F>(ctx, (const uint32_t *)scalars_dev, (const bls::AffineT<F> *)pts + 1, nullptr, count, &hi));
  int inf = 0;
  jac_out<F>(negate_lo ? bls::jac_neg(lo) : lo, lo_xy, &inf);
  *lo_inf = (uint8_t)inf;
  jac_out<F>(negate_hi ? bls::jac_neg(hi) : hi, hi_xy, &inf);
  *hi_inf = (uint8_t)inf;
  return CP_OK;
}

int groth16_srs_check_run(cp_ctx *ctx, const cp_groth16_srs *srs, const uint64_t *weights, int *verdict) {
  CP_TRY(srs_on_ctx_device(ctx, srs));
  const size_t n = (size_t)1 << srs->log_size, count = 5 * n - 5;
  for (size_t i = 0; i < count; i++)
    if (!(weights[2 * i] | weights[2 * i + 1])) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS check: weight %zu is zero", i);
  std::vector<uint64_t> scalars(4 * count, 0);
  for (size_t i = 0; i < count; i++) {
    scalars[4 * i] = weights[2 * i];
    scalars[4 * i + 1] = weights[2 * i + 1];
  }
  DevBag tmp = ctx->bag();
  uint64_t *d_scalars = nullptr;
  CP_TRY(alloc_status(ctx, tmp.alloc(&d_scalars, count * 32), count * 32));
  HIP_TRY(ctx, hipMemcpyAsync(d_scalars, scalars.data(), count * 32, hipMemcpyHostToDevice, ctx->stream));
  // product i is pairs 2 i and 2 i + 1; every equation e(X, Y) = e(X', Y') as e(X, Y) e(-X', Y') = 1
  uint64_t g1[10][12], g2[10][24];
  uint8_t g1_inf[10] = {}, g2_inf[10] = {}, is_one[5] = {}, status[5] = {};
  uint64_t neg_gen[12], t1[12], t2[24];
  {
    bls::Jac g;
    int inf = 0;
    CP_TRY(point_in<bls::Fp>(ctx, BLS_G1_GEN, "the G1 generator", &g));
    jac_out<bls::Fp>(bls::jac_neg(g), neg_gen, &inf);
    CP_TRY(srs_g1_entry(ctx, srs->tau_g1, 1, t1));
    bls::Affine2 q;
    HIP_TRY(ctx, hipMemcpyAsync(&q, (const bls::Affine2 *)srs->tau_g2 + 1, sizeof q, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t cw[48];
    bls::Field<bls::Fp2>::to_canonical(q.x, cw);
    bls::Field<bls::Fp2>::to_canonical(q.y, cw + 24);
    memcpy(t2, cw, sizeof cw);
  }
  const uint64_t *rho = d_scalars, *sigma = rho + 4 * (2 * n - 2), *rho_a = sigma + 4 * (n - 1), *rho_b = rho_a + 4 * (n - 1);
  // rows 1, 3, 4: e(H(P), G2) e(-L(P), tau_g2[1]) = 1
  struct Row1 { int product; const uint64_t *w; const void *pts; size_t pairs; } rows[] = {
      {0, rho, srs->tau_g1, 2 * n - 2}, {2, rho_a, srs->alpha_tau_g1, n - 1}, {3, rho_b, srs->beta_tau_g1, n - 1}};
  for (const Row1 &r : rows) {
    const int h = 2 * r.product, l = h + 1;
    CP_TRY(srs_pair_sums<bls::Fp>(ctx, r.w, r.pts, r.pairs, g1[l], &g1_inf[l], true, g1[h], &g1_inf[h], false));
    memcpy(g2[h], BLS_G2_GEN, sizeof g2[h]);
    memcpy(g2[l], t2, sizeof g2[l]);
  }
  // row 2: e(tau_g1[1], L(tau_g2)) e(-G1, H(tau_g2)) = 1
  CP_TRY(srs_pair_sums<bls::Fp2>(ctx, sigma, srs->tau_g2, n - 1, g2[2], &g2_inf[2], false, g2[3], &g2_inf[3], false));
  memcpy(g1[2], t1, sizeof g1[2]);
  memcpy(g1[3], neg_gen, sizeof g1[3]);
  // row 5: e(beta_tau_g1[0], G2) e(-G1, beta_g2) = 1
  memcpy(g1[8], srs->beta_g1, sizeof g1[8]);
  memcpy(g2[8], BLS_G2_GEN, sizeof g2[8]);
  memcpy(g1[9], neg_gen, sizeof g1[9]);
  memcpy(g2[9], srs->beta_g2, sizeof g2[9]);
  CP_TRY(cp_pairing_product_bls12381(ctx, &g1[0][0], g1_inf, &g2[0][0], g2_inf, 5, 2, 0, nullptr, is_one, status));
  for (int i = 0; i < 5; i++)
    if (status[i] == 3)
      return srs_verdict(ctx, 6, verdict,
                         "a combination of the SRS's points is outside the r-torsion: create the SRS with CP_GROTH16_SRS_CHECK_TORSION to find the point");
  for (int i = 0; i < 5; i++)
    if (status[i] != 0) return set_error(ctx, CP_ERR_INTERNAL, "SRS check: the pairing call refused product %d with status %d", i, (int)status[i]);
  static const char *const why[5] = {
      "e(H(tau_g1), G2) != e(L(tau_g1), tau_g2[1]): tau_g1 is not the powers of the tau of tau_g2[1]",
      "e(tau_g1[1], L(tau_g2)) != e(G1, H(tau_g2)): tau_g2 is not the powers of the tau of tau_g1[1]",
      "e(H(alpha_tau_g1), G2) != e(L(alpha_tau_g1), tau_g2[1]): alpha_tau_g1 is not one alpha times the powers of tau",
      "e(H(beta_tau_g1), G2) != e(L(beta_tau_g1), tau_g2[1]): beta_tau_g1 is not one beta times the powers of tau",
      "e(beta_tau_g1[0], G2) != e(G1, beta_g2): beta_g2 is not the beta of beta_tau_g1"};
  for (int i = 0; i < 5; i++)
    if (!is_one[i]) return srs_verdict(ctx, i + 1, verdict, why[i]);
  return srs_verdict(ctx, 0, verdict, "the arrays are the powers of one tau, one alpha and one beta times them, and [beta]_2 of the same beta");
}

}  // namespace

extern "C" {

cp_groth16_srs *cp_groth16_srs_create_bls12381(cp_ctx *ctx, const cp_groth16_srs_desc *desc, unsigned flags) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  if (!desc) { set_error(ctx, CP_ERR_INVALID_ARG, "SRS: NULL descriptor"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  cp_groth16_srs *srs = new cp_groth16_srs(ctx->device);
  struct Guard { cp_groth16_srs *s; ~Guard() { groth16_srs_free(s); } } guard{srs};
  if (groth16_srs_build(ctx, desc, flags, srs) != CP_OK) return nullptr;
  guard.s = nullptr;
  return srs;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

void cp_groth16_srs_destroy(cp_groth16_srs *srs) try {
  groth16_srs_free(srs);
} catch (...) {
}

cp_groth16_key *cp_groth16_setup_srs_bls12381(cp_ctx *ctx, const cp_r1cs_desc *system, size_t n_public, const cp_groth16_srs *srs) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  if (!system || !srs) { set_error(ctx, CP_ERR_INVALID_ARG, "setup: NULL argument"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  cp_groth16_key *key = new cp_groth16_key(ctx->device);
  struct Guard { cp_groth16_key *k; ~Guard() { groth16_key_free(k); } } guard{key};
  if (groth16_setup_srs_run(ctx, system, n_public, srs, key) != CP_OK) return nullptr;
  guard.k = nullptr;
  return key;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

int cp_groth16_key_contribute_bls12381(cp_ctx *ctx, const cp_groth16_key *key, const uint64_t d[4], cp_groth16_key **key_out) try {
  CHECK_CTX(ctx);
  if (key_out) *key_out = nullptr;
  if (!key || !d || !key_out) return set_error(ctx, CP_ERR_INVALID_ARG, "contribution: NULL argument");
  cp_groth16_key *out = new cp_groth16_key(ctx->device);
  struct Guard { cp_groth16_key *k; ~Guard() { groth16_key_free(k); } } guard{out};
  CP_TRY(groth16_contribute_run(ctx, key, d, out));
  guard.k = nullptr;
  *key_out = out;
  return CP_OK;
} CP_CATCH(ctx)

int cp_groth16_key_check_contribution_bls12381(cp_ctx *ctx, const cp_groth16_key *before, const cp_groth16_key *after, const uint64_t *weights_host,
                                               int *verdict_out) try {
  CHECK_CTX(ctx);
  if (!before || !after || !verdict_out) return set_error(ctx, CP_ERR_INVALID_ARG, "contribution check: NULL argument");
  if (!weights_host) return set_error(ctx, CP_ERR_INVALID_ARG, "contribution check: weights is NULL");
  return groth16_check_contribution_run(ctx, before, after, weights_host, verdict_out);
} CP_CATCH(ctx)

cp_groth16_srs *cp_groth16_srs_unit_bls12381(cp_ctx *ctx, int log_size) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  cp_groth16_srs *srs = new cp_groth16_srs(ctx->device);
  struct Guard { cp_groth16_srs *s; ~Guard() { groth16_srs_free(s); } } guard{srs};
  if (groth16_srs_unit_run(ctx, log_size, srs) != CP_OK) return nullptr;
  guard.s = nullptr;
  return srs;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

int cp_groth16_srs_contribute_bls12381(cp_ctx *ctx, const cp_groth16_srs *srs, const uint64_t t[4], const uint64_t a[4], const uint64_t b[4],
                                       cp_groth16_srs **srs_out) try {
  CHECK_CTX(ctx);
  if (srs_out) *srs_out = nullptr;
  if (!srs || !t || !a || !b || !srs_out) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS contribution: NULL argument");
  cp_groth16_srs *out = new cp_groth16_srs(ctx->device);
  struct Guard { cp_groth16_srs *s; ~Guard() { groth16_srs_free(s); } } guard{out};
  CP_TRY(groth16_srs_contribute_run(ctx, srs, t, a, b, out));
  guard.s = nullptr;
  *srs_out = out;
  return CP_OK;
} CP_CATCH(ctx)

int cp_groth16_srs_points_bls12381(cp_ctx *ctx, const cp_groth16_srs *srs, int *log_size_out, uint64_t *tau_g1_out, uint64_t *tau_g2_out, uint64_t *alpha_tau_g1_out,
                                   uint64_t *beta_tau_g1_out, uint64_t beta_g2_out[24]) try {
  CHECK_CTX(ctx);
  if (!srs) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS points: the SRS is NULL");
  return groth16_srs_points_run(ctx, srs, log_size_out, tau_g1_out, tau_g2_out, alpha_tau_g1_out, beta_tau_g1_out, beta_g2_out);
} CP_CATCH(ctx)

int cp_groth16_srs_check_bls12381(cp_ctx *ctx, const cp_groth16_srs *srs, const uint64_t *weights_host, int *verdict_out) try {
  CHECK_CTX(ctx);
  if (!srs || !verdict_out) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS check: NULL argument");
  if (!weights_host) return set_error(ctx, CP_ERR_INVALID_ARG, "SRS check: weights is NULL");
  return groth16_srs_check_run(ctx, srs, weights_host, verdict_out);
} CP_CATCH(ctx)

}  // extern "C"
