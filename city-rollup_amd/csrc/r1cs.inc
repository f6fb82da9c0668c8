// Host side of the device-resident R1CS (kernels: r1cs.h): create validates, classifies and uploads a constraint system;
// eval / check / prove-from-a-witness run on it. Included by bls.hip after groth16.inc.
struct cp_r1cs_bls12381 {
  explicit cp_r1cs_bls12381(int dev) : device(dev), mem(dev_pool(), dev) {}
  const int device;
  cp_r1cs_info info{};
  r1cs::System sys{};  // device pointers
  uint32_t *long_rows = nullptr;
  uint32_t n_long = 0;
  DevBag mem;  // every device array of the handle
};

namespace {

template <class T>
int r1cs_upload(cp_ctx *ctx, cp_r1cs_bls12381 *h, const std::vector<T> &v, const T **out) {
  T *d = nullptr;
  const size_t bytes = v.size() * sizeof(T);
  CP_TRY(alloc_status(ctx, h->mem.alloc(&d, bytes ? bytes : 1), bytes));
  if (bytes) HIP_TRY(ctx, hipMemcpy(d, v.data(), bytes, hipMemcpyHostToDevice));
  h->info.device_bytes += bytes;
  *out = d;
  return CP_OK;
}

void r1cs_free(cp_r1cs_bls12381 *h) {
  if (!h) return;
  if (h->mem.size()) (void)hipSetDevice(h->device);
  delete h;
}

// every refusal of a system, in the order it is read; host work alone (the Groth16 setup refuses a system before it stages anything)
int r1cs_validate(cp_ctx *ctx, const cp_r1cs_desc *desc) {
  const size_t n = desc->n_constraints;
  if (n == 0 || n > ((size_t)1 << 28)) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS: n_constraints %zu out of range (1 .. 2^28)", n);
  if (desc->n_wires == 0 || desc->n_wires > 0xffffffffull) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS: n_wires %zu out of range (1 .. 2^32 - 1)", desc->n_wires);
  if (desc->n_coeffs >= r1cs::MAX_COEFFS) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS: n_coeffs %zu out of range (below 2^29)", desc->n_coeffs);
  if (desc->n_coeffs && !desc->coeffs) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS: coeffs is NULL with n_coeffs = %zu", desc->n_coeffs);
  if (desc->flags & ~CP_R1CS_NO_TERM_CLASSES) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS: unknown flags 0x%x", desc->flags);
  std::vector<uint8_t> canonical(desc->n_coeffs), used(desc->n_coeffs, 0);
  for (size_t k = 0; k < desc->n_coeffs; k++) canonical[k] = blsfr::fr_is_canonical((const uint32_t *)(desc->coeffs + 4 * k));
  const cp_r1cs_matrix *mats[3] = {&desc->a, &desc->b, &desc->c};
  for (int m = 0; m < 3; m++) {
    const cp_r1cs_matrix &M = *mats[m];
    const char name = "ABC"[m];
    if (!M.row_ptr) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS matrix %c: row_ptr is NULL", name);
    if (M.row_ptr[0] != 0) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS matrix %c row 0: row_ptr starts at %llu, not 0", name, (unsigned long long)M.row_ptr[0]);
    for (size_t j = 0; j < n; j++)
      if (M.row_ptr[j + 1] < M.row_ptr[j]) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS matrix %c row %zu: row_ptr decreases (%llu after %llu)", name, j, (unsigned long long)M.row_ptr[j + 1], (unsigned long long)M.row_ptr[j]);
    const size_t nnz = M.row_ptr[n];
    if (nnz && (!M.col || !M.coeff)) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS matrix %c: col / coeff is NULL with %zu terms", name, nnz);
    for (size_t j = 0; j < n; j++)
      for (size_t t = M.row_ptr[j]; t < M.row_ptr[j + 1]; t++) {
        const uint32_t col = M.col[t], k = M.coeff[t];
        if (col >= desc->n_wires) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS matrix %c row %zu: wire %u >= n_wires %zu", name, j, col, desc->n_wires);
        if (k >= desc->n_coeffs) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS matrix %c row %zu: coefficient index %u >= n_coeffs %zu", name, j, k, desc->n_coeffs);
        if (!canonical[k]) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS matrix %c row %zu: coefficient %u is not canonical (>= r)", name, j, k);
        used[k] = 1;
      }
  }
  for (size_t k = 0; k < desc->n_coeffs; k++)
    if (!canonical[k] && !used[k]) return set_error(ctx, CP_ERR_INVALID_ARG, "R1CS: coefficient %zu is not canonical (>= r); no term uses it", k);
  return CP_OK;
}

int r1cs_build(cp_ctx *ctx, const cp_r1cs_desc *desc, cp_r1cs_bls12381 *h) {
  CP_TRY(r1cs_validate(ctx, desc));
  const size_t n = desc->n_constraints;
  const bool classes = !(desc->flags & CP_R1CS_NO_TERM_CLASSES);
  int log_domain = 0;
  while (((size_t)1 << log_domain) < n) log_domain++;
  h->info.n_constraints = n;
  h->info.n_wires = desc->n_wires;
  h->info.n_coeffs = desc->n_coeffs;
  h->info.log_domain = log_domain;
  h->info.long_row_threshold = r1cs::LONG_ROW_THRESHOLD;
  // the coefficient table: class, one-limb constant, Montgomery form
  std::vector<uint32_t> cls(desc->n_coeffs), small(desc->n_coeffs);
  std::vector<blsfr::Fr> mont(desc->n_coeffs);
  for (size_t k = 0; k < desc->n_coeffs; k++) {
    cls[k] = r1cs::classify(desc->coeffs + 4 * k, &small[k]);
    mont[k] = blsfr::fr_from_canonical((const uint32_t *)(desc->coeffs + 4 * k));
    if (!classes) cls[k] = r1cs::CLS_GENERAL;
  }
  const cp_r1cs_matrix *mats[3] = {&desc->a, &desc->b, &desc->c};
  std::vector<uint32_t> long_rows;
  for (int m = 0; m < 3; m++) {
    const cp_r1cs_matrix &M = *mats[m];
    const size_t nnz = M.row_ptr[n];
    h->info.nnz[m] = nnz;
    std::vector<uint64_t> row_ptr(n + 1);
    std::vector<r1cs::Term> terms;
    terms.reserve(nnz);
    for (size_t j = 0; j < n; j++) {
      row_ptr[j] = terms.size();
      // counting sort of the row by class (stable: the given order inside a class)
      for (uint32_t pass = 0; pass < r1cs::N_CLS; pass++)
        for (size_t t = M.row_ptr[j]; t < M.row_ptr[j + 1]; t++) {
          const uint32_t col = M.col[t], k = M.coeff[t];
          if (pass == 0 && cls[k] == r1cs::CLS_ZERO) h->info.n_terms_class[0]++;
          if (cls[k] != pass) continue;
          h->info.n_terms_class[1 + pass]++;
          const uint32_t payload = pass == r1cs::CLS_GENERAL ? k : small[k];
          terms.push_back(r1cs::Term{col, pass | (payload << r1cs::TAG_BITS)});
        }
      const size_t len = terms.size() - row_ptr[j];
      if (len > h->info.longest_row) h->info.longest_row = len;
      if (len > r1cs::LONG_ROW_THRESHOLD) long_rows.push_back(((uint32_t)m << 28) | (uint32_t)j);
    }
    row_ptr[n] = terms.size();
    CP_TRY(r1cs_upload(ctx, h, row_ptr, &h->sys.m[m].row_ptr));
    CP_TRY(r1cs_upload(ctx, h, terms, &h->sys.m[m].terms));
  }
  CP_TRY(r1cs_upload(ctx, h, mont, &h->sys.coeffs));
  const uint32_t *lr = nullptr;
  CP_TRY(r1cs_upload(ctx, h, long_rows, &lr));  // ascending: matrices in order, rows in order
  h->long_rows = (uint32_t *)lr;
  h->n_long = (uint32_t)long_rows.size();
  h->info.n_long_rows = long_rows.size();
  h->info.n_short_rows = 3 * n - long_rows.size();
  h->sys.n = n;
  h->sys.n_pad = (size_t)1 << log_domain;
  return CP_OK;
}

int r1cs_args(cp_ctx *ctx, const cp_r1cs_bls12381 *h, const uint64_t *witness_dev) {
  if (!h) return set_error(ctx, CP_ERR_INVALID_ARG, "r1cs is NULL");
  if (!witness_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "witness is NULL");
  if (h->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "the R1CS lives on device %d, the context on device %d", h->device, ctx->device);
  return CP_OK;
}

// the three products into out[0..2] (each 2^log_domain elements), or - out.p all NULL - the long rows alone into long_vals
int r1cs_eval_run(cp_ctx *ctx, const cp_r1cs_bls12381 *h, const uint64_t *witness_dev, r1cs::Outputs out, uint32_t *long_vals) {
  if (out.p[0])
    LAUNCH(ctx, "r1cs_eval_short", r1cs::k_eval_short, dim3(blocks_for(h->sys.n_pad, r1cs::THREADS), 3), dim3(r1cs::THREADS), h->sys,
           (const uint32_t *)witness_dev, out);
  if (h->n_long)
    LAUNCH(ctx, "r1cs_eval_long", r1cs::k_eval_long, dim3(h->n_long), dim3(r1cs::THREADS), h->sys, (const uint32_t *)witness_dev,
           (const uint32_t *)h->long_rows, out, long_vals);
  return CP_OK;
}

// counts the violated rows; evals = NULL: evaluates the rows itself. Synchronises.
int r1cs_check_run(cp_ctx *ctx, const cp_r1cs_bls12381 *h, const uint64_t *witness_dev, uint64_t *const evals[3], size_t *n_violated,
                   size_t *first_violated) {
  DevBag pool = ctx->bag(DevOwn::POOLED);  // back to the pool on every exit path, as reusable once the stream is idle
  unsigned long long *counters = nullptr;
  uint32_t *long_vals = nullptr;
  CP_TRY(alloc_status(ctx, pool.alloc(&counters, 256), 256));
  const unsigned long long init[2] = {0, ~0ull};
  HIP_TRY(ctx, hipMemcpyAsync(counters, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
  const dim3 grid(blocks_for(h->sys.n, r1cs::THREADS)), block(r1cs::THREADS);
  if (evals) {
    LAUNCH(ctx, "r1cs_check_evals", r1cs::k_check<false>, grid, block, h->sys, (const uint32_t *)witness_dev, (const uint32_t *)nullptr, 0u,
           (const uint32_t *)nullptr, (const uint32_t *)evals[0], (const uint32_t *)evals[1], (const uint32_t *)evals[2], counters);
  } else {
    if (h->n_long) {
      CP_TRY(alloc_status(ctx, pool.alloc(&long_vals, (size_t)h->n_long * 32), (size_t)h->n_long * 32));
      CP_TRY(r1cs_eval_run(ctx, h, witness_dev, r1cs::Outputs{{nullptr, nullptr, nullptr}}, long_vals));
    }
    LAUNCH(ctx, "r1cs_check", r1cs::k_check<true>, grid, block, h->sys, (const uint32_t *)witness_dev, (const uint32_t *)h->long_rows, h->n_long,
           (const uint32_t *)long_vals, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, counters);
  }
  unsigned long long got[2] = {0, 0};
  HIP_TRY(ctx, hipMemcpyAsync(got, counters, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  *n_violated = (size_t)got[0];
  *first_violated = got[0] ? (size_t)got[1] : r1cs::NO_ROW;
  return CP_OK;
}

}  // namespace

extern "C" {

cp_r1cs_bls12381 *cp_r1cs_bls12381_create(cp_ctx *ctx, const cp_r1cs_desc *desc) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  if (!desc) { set_error(ctx, CP_ERR_INVALID_ARG, "R1CS: desc is NULL"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  cp_r1cs_bls12381 *h = new cp_r1cs_bls12381(ctx->device);
  struct Guard { cp_r1cs_bls12381 *h; ~Guard() { r1cs_free(h); } } guard{h};
  if (r1cs_build(ctx, desc, h) != CP_OK) return nullptr;
  guard.h = nullptr;
  return h;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

void cp_r1cs_bls12381_destroy(cp_r1cs_bls12381 *r1cs) try {
  r1cs_free(r1cs);
} catch (...) {
}

int cp_r1cs_bls12381_get_info(const cp_r1cs_bls12381 *r1cs, cp_r1cs_info *out) try {
  if (!r1cs || !out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  *out = r1cs->info;
  return CP_OK;
} CP_CATCH(nullptr)

int cp_r1cs_bls12381_eval_dev(cp_ctx *ctx, const cp_r1cs_bls12381 *r1cs, const uint64_t *witness_dev, uint64_t *a_out_dev,
                              uint64_t *b_out_dev, uint64_t *c_out_dev) try {
  CHECK_CTX(ctx);
  CP_TRY(r1cs_args(ctx, r1cs, witness_dev));
  if (!a_out_dev || !b_out_dev || !c_out_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "an output array is NULL");
  if (a_out_dev == b_out_dev || a_out_dev == c_out_dev || b_out_dev == c_out_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "a, b, c must be distinct arrays");
  return r1cs_eval_run(ctx, r1cs, witness_dev, r1cs::Outputs{{(uint32_t *)a_out_dev, (uint32_t *)b_out_dev, (uint32_t *)c_out_dev}}, nullptr);
} CP_CATCH(ctx)

int cp_r1cs_bls12381_check_dev(cp_ctx *ctx, const cp_r1cs_bls12381 *r1cs, const uint64_t *witness_dev, size_t *n_violated_out,
                               size_t *first_violated_out) try {
  CHECK_CTX(ctx);
  CP_TRY(r1cs_args(ctx, r1cs, witness_dev));
  if (!n_violated_out || !first_violated_out) return set_error(ctx, CP_ERR_INVALID_ARG, "an output pointer is NULL");
  return r1cs_check_run(ctx, r1cs, witness_dev, nullptr, n_violated_out, first_violated_out);
} CP_CATCH(ctx)

int cp_groth16_prove_r1cs_bls12381(cp_ctx *ctx, const cp_groth16_pk *pk, const cp_r1cs_bls12381 *r1cs, const uint64_t *witness_dev,
                                   const uint64_t r[4], const uint64_t s[4], uint64_t out_a[12], uint64_t out_b[24],
                                   uint64_t out_c[12]) try {
  CHECK_CTX(ctx);
  if (!pk) return set_error(ctx, CP_ERR_INVALID_ARG, "proving key is NULL");
  CP_TRY(r1cs_args(ctx, r1cs, witness_dev));
  if (!r || !s || !out_a || !out_b || !out_c) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (pk->n_wires != r1cs->info.n_wires)
    return set_error(ctx, CP_ERR_INVALID_ARG, "the proving key has n_wires = %zu, the R1CS %zu", pk->n_wires, r1cs->info.n_wires);
  if (pk->log_domain != r1cs->info.log_domain)
    return set_error(ctx, CP_ERR_INVALID_ARG, "the proving key has log_domain = %d, the R1CS %d", pk->log_domain, r1cs->info.log_domain);
  DevBag pool = ctx->bag(DevOwn::POOLED);
  uint64_t *ev[3];
  const size_t bytes = r1cs->sys.n_pad * 32;
  for (int k = 0; k < 3; k++) CP_TRY(alloc_status(ctx, pool.alloc(&ev[k], bytes), bytes));
  CP_TRY(r1cs_eval_run(ctx, r1cs, witness_dev, r1cs::Outputs{{(uint32_t *)ev[0], (uint32_t *)ev[1], (uint32_t *)ev[2]}}, nullptr));
  size_t n_violated = 0, first = 0;
  CP_TRY(r1cs_check_run(ctx, r1cs, witness_dev, ev, &n_violated, &first));
  if (n_violated)
    return set_error(ctx, CP_ERR_INVALID_ARG, "the witness does not satisfy the R1CS: %zu of %zu constraints violated, the first is constraint %zu",
                     n_violated, r1cs->info.n_constraints, first);
  return cp_groth16_prove_bls12381(ctx, pk, witness_dev, ev[0], ev[1], ev[2], r, s, out_a, out_b, out_c);
} CP_CATCH(ctx)

}  // extern "C"
