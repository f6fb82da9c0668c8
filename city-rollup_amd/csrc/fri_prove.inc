// C ABI of the two plonky2-level seams (include/cityprover.h "the two plonky2-level seams"): cp_batch_* = plonky2
// `PolynomialBatch` with the data resident on the device, cp_fri_prove = `PolynomialBatch::prove_openings`, cp_fri_verify =
// `verify_fri_proof`. The engine is fri_engine.inc (shared with cp_prove), the verifier verify.inc (shared with
// cp_verify). Reference call site of this pair outside CircuitData::prove: starkyx `ByteStark::prove` / `::verify`,
// city_common_circuit/src/hash/accelerator/sha256/smartgadget.rs:518-524. Included at the end of cityprover.hip.

struct cp_poly_batch {
  cp_ctx *ctx = nullptr;  // nullptr once the context has been destroyed (orphan: cp_batch_destroy is the only call left)
  int device = 0;         // where the buffers live
  size_t k = 0;
  int degree_bits = 0, rate_bits = 0, cap_height = 0, n_salt = 0;
  // pool-owned (dev_mem.h), behind the plain pointers below. A buffer goes back to the pool as reusable only when it was
  // marked idle (cp_batch_destroy, after the stream was drained) or when the whole device has been waited for (a commit
  // that failed half way); cp_batch_device_ptrs marks all five exported: the caller's streams may use them (dev_pool.h)
  DevBuf own[5];
  uint64_t *coeffs = nullptr, *lde = nullptr, *digests = nullptr, *cap = nullptr, *salt = nullptr;
  std::vector<uint64_t> cap_host;
};

namespace {

// the pool itself: dev_pool.h, instantiated in core.h (dev_pool()); the owners: dev_mem.h

// one buffer of the handle, from the pool
int batch_buf(cp_ctx *ctx, cp_poly_batch *b, int i, size_t bytes, uint64_t **out) {
  b->own[i] = DevBuf(dev_pool(), b->device, DevOwn::POOLED, [] { return hipDeviceSynchronize() == hipSuccess; });
  CP_TRY(alloc_status(ctx, b->own[i].alloc(bytes), bytes));
  *out = b->own[i].get<uint64_t>();
  return CP_OK;
}
void batch_register(cp_ctx *ctx, cp_poly_batch *b) {
  std::lock_guard<std::mutex> l(ctx->batches_m);
  ctx->live_batches.push_back(b);
}
void batch_unregister(cp_ctx *ctx, cp_poly_batch *b) {
  std::lock_guard<std::mutex> l(ctx->batches_m);
  for (size_t i = 0; i < ctx->live_batches.size(); i++)
    if (ctx->live_batches[i] == b) { ctx->live_batches[i] = ctx->live_batches.back(); ctx->live_batches.pop_back(); break; }
}
// cp_ctx_destroy: the handles outlive their context as orphans
void batches_orphan(cp_ctx *ctx) {
  std::lock_guard<std::mutex> l(ctx->batches_m);
  for (cp_poly_batch *b : ctx->live_batches) b->ctx = nullptr;
  ctx->live_batches.clear();
}
#define CHECK_BATCH(b)                                                                                        \
  do {                                                                                                        \
    if (!(b)) return set_error(nullptr, CP_ERR_INVALID_ARG, "batch is NULL");                                 \
    if (!(b)->ctx) return set_error(nullptr, CP_ERR_INVALID_ARG, "the context of this batch was destroyed");  \
  } while (0)

// natural-order rows of the bit-reversed, polynomial-major LDE: out[r][j] = lde[j][bitrev((first + r) * step)]
__global__ __launch_bounds__(256) void k_lde_rows(const uint64_t *__restrict__ lde, size_t N, int log_N, size_t k, size_t first, size_t count,
                                                  size_t step, uint64_t *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= count * k) return;
  const size_t r = t / k, j = t % k;
  const size_t nat = ((first + r) * step) & (N - 1);
  const size_t pos = log_N ? (size_t)(__brevll((unsigned long long)nat) >> (64 - log_N)) : 0;
  out[t] = lde[j * N + pos];
}

// Merkle leaves in leaf order: out[r][j] = lde[j][first + r], then the salt elements of that leaf
__global__ __launch_bounds__(256) void k_leaves(const uint64_t *__restrict__ lde, const uint64_t *__restrict__ salt, size_t N, size_t k, int n_salt,
                                                size_t first, size_t count, uint64_t *__restrict__ out) {
  const size_t w = k + (size_t)n_salt, t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= count * w) return;
  const size_t r = t / w, j = t % w;
  out[t] = j < k ? lde[j * N + first + r] : salt[(j - k) * N + first + r];
}

// src: device (from_dev) or host polynomials; on success *out owns everything
int poly_batch_commit(cp_ctx *ctx, const uint64_t *src, bool from_dev, size_t k, int db, int rb, int ch, unsigned flags, const uint64_t *salts,
                      cp_poly_batch **out, bool check_host_input = false) {
  if (!src || !out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  *out = nullptr;
  if (flags & ~CP_BATCH_FROM_COEFFS) return set_error(ctx, CP_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
  if (k == 0 || k > 65535) return set_error(ctx, CP_ERR_INVALID_ARG, "k %zu out of range [1, 65535]", k);
  if (db < 0 || rb < 0 || db + rb > 30 || db + rb < 1) return set_error(ctx, CP_ERR_INVALID_ARG, "degree_bits / rate_bits out of range");
  const size_t n = (size_t)1 << db, N = n << rb;
  if (!valid_merkle_shape(N, ch)) return set_error(ctx, CP_ERR_INVALID_ARG, "cap_height %d out of range for 2^%d leaves", ch, db + rb);
  std::unique_ptr<cp_poly_batch> guard(new (std::nothrow) cp_poly_batch());  // dropped on a failure: the owners wait for the device
  cp_poly_batch *b = guard.get();
  if (!b) return set_error(ctx, CP_ERR_OOM, "out of host memory");
  b->ctx = ctx; b->device = ctx->device; b->k = k; b->degree_bits = db; b->rate_bits = rb; b->cap_height = ch;
  CP_TRY(batch_buf(ctx, b, 0, b->k * ((size_t)8 << db), &b->coeffs));
  CP_TRY(batch_buf(ctx, b, 1, b->k * N * 8, &b->lde));
  CP_TRY(batch_buf(ctx, b, 2, merkle_words_per_tree(N, ch) * 8, &b->digests));
  CP_TRY(batch_buf(ctx, b, 3, ((size_t)4 << ch) * 8, &b->cap));
  if (salts) {
    b->n_salt = CP_SALT_SIZE;
    CP_TRY(batch_buf(ctx, b, 4, (size_t)CP_SALT_SIZE * N * 8, &b->salt));
    if (from_dev) CP_TRY(cp_d2d(ctx, b->salt, salts, (size_t)CP_SALT_SIZE * N * 8));
    else CP_TRY(cp_h2d(ctx, b->salt, salts, (size_t)CP_SALT_SIZE * N * 8));
  }
  // values (or coefficients) land in the coefficient array; values are transformed in place
  if (from_dev) CP_TRY(cp_d2d(ctx, b->coeffs, src, k * n * 8));
  else CP_TRY(cp_h2d(ctx, b->coeffs, src, k * n * 8));
  if (check_host_input) {  // host arrays are scanned for elements >= p on the device, behind the upload; read below, after the cap
    CP_TRY(canonical_check_enqueue(ctx, b->coeffs, k * n, true));
    if (salts) CP_TRY(canonical_check_enqueue(ctx, b->salt, (size_t)CP_SALT_SIZE * N, false));
  }
  if (!(flags & CP_BATCH_FROM_COEFFS) && db > 0) CP_TRY(cp_ntt_dev(ctx, b->coeffs, db, k, n, CP_NTT_INVERSE, 0));
  CP_TRY(cp_lde_dev(ctx, b->coeffs, n, db, rb, k, 7, CP_NTT_BITREV_OUT, b->lde, N));
  CP_TRY(merkle_cols_batch(ctx, b->lde, N, k, N, 1, k * N, ch, b->digests, b->cap, b->salt, b->n_salt, 0));
  b->cap_host.resize((size_t)4 << ch);
  CP_TRY(cp_d2h(ctx, b->cap_host.data(), b->cap, b->cap_host.size() * 8));
  if (check_host_input && canonical_check_failed(ctx)) {  // rare: find the index for the message on the host
    for (size_t i = 0; i < k * n; i++)
      if (src[i] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "polynomial element %zu is not canonical", i);
    for (size_t i = 0; salts && i < (size_t)CP_SALT_SIZE * N; i++)
      if (salts[i] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "salt element %zu is not canonical", i);
    return set_error(ctx, CP_ERR_INVALID_ARG, "an element was not canonical when it was uploaded (the host array changed during the call)");
  }
  for (uint64_t v : b->cap_host)
    if (v >= gl::P) return set_error(ctx, CP_ERR_INTERNAL, "non-canonical cap element");
  batch_register(ctx, b);
  *out = guard.release();
  return CP_OK;
}

inline void challenger_load(HostChallenger &C, const cp_challenger_state &s) {
  memcpy(C.state, s.sponge_state, sizeof C.state);
  memcpy(C.in, s.input_buffer, sizeof C.in);
  memcpy(C.out, s.output_buffer, sizeof C.out);
  C.n_in = (int)s.n_input;
  C.n_out = (int)s.n_output;
}
inline void challenger_store(const HostChallenger &C, cp_challenger_state &s) {
  memcpy(s.sponge_state, C.state, sizeof C.state);
  memset(s.input_buffer, 0, sizeof s.input_buffer);
  memset(s.output_buffer, 0, sizeof s.output_buffer);
  memcpy(s.input_buffer, C.in, (size_t)C.n_in * 8);
  memcpy(s.output_buffer, C.out, (size_t)C.n_out * 8);
  s.n_input = (uint32_t)C.n_in;
  s.n_output = (uint32_t)C.n_out;
}
const char *challenger_problem(const cp_challenger_state *s) {
  if (!s) return "challenger is NULL";
  if (s->n_input >= 8) return "challenger: input_buffer holds 8 or more elements (plonky2 duplexes at 8)";
  if (s->n_output > 8) return "challenger: output_buffer holds more than 8 elements";
  for (int i = 0; i < 12; i++) if (s->sponge_state[i] >= gl::P) return "challenger: sponge state element is not canonical";
  for (uint32_t i = 0; i < s->n_input; i++) if (s->input_buffer[i] >= gl::P) return "challenger: input element is not canonical";
  for (uint32_t i = 0; i < s->n_output; i++) if (s->output_buffer[i] >= gl::P) return "challenger: output element is not canonical";
  return nullptr;
}
int load_fri_cfg(cp_ctx *ctx, const cp_fri_params *params, FriCfg &cfg) {
  cfg.rate_bits = params->rate_bits; cfg.cap_height = params->cap_height; cfg.pow_bits = params->pow_bits;
  cfg.num_query_rounds = params->num_query_rounds; cfg.n_arity = params->n_arity;
  for (int l = 0; l < 8; l++) cfg.arity_bits[l] = params->arity_bits[l];
  if (const char *why = fri_cfg_problem(params->degree_bits, cfg)) return set_error(ctx, CP_ERR_INVALID_ARG, "FriParams: %s", why);
  return CP_OK;
}

}  // namespace

extern "C" {

int cp_batch_commit(cp_ctx *ctx, const uint64_t *polys_host, size_t k, int degree_bits, int rate_bits, int cap_height, unsigned flags,
                    const uint64_t *salts_host, cp_poly_batch **batch_out) try {
  CHECK_CTX(ctx);
  return poly_batch_commit(ctx, polys_host, false, k, degree_bits, rate_bits, cap_height, flags, salts_host, batch_out, true);
} CP_CATCH(ctx)

int cp_batch_commit_dev(cp_ctx *ctx, const uint64_t *polys_dev, size_t k, int degree_bits, int rate_bits, int cap_height, unsigned flags,
                        const uint64_t *salts_dev, cp_poly_batch **batch_out) try {
  CHECK_CTX(ctx);
  return poly_batch_commit(ctx, polys_dev, true, k, degree_bits, rate_bits, cap_height, flags, salts_dev, batch_out);
} CP_CATCH(ctx)

void cp_batch_destroy(cp_poly_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  if (b->ctx) {  // every entry point drains the stream before it returns; this is the belt to those braces
    (void)hipStreamSynchronize(b->ctx->stream);
    batch_unregister(b->ctx, b);
  }
  for (DevBuf &o : b->own) o.mark_idle();  // exported ones stay exported
  delete b;
}

int cp_batch_pool_stats(int device, cp_batch_pool_info *out) try {
  if (!out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  const auto st = dev_pool().stats(device);
  out->bytes = st.bytes; out->buffers = st.buffers; out->hits = st.hits; out->misses = st.misses; out->trims = st.trims;
  out->cap_bytes = dev_pool().cap();
  out->pooled = dev_pool().has_pool(device) ? 1 : 0;
  return CP_OK;
} CP_CATCH(nullptr)

int cp_batch_pool_trim(cp_ctx *ctx, size_t *released_out) try {
  CHECK_CTX(ctx);
  const size_t r = dev_pool().trim(ctx->device);
  if (released_out) *released_out = r;
  return CP_OK;
} CP_CATCH(ctx)

int cp_batch_info(const cp_poly_batch *b, size_t *k_out, int *degree_bits_out, int *rate_bits_out, int *cap_height_out, int *n_salt_out) try {
  if (!b) return set_error(nullptr, CP_ERR_INVALID_ARG, "batch is NULL");
  if (k_out) *k_out = b->k;
  if (degree_bits_out) *degree_bits_out = b->degree_bits;
  if (rate_bits_out) *rate_bits_out = b->rate_bits;
  if (cap_height_out) *cap_height_out = b->cap_height;
  if (n_salt_out) *n_salt_out = b->n_salt;
  return CP_OK;
} CP_CATCH(nullptr)

int cp_batch_cap(cp_poly_batch *b, uint64_t *cap_out) try {
  CHECK_BATCH(b);
  if (!cap_out) return set_error(b->ctx, CP_ERR_INVALID_ARG, "NULL argument");
  memcpy(cap_out, b->cap_host.data(), b->cap_host.size() * 8);
  return CP_OK;
} CP_CATCH(b ? b->ctx : nullptr)

int cp_batch_device_ptrs(cp_poly_batch *b, const uint64_t **coeffs_dev_out, const uint64_t **lde_dev_out) try {
  CHECK_BATCH(b);
  for (DevBuf &o : b->own) o.mark_exported();
  if (coeffs_dev_out) *coeffs_dev_out = b->coeffs;
  if (lde_dev_out) *lde_dev_out = b->lde;
  return CP_OK;
} CP_CATCH(b ? b->ctx : nullptr)

int cp_batch_eval_ext(cp_poly_batch *b, size_t first, size_t count, const uint64_t point[2], uint64_t *out_host) try {
  CHECK_BATCH(b);
  cp_ctx *ctx = b->ctx;
  CHECK_CTX(ctx);
  if (count == 0) return CP_OK;
  if (!point || !out_host) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (first > b->k || count > b->k - first) return set_error(ctx, CP_ERR_INVALID_ARG, "polynomials [%zu, %zu) out of range (k = %zu)", first, first + count, b->k);
  if (point[0] >= gl::P || point[1] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "point is not canonical");
  const size_t n = (size_t)1 << b->degree_bits;
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);
  gl::Ext *d_pt, *zpow, *d_out;
  CP_TRY(arena_alloc(ctx, 16, (void **)&d_pt));
  CP_TRY(arena_alloc(ctx, n * 16, (void **)&zpow));
  CP_TRY(arena_alloc(ctx, count * 16, (void **)&d_out));
  const gl::Ext pt{point[0], point[1]};
  CP_TRY(push(ctx, d_pt, &pt, 16));
  LAUNCH(ctx, "fri_ext_powers", fri::k_ext_powers, dim3(blocks_for(n, 256), 1), dim3(256), d_pt, n, zpow);
  LAUNCH(ctx, "eval_at_point", fri::k_eval_at_point, dim3((unsigned)count, 1), dim3(256), b->coeffs + first * n, (size_t)0,
         (const uint64_t *const *)nullptr, n, zpow, n, d_out, count, (size_t)0);
  return fetch(ctx, out_host, d_out, count * 16);
} CP_CATCH(b ? b->ctx : nullptr)

int cp_batch_lde_rows(cp_poly_batch *b, size_t first_index, size_t count, size_t step, uint64_t *out_host) try {
  CHECK_BATCH(b);
  cp_ctx *ctx = b->ctx;
  CHECK_CTX(ctx);
  if (count == 0) return CP_OK;
  if (!out_host) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  const int log_N = b->degree_bits + b->rate_bits;
  const size_t N = (size_t)1 << log_N;
  if (step == 0 || step > N || count > N || first_index >= N) return set_error(ctx, CP_ERR_INVALID_ARG, "index / count / step out of range");
  if (count * b->k > ((size_t)1 << 31)) return set_error(ctx, CP_ERR_INVALID_ARG, "more than 2^31 values per call: fetch in slices");
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);  // gather scratch: the context's arena (drained and rewound on every exit)
  uint64_t *d_out = nullptr;
  CP_TRY(arena_alloc(ctx, count * b->k * 8, (void **)&d_out));
  LAUNCH(ctx, "batch_lde_rows", k_lde_rows, dim3(blocks_for(count * b->k, 256)), dim3(256), b->lde, N, log_N, b->k, first_index, count, step, d_out);
  return cp_d2h(ctx, out_host, d_out, count * b->k * 8);
} CP_CATCH(b ? b->ctx : nullptr)

int cp_batch_coeffs(cp_poly_batch *b, size_t first, size_t count, uint64_t *out_host) try {
  CHECK_BATCH(b);
  cp_ctx *ctx = b->ctx;
  CHECK_CTX(ctx);
  if (count == 0) return CP_OK;
  if (!out_host) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (first > b->k || count > b->k - first) return set_error(ctx, CP_ERR_INVALID_ARG, "polynomials [%zu, %zu) out of range (k = %zu)", first, first + count, b->k);
  const size_t n = (size_t)1 << b->degree_bits;
  return cp_d2h(ctx, out_host, b->coeffs + first * n, count * n * 8);
} CP_CATCH(b ? b->ctx : nullptr)

int cp_batch_leaves(cp_poly_batch *b, size_t first_leaf, size_t count, uint64_t *out_host) try {
  CHECK_BATCH(b);
  cp_ctx *ctx = b->ctx;
  CHECK_CTX(ctx);
  if (count == 0) return CP_OK;
  if (!out_host) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  const size_t N = (size_t)1 << (b->degree_bits + b->rate_bits), w = b->k + (size_t)b->n_salt;
  if (first_leaf >= N || count > N - first_leaf) return set_error(ctx, CP_ERR_INVALID_ARG, "leaves [%zu, %zu) out of range", first_leaf, first_leaf + count);
  if (count * w > ((size_t)1 << 31)) return set_error(ctx, CP_ERR_INVALID_ARG, "more than 2^31 values per call: fetch in slices");
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);
  uint64_t *d_out = nullptr;
  CP_TRY(arena_alloc(ctx, count * w * 8, (void **)&d_out));
  LAUNCH(ctx, "batch_leaves", k_leaves, dim3(blocks_for(count * w, 256)), dim3(256), b->lde, b->salt, N, b->k, b->n_salt, first_leaf, count, d_out);
  return cp_d2h(ctx, out_host, d_out, count * w * 8);
} CP_CATCH(b ? b->ctx : nullptr)

int cp_fri_prove(cp_ctx *ctx, cp_poly_batch *const *oracles, size_t n_oracles, const cp_fri_batch *batches, size_t n_batches,
                 const cp_fri_params *params, cp_challenger_state *challenger, int use_pow_override, uint64_t pow_override,
                 uint8_t **fri_proof_out, size_t *fri_proof_len) try {
  CHECK_CTX(ctx);
  if (!oracles || !batches || !params || !challenger || !fri_proof_out || !fri_proof_len) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  *fri_proof_out = nullptr;
  *fri_proof_len = 0;
  if (n_oracles < 1 || n_oracles > (size_t)fri::MAX_ORACLES) return set_error(ctx, CP_ERR_UNSUPPORTED, "1..%d oracles per FRI instance", fri::MAX_ORACLES);
  if (n_batches < 1 || n_batches > 64) return set_error(ctx, CP_ERR_INVALID_ARG, "1..64 opening batches");
  FriCfg cfg;
  CP_TRY(load_fri_cfg(ctx, params, cfg));
  if (const char *why = challenger_problem(challenger)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s", why);
  if (use_pow_override && pow_override >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "pow witness is not canonical");
  const int db = params->degree_bits;
  const size_t n = (size_t)1 << db;
  std::vector<OracleRef> refs(n_oracles);
  for (size_t o = 0; o < n_oracles; o++) {
    const cp_poly_batch *b = oracles[o];
    if (!b) return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu is NULL", o);
    if (!b->ctx) return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu: the context of this batch was destroyed", o);
    if (!(b->ctx == ctx || (ctx->parent && b->ctx == ctx->parent))) return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu belongs to another context", o);
    if (b->degree_bits != db || b->rate_bits != cfg.rate_bits || b->cap_height != cfg.cap_height)
      return set_error(ctx, CP_ERR_INVALID_ARG, "oracle %zu: degree_bits %d / rate_bits %d / cap_height %d differ from the FriParams (%d / %d / %d)", o,
                       b->degree_bits, b->rate_bits, b->cap_height, db, cfg.rate_bits, cfg.cap_height);
    OracleRef &R = refs[o];
    R.k = b->k;
    R.coeffs = b->coeffs; R.lde = b->lde; R.digests = b->digests;
    R.salt = b->salt; R.n_salt = b->n_salt;
  }
  std::vector<FriBatchDesc> descs(n_batches);
  std::vector<gl::Ext> pts(2 * n_batches);  // points, then their inverses
  for (size_t i = 0; i < n_batches; i++) {
    const cp_fri_batch &fb = batches[i];
    if (fb.n_ranges && !fb.ranges) return set_error(ctx, CP_ERR_INVALID_ARG, "batch %zu: ranges are NULL", i);
    if (fb.point[0] >= gl::P || fb.point[1] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "batch %zu: point is not canonical", i);
    const gl::Ext z{fb.point[0], fb.point[1]};
    // a point of the LDE coset would make (X - z) vanish on the evaluation domain; plonky2's verifier divides by it
    if (z.b == 0 && gl::pow(gl::mul(z.a, gl::inv(7)), (uint64_t)1 << (db + cfg.rate_bits)) == 1 && z.a != 0)
      return set_error(ctx, CP_ERR_INVALID_ARG, "batch %zu: the opening point lies on the LDE coset", i);
    if (z.a == 0 && z.b == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "batch %zu: the opening point is zero", i);
    for (size_t r = 0; r < fb.n_ranges; r++) {
      const cp_fri_poly_range &R = fb.ranges[r];
      if (R.oracle >= n_oracles || R.first > refs[R.oracle].k || R.count > refs[R.oracle].k - R.first)
        return set_error(ctx, CP_ERR_INVALID_ARG, "batch %zu, range %zu: polynomials [%u, %u) of oracle %u out of range", i, r, R.first, R.first + R.count, R.oracle);
      if (R.count == 0) continue;
      descs[i].ranges.push_back(R);
      descs[i].n_polys += R.count;
    }
    if (descs[i].n_polys > ((size_t)1 << 24)) return set_error(ctx, CP_ERR_INVALID_ARG, "batch %zu: too many polynomials", i);
    pts[i] = z;
    pts[n_batches + i] = host_ext_inv(z);
  }
  // plonky2's output buffer is the squeezed block itself — a prefix of the sponge state: anything else is not a state its
  // Challenger can be in (and the device form of the transcript keeps only the count)
  for (uint32_t i = 0; i < challenger->n_output; i++)
    if (challenger->output_buffer[i] != challenger->sponge_state[i])
      return set_error(ctx, CP_ERR_INVALID_ARG, "challenger: output_buffer is not the squeezed prefix of the sponge state");
  HostChallenger C;
  challenger_load(C, *challenger);
  tr::DevCh hch;
  ByteBuf bytes;
  {
    ArenaScope arena_scope(ctx);
    host_phase(ctx, "setup");
    gl::Ext *d_pts, *zpow;
    unsigned *d_flags;
    Transcript T;
    CP_TRY(arena_alloc(ctx, pts.size() * 16, (void **)&d_pts));
    CP_TRY(arena_alloc(ctx, pts.size() * n * 16, (void **)&zpow));
    CP_TRY(arena_alloc(ctx, sizeof(unsigned), (void **)&d_flags));
    CP_TRY(push(ctx, d_pts, pts.data(), pts.size() * 16));
    CP_TRY(T.init_from(ctx, C));
    HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, sizeof(unsigned), ctx->stream));
    LAUNCH(ctx, "fri_ext_powers", fri::k_ext_powers, dim3(blocks_for(n, 256), (unsigned)pts.size()), dim3(256), d_pts, n, zpow);
    const int up = use_pow_override ? 1 : 0;
    FriHostOut fo;
    CP_TRY(fri_prove_impl(ctx, 1, db, cfg, refs, descs, zpow, zpow + n_batches * n, T, tr::Seg{nullptr, nullptr, 0, 0}, &up, &pow_override,
                          d_flags, fo));
    if (T.device) CP_TRY(fetch_async(ctx, &hch, T.d_ch, sizeof hch));
    host_phase(ctx, "drain");
    CP_TRY(fetch_flush(ctx));
    CP_TRY(fo.check(ctx));
    host_phase(ctx, "copy_out");
    fo.bytes(0, bytes);
    if (!T.device) hch = Transcript::pack(T.C[0]);
  }
  host_phase(ctx, nullptr);
  uint8_t *buf = (uint8_t *)malloc(bytes.v.size() ? bytes.v.size() : 1);
  if (!buf) return set_error(ctx, CP_ERR_OOM, "out of host memory");
  memcpy(buf, bytes.v.data(), bytes.v.size());
  *fri_proof_out = buf;
  *fri_proof_len = bytes.v.size();
  memcpy(challenger->sponge_state, hch.state, sizeof hch.state);
  memset(challenger->input_buffer, 0, sizeof challenger->input_buffer);
  memset(challenger->output_buffer, 0, sizeof challenger->output_buffer);
  memcpy(challenger->input_buffer, hch.in, (size_t)hch.n_in * 8);
  memcpy(challenger->output_buffer, hch.state, (size_t)hch.n_out * 8);
  challenger->n_input = (uint32_t)hch.n_in;
  challenger->n_output = (uint32_t)hch.n_out;
  return CP_OK;
} CP_CATCH(ctx)

int cp_fri_verify(const cp_fri_params *params, const cp_fri_oracle_info *oracles, size_t n_oracles, const uint64_t *const *oracle_caps,
                  const cp_fri_batch *batches, size_t n_batches, const uint64_t *const *opened_values, cp_challenger_state *challenger,
                  const uint8_t *fri_proof, size_t fri_proof_len) try {
  if (!params || !oracles || !oracle_caps || !batches || !opened_values || !challenger || !fri_proof) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  if (n_oracles < 1 || n_oracles > (size_t)fri::MAX_ORACLES) return set_error(nullptr, CP_ERR_UNSUPPORTED, "1..%d oracles per FRI instance", fri::MAX_ORACLES);
  if (n_batches < 1 || n_batches > 64) return set_error(nullptr, CP_ERR_INVALID_ARG, "1..64 opening batches");
  FriVerifyInstance I;
  CP_TRY(load_fri_cfg(nullptr, params, I.cfg));
  if (const char *why = challenger_problem(challenger)) return set_error(nullptr, CP_ERR_INVALID_ARG, "%s", why);
  I.db = params->degree_bits;
  I.n_oracles = (int)n_oracles;
  const size_t cap_n = (size_t)1 << I.cfg.cap_height;
  for (size_t o = 0; o < n_oracles; o++) {
    if (oracles[o].num_polys == 0 || oracles[o].num_polys > 65535) return set_error(nullptr, CP_ERR_INVALID_ARG, "oracle %zu: num_polys out of range", o);
    if (!oracle_caps[o]) return set_error(nullptr, CP_ERR_INVALID_ARG, "cap of oracle %zu is NULL", o);
    for (size_t i = 0; i < cap_n * 4; i++)
      if (oracle_caps[o][i] >= gl::P) return set_error(nullptr, CP_ERR_INVALID_ARG, "cap of oracle %zu: element %zu is not canonical", o, i);
    I.kk[o] = oracles[o].num_polys;
    I.leaf_len[o] = I.kk[o] + (oracles[o].blinding ? CP_SALT_SIZE : 0);
    I.caps[o] = oracle_caps[o];
  }
  I.points.resize(n_batches);
  I.ranges.assign(n_batches, {});
  I.opened.assign(n_batches, {});
  for (size_t i = 0; i < n_batches; i++) {
    const cp_fri_batch &fb = batches[i];
    if (fb.n_ranges && !fb.ranges) return set_error(nullptr, CP_ERR_INVALID_ARG, "batch %zu: ranges are NULL", i);
    if (fb.point[0] >= gl::P || fb.point[1] >= gl::P) return set_error(nullptr, CP_ERR_INVALID_ARG, "batch %zu: point is not canonical", i);
    I.points[i] = gl::Ext{fb.point[0], fb.point[1]};
    size_t cnt = 0;
    for (size_t r = 0; r < fb.n_ranges; r++) {
      const cp_fri_poly_range &R = fb.ranges[r];
      if (R.oracle >= n_oracles || R.first > I.kk[R.oracle] || R.count > I.kk[R.oracle] - R.first)
        return set_error(nullptr, CP_ERR_INVALID_ARG, "batch %zu, range %zu out of range", i, r);
      if (R.count == 0) continue;
      I.ranges[i].push_back(R);
      cnt += R.count;
    }
    if (cnt && !opened_values[i]) return set_error(nullptr, CP_ERR_INVALID_ARG, "batch %zu: opened values are NULL", i);
    I.opened[i].resize(cnt);
    for (size_t j = 0; j < cnt; j++) {
      if (opened_values[i][2 * j] >= gl::P || opened_values[i][2 * j + 1] >= gl::P)
        return set_error(nullptr, CP_ERR_VERIFY, "batch %zu: opened value %zu is not canonical", i, j);
      I.opened[i][j] = gl::Ext{opened_values[i][2 * j], opened_values[i][2 * j + 1]};
    }
  }
  Rd r{fri_proof, fri_proof_len};
  ParsedFri pf;
  CP_TRY(parse_fri_proof(nullptr, I, r, pf));
  if (r.o != fri_proof_len) return set_error(nullptr, CP_ERR_VERIFY, "malformed proof: length");
  if (r.noncanonical) return set_error(nullptr, CP_ERR_VERIFY, "a field element of the proof is not canonical (>= p)");
  hostu::alloc_checkpoint();
  HostChallenger C;
  challenger_load(C, *challenger);
  gl::Ext alpha;
  std::vector<gl::Ext> fbetas;
  std::vector<uint64_t> x_indices;
  CP_TRY(fri_challenges(nullptr, C, I, pf, alpha, fbetas, x_indices));
  CP_TRY(verify_fri_queries(nullptr, I, fri_proof, fri_proof_len, pf, alpha, fbetas.data(), x_indices.data()));
  challenger_store(C, *challenger);
  return CP_OK;
} CP_CATCH(nullptr)

int cp_challenger_observe(cp_challenger_state *challenger, const uint64_t *elements, size_t count) try {
  if (const char *why = challenger_problem(challenger)) return set_error(nullptr, CP_ERR_INVALID_ARG, "%s", why);
  if (count && !elements) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  for (size_t i = 0; i < count; i++)
    if (elements[i] >= gl::P) return set_error(nullptr, CP_ERR_INVALID_ARG, "element %zu is not canonical", i);
  HostChallenger C;
  challenger_load(C, *challenger);
  C.observe(elements, count);
  challenger_store(C, *challenger);
  return CP_OK;
} CP_CATCH(nullptr)

int cp_challenger_challenges(cp_challenger_state *challenger, uint64_t *out, size_t count) try {
  if (const char *why = challenger_problem(challenger)) return set_error(nullptr, CP_ERR_INVALID_ARG, "%s", why);
  if (count && !out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  HostChallenger C;
  challenger_load(C, *challenger);
  for (size_t i = 0; i < count; i++) out[i] = C.challenge();
  challenger_store(C, *challenger);
  return CP_OK;
} CP_CATCH(nullptr)

}  // extern "C"
