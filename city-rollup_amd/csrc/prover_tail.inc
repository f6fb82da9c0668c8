// Host orchestration of the tail of CircuitData::prove (included at the end of cityprover.hip).
// A call proves B independent proofs of one shape: every device step is one launch over the whole
// batch, and every Fiat-Shamir step advances B host challengers. The transcript runs on the host — it
// is a strictly sequential chain of ~60 permutations per proof — with the same __host__ __device__
// Poseidon the kernels use; everything proportional to the trace runs on the device.

namespace {

struct HostChallenger {
  uint64_t state[12] = {0};
  uint64_t in[8];
  int n_in = 0;
  uint64_t out[8];
  int n_out = 0;
  void duplex() {
    for (int i = 0; i < n_in; i++) state[i] = in[i];
    n_in = 0;
    poseidon::permute_host(state);
    memcpy(out, state, sizeof out);
    n_out = 8;
  }
  void observe(const uint64_t *e, size_t n) {
    for (size_t i = 0; i < n; i++) {
      n_out = 0;
      in[n_in++] = e[i];
      if (n_in == 8) duplex();
    }
  }
  uint64_t challenge() {
    if (n_in > 0 || n_out == 0) duplex();
    return out[--n_out];
  }
  gl::Ext ext_challenge() {
    uint64_t a = challenge(), b = challenge();
    return gl::Ext{a, b};
  }
};

gl::Ext host_ext_pow(gl::Ext b, uint64_t e) {
  gl::Ext r{1, 0};
  while (e) {
    if (e & 1) r = gl::ext_mul(r, b);
    b = gl::ext_mul(b, b);
    e >>= 1;
  }
  return r;
}
gl::Ext host_ext_inv(gl::Ext x) {
  // 1/(a + bX) = (a - bX) / (a^2 - 7 b^2)
  uint64_t n = gl::sub(gl::mul(x.a, x.a), gl::mul(7, gl::mul(x.b, x.b)));
  uint64_t ni = gl::inv(n);
  return gl::Ext{gl::mul(x.a, ni), gl::mul(gl::neg(x.b), ni)};
}

// one oracle of B proofs: [proof][k][...] with fixed per-proof strides
struct DevBatch {
  size_t k = 0;
  uint64_t *coeffs = nullptr, *lde = nullptr, *digests = nullptr, *cap = nullptr;
  size_t coeffs_stride = 0, lde_stride = 0, dig_stride = 0;  // per proof, in u64
  const uint64_t *salt = nullptr;  // zero-knowledge: [proof][CP_SALT_SIZE][N] extra leaf elements (leaf order), else null
  size_t salt_stride = 0;
  int n_salt = 0;
  std::vector<uint64_t> cap_host;                            // B x 2^cap_height x 4
};

// Per-context workspace arena: per-proof device buffers are bump-allocated from chunks that survive
// between calls, so the steady-state proving path performs no hipMalloc / hipFree (both serialise the
// whole device).
int arena_alloc(cp_ctx *ctx, size_t bytes, void **out) {
  bytes = (bytes + 255) & ~(size_t)255;
  auto &A = ctx->arena;
  while (A.cur < A.chunks.size()) {
    if (A.off + bytes <= A.chunks[A.cur].bytes()) {
      *out = A.chunks[A.cur].get<char>() + A.off;
      A.off += bytes;
      A.used += bytes;
      return CP_OK;
    }
    A.cur++;
    A.off = 0;
  }
  size_t sz = bytes > ((size_t)64 << 20) ? bytes : ((size_t)64 << 20);
  A.chunks.reserve(A.chunks.size() + 1);
  DevBuf chunk = ctx->buf();
  CP_TRY(alloc_status(ctx, chunk.alloc(sz), sz));
  *out = chunk.get();
  A.chunks.push_back(std::move(chunk));
  A.cur = A.chunks.size() - 1;
  A.off = bytes;
  A.used += bytes;
  return CP_OK;
}
// called with the stream idle: rewind; if the call spilled over several chunks, coalesce them into one
void arena_reset(cp_ctx *ctx) {
  auto &A = ctx->arena;
  if (A.chunks.size() > 1) {
    size_t total = 0;
    for (auto &c : A.chunks) total += c.bytes();
    A.chunks.resize(1);  // frees the others first
    if (A.chunks[0].alloc(total) != 0) A.chunks.clear();  // refused: the arena is empty and grows again
  }
  A.cur = 0;
  A.off = 0;
  A.used = 0;
}

// the arrays of `b` live in `mem` (the handle that holds b), not in the arena
int batch_alloc_persistent(cp_ctx *ctx, DevBag &mem, DevBatch &b, size_t k, size_t n, size_t N, int cap_height) {
  b.k = k;
  const size_t dig = merkle_words_per_tree(N, cap_height) * 8, cap = ((size_t)4 << cap_height) * 8;
  CP_TRY(alloc_status(ctx, mem.alloc(&b.coeffs, k * n * 8), k * n * 8));
  CP_TRY(alloc_status(ctx, mem.alloc(&b.lde, k * N * 8), k * N * 8));
  CP_TRY(alloc_status(ctx, mem.alloc(&b.digests, dig), dig));
  return alloc_status(ctx, mem.alloc(&b.cap, cap), cap);
}
int batch_alloc(cp_ctx *ctx, DevBatch &b, size_t Bn, size_t k, size_t n, size_t N, int cap_height) {
  b.k = k;
  b.coeffs_stride = k * n;
  b.lde_stride = k * N;
  b.dig_stride = merkle_words_per_tree(N, cap_height);
  CP_TRY(arena_alloc(ctx, Bn * b.coeffs_stride * 8, (void **)&b.coeffs));
  CP_TRY(arena_alloc(ctx, Bn * b.lde_stride * 8, (void **)&b.lde));
  CP_TRY(arena_alloc(ctx, Bn * b.dig_stride * 8, (void **)&b.digests));
  CP_TRY(arena_alloc(ctx, Bn * ((size_t)4 << cap_height) * 8, (void **)&b.cap));
  return CP_OK;
}
// hands every enqueued device-to-host copy to its destination (one stream synchronisation) and recycles the staging area
int fetch_flush(cp_ctx *ctx) {
  HIP_TRY(ctx, sync_stream(ctx));
  for (const auto &f : ctx->pending_fetches) memcpy(f.host, f.stage, f.bytes);
  ctx->pending_fetches.clear();
  ctx->pin_off = 0;  // stream drained: every staged transfer is done
  return CP_OK;
}
// page-locked staging area: at least `bytes` free, 64-byte aligned slots; the area is recycled at every flush
int pin_reserve(cp_ctx *ctx, size_t bytes, char **out) {
  bytes = (bytes + 63) & ~(size_t)63;
  if (ctx->pin_off + bytes > ctx->pin.bytes()) {
    CP_TRY(fetch_flush(ctx));  // everything staged so far has been consumed / delivered
    if (bytes > ctx->pin.bytes()) {
      const size_t want = bytes < ((size_t)8 << 20) ? ((size_t)8 << 20) : bytes * 2;
      CP_TRY(alloc_status(ctx, ctx->pin.grow(want), want));
    }
  }
  *out = ctx->pin.get<char>() + ctx->pin_off;
  ctx->pin_off += bytes;
  return CP_OK;
}
// enqueue a device-to-host copy; `host` is filled by the next fetch_flush (it must stay valid until then)
int fetch_async(cp_ctx *ctx, void *host, const void *dev, size_t bytes) {
  if (bytes == 0) return CP_OK;
  char *st;
  CP_TRY(pin_reserve(ctx, bytes, &st));
  HIP_TRY(ctx, hipMemcpyAsync(st, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ctx->pending_fetches.push_back({host, st, bytes});
  return CP_OK;
}
int fetch(cp_ctx *ctx, void *host, const void *dev, size_t bytes) {
  if (bytes == 0) return CP_OK;
  CP_TRY(fetch_async(ctx, host, dev, bytes));
  return fetch_flush(ctx);
}
int push(cp_ctx *ctx, void *dev, const void *host, size_t bytes) {
  if (bytes == 0) return CP_OK;
  char *st;
  CP_TRY(pin_reserve(ctx, bytes, &st));
  memcpy(st, host, bytes);  // `host` may be reused as soon as this returns
  HIP_TRY(ctx, hipMemcpyAsync(dev, st, bytes, hipMemcpyHostToDevice, ctx->stream));
  return CP_OK;
}
int batch_fetch_caps(cp_ctx *ctx, DevBatch &b, size_t Bn, int cap_height) {
  b.cap_host.resize(Bn * ((size_t)4 << cap_height));
  return fetch(ctx, b.cap_host.data(), b.cap, b.cap_host.size() * 8);
}

struct ByteBuf {
  std::vector<uint8_t> v;
  void u64(uint64_t x) { const uint8_t *p = (const uint8_t *)&x; v.insert(v.end(), p, p + 8); }
  void felts(const uint64_t *x, size_t n) { const uint8_t *p = (const uint8_t *)x; v.insert(v.end(), p, p + 8 * n); }
};

int ilog2(size_t x) { int l = 0; while (((size_t)1 << l) < x) l++; return l; }

// leaves (x batch) up to which the FRI layer leaves are hashed twelve lanes per leaf; CITYPROVER_COOP_MAX overrides (0 = never)
size_t coop_leaf_max(cp_ctx *ctx) {
  long v = -1;
  if (ctx_option(ctx, "COOP_FRI_MAX", v)) return (size_t)v;
  if (ctx_option(ctx, "COOP_MAX", v)) return (size_t)v / 2;
  static const size_t env = getenv("CITYPROVER_COOP_FRI_MAX") ? strtoull(getenv("CITYPROVER_COOP_FRI_MAX"), nullptr, 10)
                            : getenv("CITYPROVER_COOP_MAX") ? strtoull(getenv("CITYPROVER_COOP_MAX"), nullptr, 10) / 2 : 16384;
  return env;
}

}  // namespace

#include "fri_engine.inc"

// Every range a cp_shape must satisfy — shared by cp_circuit_load and the circuit-file reader (cp_circuit_file_info is
// the validator that needs no GPU: it must refuse exactly what the loader would refuse).
static const char *shape_problem(const cp_shape &sh) {
  if (sh.degree_bits < 2 || sh.degree_bits + sh.rate_bits > 30 || sh.rate_bits < 0 || sh.num_challenges < 1 || sh.num_challenges > 8 ||
      sh.num_wires < 1 || sh.num_wires > 65535 || sh.num_constants < 0 || sh.num_constants > 4096 || sh.num_routed_wires < 0 ||
      sh.num_routed_wires > 4096 || sh.num_routed_wires > sh.num_wires || sh.num_partial_products < 0 || sh.num_partial_products > 4096 ||
      sh.quotient_degree_factor < 1 || sh.quotient_degree_factor > 64 || (sh.zero_knowledge != 0 && sh.zero_knowledge != 1) ||
      sh.num_public_inputs < 0 || sh.num_public_inputs > (1 << 20))
    return "circuit shape out of range";
  FriCfg c;
  c.rate_bits = sh.rate_bits; c.cap_height = sh.cap_height; c.pow_bits = sh.pow_bits; c.num_query_rounds = sh.num_query_rounds;
  c.n_arity = sh.n_arity;
  if (c.n_arity < 0 || c.n_arity > 8) return "0..8 FRI reduction layers";
  for (int l = 0; l < 8; l++) c.arity_bits[l] = sh.arity_bits[l];
  return fri_cfg_problem(sh.degree_bits, c);
}

struct cp_circuit {
  cp_ctx *ctx = nullptr;
  cp_shape sh;
  uint64_t digest[4];
  explicit cp_circuit(cp_ctx *c) : ctx(c), mem(c->bag()) {}
  DevBag mem;   // owns what cs, cs_values and k_is point to; waits for the context's stream before it frees
  DevBatch cs;  // constants + sigmas commitment (device resident for the circuit's lifetime)
  uint64_t *cs_values = nullptr;  // the same polynomials as VALUES over <omega_n> (sigma rows feed the Z computation)
  uint64_t *k_is = nullptr;       // num_routed_wires coset shifts
  std::vector<quot::Gate> gates;  // CommonCircuitData::gates with their selector groups (cp_circuit_set_gates)
  int num_selectors = 0;
  bool has_gates = false;
  std::vector<uint32_t> pi_targets;  // (row, wire) of every public input in the wire matrix; empty = not known
};

// a circuit may be used by the context that loaded it and by that context's lanes (its device data is read-only)
static bool owns(const cp_ctx *ctx, const cp_circuit *c) { return c->ctx == ctx || (ctx->parent && c->ctx == ctx->parent); }
// "one batch = one shape": everything but the number of public inputs (which only enters the transcript per proof)
static bool same_shape(const cp_shape &a, const cp_shape &b) {
  cp_shape x = a, y = b;
  x.num_public_inputs = y.num_public_inputs = 0;
  return memcmp(&x, &y, sizeof(cp_shape)) == 0;
}
// the grid's y / z dimensions carry polynomials and proofs: at most 65535 each
static size_t max_batch(const cp_shape &sh) {
  size_t k = (size_t)sh.num_wires;
  const size_t kz = (size_t)sh.num_challenges * (1 + sh.num_partial_products), kq = (size_t)sh.num_challenges * sh.quotient_degree_factor;
  if (kz > k) k = kz;
  if (kq > k) k = kq;
  size_t m = 65535 / (k ? k : 1);
  return m > 4096 ? 4096 : m;
}
// rewinds the context's arena when the scope ends, whichever way it ends (the stream is drained first)
struct ArenaScope {
  cp_ctx *ctx;
  bool armed;
  explicit ArenaScope(cp_ctx *c, bool a = true) : ctx(c), armed(a) {}
  ~ArenaScope() {
    if (!armed) return;
    (void)sync_stream(ctx);
    ctx->pending_fetches.clear();  // an early exit leaves copies nobody waits for: their destinations may be gone
    ctx->pin_off = 0;
    arena_reset(ctx);
  }
};

// A7 launch on device-resident parameters: d_sig = per-proof sigma-values pointers; betas[proof*stride + c], gammas likewise
static int zs_launch(cp_ctx *ctx, const cp_shape &sh, size_t Bn, const uint64_t *const *d_sig, const uint64_t *k_is,
                     const uint64_t *wires, const uint64_t *betas, const uint64_t *gammas, size_t chal_stride, uint64_t *out) {
  const int nc = sh.num_challenges, R = sh.num_routed_wires, chunk = sh.quotient_degree_factor, npp = sh.num_partial_products;
  if (R <= 0 || (R + chunk - 1) / chunk != npp + 1 || npp + 1 > zs::MAX_CHUNKS)
    return set_error(ctx, CP_ERR_INVALID_ARG, "num_partial_products %d inconsistent with %d routed wires in chunks of %d", npp, R, chunk);
  const size_t n = (size_t)1 << sh.degree_bits;
  const uint64_t *wt;
  CP_TRY(get_pow_table(ctx, GL_ROOTS[sh.degree_bits], &wt));
  zs::Args a;
  a.wires = wires;
  a.wires_proof_stride = (size_t)sh.num_wires * n;
  a.sigmas = d_sig;
  a.k_is = k_is;
  a.betas = betas;
  a.gammas = gammas;
  a.chal_stride = chal_stride;
  a.out = out;
  a.out_proof_stride = (size_t)nc * (1 + npp) * n;
  a.omega_tab = wt;
  a.n = n;
  a.num_routed = R; a.chunk = chunk; a.npp = npp; a.nc = nc;
  if (a.npp + 1 <= 10) LAUNCH(ctx, "zs_chunk_products", zs::k_chunk_products<10>, dim3(blocks_for(n, 256), nc, (unsigned)Bn), dim3(256), a);
  else LAUNCH(ctx, "zs_chunk_products", zs::k_chunk_products<zs::MAX_CHUNKS>, dim3(blocks_for(n, 256), nc, (unsigned)Bn), dim3(256), a);
  LAUNCH(ctx, "zs_scan_rows", zs::k_scan_rows, dim3(1, nc, (unsigned)Bn), dim3(256), a);
  return CP_OK;
}

extern "C" {

void cp_free(void *p) { free(p); }

cp_circuit *cp_circuit_load(cp_ctx *ctx, const cp_shape *sh, const uint64_t circuit_digest[4],
                            const uint64_t *cs_values_host, const uint64_t *k_is_host) try {
  if (!ctx || !sh || !circuit_digest || !cs_values_host) {
    set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
    return nullptr;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  if (const char *why = shape_problem(*sh)) {
    set_error(ctx, CP_ERR_INVALID_ARG, "%s", why);
    return nullptr;
  }
  std::unique_ptr<cp_circuit> c(new (std::nothrow) cp_circuit(ctx));
  if (!c) { set_error(ctx, CP_ERR_OOM, "out of host memory"); return nullptr; }
  c->sh = *sh;
  memcpy(c->digest, circuit_digest, 32);
  const int rc = [&]() -> int {
    size_t n = (size_t)1 << sh->degree_bits, N = n << sh->rate_bits;
    size_t k = (size_t)sh->num_constants + sh->num_routed_wires;
    CP_TRY(batch_alloc_persistent(ctx, c->mem, c->cs, k, n, N, sh->cap_height));
    CP_TRY(alloc_status(ctx, c->mem.alloc(&c->cs_values, k * n * 8), k * n * 8));
    CP_TRY(cp_h2d(ctx, c->cs_values, cs_values_host, k * n * 8));
    CP_TRY(cp_commit_dev(ctx, c->cs_values, k, sh->degree_bits, sh->rate_bits, sh->cap_height, c->cs.coeffs, c->cs.lde, c->cs.digests, c->cs.cap));
    CP_TRY(batch_fetch_caps(ctx, c->cs, 1, sh->cap_height));
    if (sh->num_routed_wires <= 0) return CP_OK;
    // coset shifts k_i of the routed wires (CommonCircuitData::k_is); plonky2's own choice is 7^i
    std::vector<uint64_t> ks(sh->num_routed_wires);
    uint64_t acc = 1;
    for (int i = 0; i < sh->num_routed_wires; i++) {
      ks[i] = k_is_host ? k_is_host[i] : acc;
      if (ks[i] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "k_is[%d] is not canonical", i);
      acc = gl::mul(acc, 7);
    }
    CP_TRY(alloc_status(ctx, c->mem.alloc(&c->k_is, ks.size() * 8), ks.size() * 8));
    return cp_h2d(ctx, c->k_is, ks.data(), ks.size() * 8);
  }();
  return rc == CP_OK ? c.release() : nullptr;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

void cp_circuit_destroy(cp_circuit *c) {
  if (!c) return;
  (void)hipSetDevice(c->ctx->device);
  delete c;  // c->mem waits for the context's stream, then frees
}

// A7: Z / partial products for n_proofs proofs (same shape); betas, gammas: [proof][num_challenges] (host)
int cp_zs_partial_products_dev(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *wires_values_dev,
                               const uint64_t *betas_host, const uint64_t *gammas_host, uint64_t *out_dev) try {
  CHECK_CTX(ctx);
  if (n_proofs == 0) return CP_OK;
  if (!circuits || !wires_values_dev || !betas_host || !gammas_host || !out_dev)
    return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (n_proofs > 65535) return set_error(ctx, CP_ERR_INVALID_ARG, "too many proofs");
  for (size_t p = 0; p < n_proofs; p++) {
    if (!circuits[p] || !owns(ctx, circuits[p])) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit %zu invalid", p);
    if (!same_shape(circuits[p]->sh, circuits[0]->sh))
      return set_error(ctx, CP_ERR_INVALID_ARG, "circuit %zu has a different shape", p);
  }
  const cp_shape &sh = circuits[0]->sh;
  const int nc = sh.num_challenges, R = sh.num_routed_wires, chunk = sh.quotient_degree_factor, npp = sh.num_partial_products;
  if (R <= 0 || (R + chunk - 1) / chunk != npp + 1 || npp + 1 > zs::MAX_CHUNKS)
    return set_error(ctx, CP_ERR_INVALID_ARG, "num_partial_products %d inconsistent with %d routed wires in chunks of %d", npp, R, chunk);
  for (size_t i = 0; i < n_proofs * (size_t)nc; i++)
    if (betas_host[i] >= gl::P || gammas_host[i] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "challenge %zu is not canonical", i);
  const size_t n = (size_t)1 << sh.degree_bits;
  const uint64_t **d_sig;
  uint64_t *d_bg;
  // small per-call parameter block in the arena (released by the caller's arena_reset or below)
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);  // every exit path rewinds the arena this call opened
  CP_TRY(arena_alloc(ctx, n_proofs * sizeof(void *), (void **)&d_sig));
  CP_TRY(arena_alloc(ctx, 2 * n_proofs * nc * 8, (void **)&d_bg));
  {
    std::vector<const uint64_t *> h(n_proofs);
    for (size_t p = 0; p < n_proofs; p++) h[p] = circuits[p]->cs_values + (size_t)sh.num_constants * n;
    std::vector<uint64_t> bg(2 * n_proofs * nc);
    memcpy(bg.data(), betas_host, n_proofs * nc * 8);
    memcpy(bg.data() + n_proofs * nc, gammas_host, n_proofs * nc * 8);
    CP_TRY(push(ctx, d_sig, h.data(), n_proofs * sizeof(void *)));
    CP_TRY(push(ctx, d_bg, bg.data(), bg.size() * 8));
  }
  return zs_launch(ctx, sh, n_proofs, d_sig, circuits[0]->k_is, wires_values_dev, d_bg, d_bg + n_proofs * nc, (size_t)nc, out_dev);
} CP_CATCH(ctx)

int cp_circuit_cs_cap(cp_circuit *c, uint64_t *cap_out) try {
  if (!c || !cap_out) return set_error(c ? c->ctx : nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  memcpy(cap_out, c->cs.cap_host.data(), c->cs.cap_host.size() * 8);
  return CP_OK;
} CP_CATCH(c ? c->ctx : nullptr)

// sizes of one proof of a shape: rows, LDE points, cap digests, polynomials per oracle (constants + sigmas, wires, Z / partial
// products, quotient chunks) and in all, opened values per proof (every polynomial at zeta, then the Z polynomials at g*zeta)
struct TailDims {
  size_t n, N, cap_n, k_cs, k_w, k_z, k_q, k_all, open_stride;
  explicit TailDims(const cp_shape &sh)
      : n((size_t)1 << sh.degree_bits), N(n << sh.rate_bits), cap_n((size_t)1 << sh.cap_height),
        k_cs((size_t)sh.num_constants + sh.num_routed_wires), k_w(sh.num_wires), k_z((size_t)sh.num_challenges * (1 + sh.num_partial_products)),
        k_q((size_t)sh.num_challenges * sh.quotient_degree_factor), k_all(k_cs + k_w + k_z + k_q), open_stride(k_all + sh.num_challenges) {}
};
// per-proof device tables of a call: oracle 0 (coeffs / lde / digests of each proof's circuit), the sigma-values table of A7, the
// transcript head and the error flags
struct TailTables {
  const uint64_t **t_coeffs, **t_lde, **t_dig, **d_sig;
  uint64_t *d_head;   // [proof][circuit_digest (4) | public_inputs_hash (4)]
  unsigned *d_flags;
};

static int tail_setup(cp_ctx *ctx, size_t Bn, cp_circuit *const *circs, const uint64_t *const *pis, const size_t *n_pis, const TailDims &D,
                      Transcript &T, TailTables &t) {
  const cp_shape &sh = circs[0]->sh;
  {
    std::vector<const uint64_t *> h(4 * Bn);
    for (size_t p = 0; p < Bn; p++) {
      h[p] = circs[p]->cs.coeffs; h[Bn + p] = circs[p]->cs.lde; h[2 * Bn + p] = circs[p]->cs.digests;
      h[3 * Bn + p] = circs[p]->cs_values + (size_t)sh.num_constants * D.n;
    }
    CP_TRY(arena_alloc(ctx, 4 * Bn * sizeof(void *), (void **)&t.t_coeffs));
    t.t_lde = t.t_coeffs + Bn;
    t.t_dig = t.t_coeffs + 2 * Bn;
    t.d_sig = t.t_coeffs + 3 * Bn;
    CP_TRY(push(ctx, t.t_coeffs, h.data(), 4 * Bn * sizeof(void *)));
  }
  // transcripts: zero state; head = circuit_digest || public_inputs_hash per proof (the hash of the public inputs is a
  // sponge of its own over host data: computed here, it needs nothing from the device)
  std::vector<uint64_t> head(8 * Bn);
  CP_TRY(T.init(ctx, Bn));
  CP_TRY(arena_alloc(ctx, Bn * 64, (void **)&t.d_head));
  CP_TRY(arena_alloc(ctx, Bn * sizeof(unsigned), (void **)&t.d_flags));
  HIP_TRY(ctx, hipMemsetAsync(t.d_flags, 0, Bn * sizeof(unsigned), ctx->stream));
  host_for(Bn, [&](size_t p) {
    uint64_t st[12] = {0};
    for (size_t off = 0; off < n_pis[p]; off += 8) {
      size_t c = n_pis[p] - off < 8 ? n_pis[p] - off : 8;
      memcpy(st, pis[p] + off, c * 8);
      poseidon::permute_host(st);
    }
    memcpy(&head[8 * p], circs[p]->digest, 32);
    memcpy(&head[8 * p + 4], st, 32);  // public_inputs_hash
  });
  return push(ctx, t.d_head, head.data(), head.size() * 8);
}

// every polynomial of the four oracles at zeta and the Z polynomials at g*zeta: d_open [proof][open_stride], copied to `open`
// behind the kernels; zpow = powers of the two points and (second half) of their inverses, for FRI
static int tail_openings(cp_ctx *ctx, size_t Bn, int nc, const TailDims &D, const TailTables &t, const DevBatch *B, const gl::Ext *d_pts,
                         gl::Ext **zpow_out, gl::Ext **d_open_out, std::vector<gl::Ext> &open) {
  const unsigned Bu = (unsigned)Bn;
  const size_t n = D.n;
  gl::Ext *zpow, *d_open;
  CP_TRY(arena_alloc(ctx, 4 * Bn * n * 16, (void **)&zpow));
  CP_TRY(arena_alloc(ctx, Bn * D.open_stride * 16, (void **)&d_open));
  LAUNCH(ctx, "fri_ext_powers", fri::k_ext_powers, dim3(blocks_for(n, 256), 4 * Bu), dim3(256), d_pts, n, zpow);
  size_t o = 0;
  LAUNCH(ctx, "eval_at_point", fri::k_eval_at_point, dim3((unsigned)D.k_cs, Bu), dim3(256), (const uint64_t *)nullptr,
         (size_t)0, t.t_coeffs, n, zpow, 2 * n, d_open, D.open_stride, o);
  o += D.k_cs;
  for (int b = 1; b < 4; b++) {
    LAUNCH(ctx, "eval_at_point", fri::k_eval_at_point, dim3((unsigned)B[b].k, Bu), dim3(256), B[b].coeffs,
           B[b].coeffs_stride, (const uint64_t *const *)nullptr, n, zpow, 2 * n, d_open, D.open_stride, o);
    o += B[b].k;
  }
  LAUNCH(ctx, "eval_at_point", fri::k_eval_at_point, dim3((unsigned)nc, Bu), dim3(256), B[2].coeffs, B[2].coeffs_stride,
         (const uint64_t *const *)nullptr, n, zpow + n, 2 * n, d_open, D.open_stride, o);
  open.resize(Bn * D.open_stride);
  *zpow_out = zpow;
  *d_open_out = d_open;
  return fetch_async(ctx, open.data(), d_open, open.size() * 16);
}

// the FRI opening proof: PolynomialBatch::prove_openings over the four oracles, batches at zeta and g*zeta
static int tail_fri(cp_ctx *ctx, size_t Bn, const cp_shape &sh, const TailDims &D, const TailTables &t, const DevBatch *B, const gl::Ext *zpow,
                    const gl::Ext *d_open, Transcript &T, const int *use_pow, const uint64_t *pow_ov, FriHostOut &fri_out) {
  const int nc = sh.num_challenges;
  std::vector<OracleRef> oracles(4);
  oracles[0].k = D.k_cs;
  oracles[0].t_coeffs = t.t_coeffs; oracles[0].t_lde = t.t_lde; oracles[0].t_dig = t.t_dig;
  for (int b = 1; b < 4; b++) {
    OracleRef &O = oracles[b];
    O.k = B[b].k;
    O.coeffs = B[b].coeffs; O.lde = B[b].lde; O.digests = B[b].digests;
    O.coeffs_stride = B[b].coeffs_stride; O.lde_stride = B[b].lde_stride; O.dig_stride = B[b].dig_stride;
    O.salt = B[b].salt; O.salt_stride = B[b].salt_stride; O.n_salt = B[b].n_salt;
  }
  std::vector<FriBatchDesc> fbatches(2);  // plonky2 `FRI_ORACLES` / `fri_instance`: everything at zeta, the Z polynomials at g*zeta
  fbatches[0].ranges = {{0, 0, (uint32_t)D.k_cs}, {1, 0, (uint32_t)D.k_w}, {2, 0, (uint32_t)D.k_z}, {3, 0, (uint32_t)D.k_q}};
  fbatches[0].n_polys = D.k_all;
  fbatches[1].ranges = {{2, 0, (uint32_t)nc}};
  fbatches[1].n_polys = (size_t)nc;
  FriCfg cfg;
  cfg.rate_bits = sh.rate_bits; cfg.cap_height = sh.cap_height; cfg.pow_bits = sh.pow_bits; cfg.num_query_rounds = sh.num_query_rounds;
  cfg.n_arity = sh.n_arity;
  for (int l = 0; l < 8; l++) cfg.arity_bits[l] = sh.arity_bits[l];
  // observe_openings: the zeta batch, then zs_next — exactly the layout of d_open
  const tr::Seg opened{(const uint64_t *)d_open, nullptr, D.open_stride * 2, (uint32_t)(D.open_stride * 2)};
  return fri_prove_impl(ctx, Bn, sh.degree_bits, cfg, oracles, fbatches, zpow, zpow + 2 * Bn * D.n, T, opened, use_pow, pow_ov, t.d_flags, fri_out);
}

// bincode ProofWithPublicInputs of every proof
static void tail_encode(size_t Bn, const cp_shape &sh, const TailDims &D, const DevBatch *B, const std::vector<gl::Ext> &open,
                        const FriHostOut &fri_out, const uint64_t *const *pis, const size_t *n_pis, std::vector<ByteBuf> &outs) {
  const size_t nc = sh.num_challenges;
  outs.resize(Bn);
  for (size_t p = 0; p < Bn; p++) {
    ByteBuf &out = outs[p];
    out.v.reserve(8 * ((size_t)sh.num_query_rounds * fri_out.words + 8192 + n_pis[p]));
    for (int b = 1; b <= 3; b++) { out.u64(D.cap_n); out.felts(B[b].cap_host.data() + p * D.cap_n * 4, D.cap_n * 4); }
    const uint64_t *o = (const uint64_t *)(open.data() + p * D.open_stride);
    size_t pos = 0;
    auto put = [&](size_t cnt, size_t at) { out.u64(cnt); out.felts(o + 2 * at, 2 * cnt); };
    put(sh.num_constants, pos); pos += sh.num_constants;
    put(sh.num_routed_wires, pos); pos += sh.num_routed_wires;
    put(D.k_w, pos); pos += D.k_w;
    put(nc, pos);                 // plonk_zs
    put(nc, D.k_all);             // plonk_zs_next
    put(D.k_z - nc, pos + nc);    // partial_products
    pos += D.k_z;
    put(D.k_q, pos);
    out.u64(0); out.u64(0);       // lookup_zs, lookup_zs_next
    fri_out.bytes(p, out);        // FriProof
    out.u64(n_pis[p]); out.felts(pis[p], n_pis[p]);
  }
}

// `full`: wires -> proof (Z / partial products and the quotient chunks are computed here, A7 + A8);
// otherwise zs_pp_values / quotient_coeffs are supplied by the caller.
// The whole proof is ENQUEUED without a host round trip: the Fiat-Shamir transcripts live on the device (transcript.h), every
// challenge-dependent table is built by a kernel, every output is copied back behind the last kernel, and the host
// synchronises once, at the end.
static int prove_tail_batch_impl(cp_ctx *ctx, size_t Bn, cp_circuit *const *circs, const uint64_t *const *pis,
                                 const size_t *n_pis, const uint64_t *wires_values, const uint64_t *zs_pp_values,
                                 const uint64_t *quotient_coeffs, const int *use_pow, const uint64_t *pow_ov,
                                 std::vector<ByteBuf> &outs, bool full = false, const uint64_t *salts_dev = nullptr) {
  // salts_dev (zero-knowledge circuits only): [proof][3 oracles: wires, zs/partial products, quotient][CP_SALT_SIZE][N]
  host_phase(ctx, "setup");
  if ((circs[0]->sh.zero_knowledge != 0) != (salts_dev != nullptr))
    return set_error(ctx, CP_ERR_INVALID_ARG, circs[0]->sh.zero_knowledge ? "zero-knowledge circuit: use the *_zk entry point (salts needed)"
                                                                          : "salts given for a circuit that is not zero-knowledge");
  const cp_circuit &c0 = *circs[0];
  const cp_shape &sh = c0.sh;
  const int db = sh.degree_bits, rb = sh.rate_bits, ch = sh.cap_height, nc = sh.num_challenges;
  const TailDims D(sh);
  const size_t n = D.n, N = D.N;
  Transcript T;
  TailTables t;
  CP_TRY(tail_setup(ctx, Bn, circs, pis, n_pis, D, T, t));

  host_phase(ctx, "commit");
  // ---- commitments + transcript head -----------------------------------------------------------
  DevBatch B[4];
  B[0].k = D.k_cs;
  if (salts_dev)
    for (int b = 1; b <= 3; b++) {
      B[b].salt = salts_dev + (size_t)(b - 1) * CP_SALT_SIZE * N;
      B[b].salt_stride = (size_t)3 * CP_SALT_SIZE * N;
      B[b].n_salt = CP_SALT_SIZE;
    }
  // oracle b: k polynomials per proof, given as values over <omega_n> or (values == nullptr) as coefficients; its caps are copied back
  auto commit = [&](int b, size_t k, const uint64_t *values, const uint64_t *coeffs) -> int {
    DevBatch &O = B[b];
    CP_TRY(batch_alloc(ctx, O, Bn, k, n, N, ch));
    if (values) {
      CP_TRY(cp_commit_batch_dev(ctx, values, k, Bn, db, rb, ch, O.coeffs, O.lde, O.digests, O.cap));
    } else {  // LDE only
      CP_TRY(cp_d2d(ctx, O.coeffs, coeffs, Bn * k * n * 8));
      CP_TRY(cp_lde_dev(ctx, O.coeffs, n, db, rb, Bn * k, 7, CP_NTT_BITREV_OUT, O.lde, N));
    }
    if (!values || O.salt)  // no trees yet, or the leaves are longer than what the plain commitment hashed: trees over values + salt
      CP_TRY(merkle_cols_batch(ctx, O.lde, N, k, N, Bn, k * N, ch, O.digests, O.cap, O.salt, O.n_salt, O.salt_stride));
    O.cap_host.resize(Bn * D.cap_n * 4);
    return fetch_async(ctx, O.cap_host.data(), O.cap, O.cap_host.size() * 8);
  };
  auto cap_seg = [&](const DevBatch &b) { return tr::Seg{b.cap, nullptr, D.cap_n * 4, (uint32_t)(D.cap_n * 4)}; };
  CP_TRY(commit(1, D.k_w, wires_values, nullptr));
  uint64_t *d_chal;  // [proof][betas (nc) | gammas (nc)]: what the quotient kernels read; A7 reads it with stride 2 nc
  CP_TRY(arena_alloc(ctx, Bn * 2 * nc * 8, (void **)&d_chal));
  CP_TRY(transcript_step(ctx, T, {tr::Seg{t.d_head, nullptr, 8, 8}, cap_seg(B[1])}, 2 * nc, d_chal, (size_t)2 * nc));
  if (full) {  // A7: Z and partial products from the witness and (beta, gamma)
    uint64_t *zs_vals;
    CP_TRY(arena_alloc(ctx, Bn * D.k_z * n * 8, (void **)&zs_vals));
    CP_TRY(zs_launch(ctx, sh, Bn, t.d_sig, c0.k_is, wires_values, d_chal, d_chal + nc, (size_t)2 * nc, zs_vals));
    zs_pp_values = zs_vals;
  }
  CP_TRY(commit(2, D.k_z, zs_pp_values, nullptr));
  uint64_t *d_alphas;  // [proof][nc]
  CP_TRY(arena_alloc(ctx, Bn * nc * 8, (void **)&d_alphas));
  CP_TRY(transcript_step(ctx, T, {cap_seg(B[2])}, nc, d_alphas, (size_t)nc));
  if (full) {  // A8: quotient values on the LDE coset -> coefficients -> degree-n chunks
    uint64_t *qv;
    CP_TRY(quot_launch(ctx, sh, Bn, c0.gates, c0.num_selectors, c0.k_is, t.t_lde, B[1].lde, B[1].lde_stride, B[2].lde, B[2].lde_stride, d_chal,
                       d_alphas, t.d_head, &qv));
    quotient_coeffs = qv;
  }
  CP_TRY(commit(3, D.k_q, nullptr, quotient_coeffs));  // quotient chunks in coefficient form
  // zeta, and from it the two opening points [proof][zeta, g*zeta] and their inverses (plonky2: zeta must not lie in the subgroup)
  uint64_t *d_zeta;
  gl::Ext *d_pts;
  CP_TRY(arena_alloc(ctx, Bn * 16, (void **)&d_zeta));
  CP_TRY(arena_alloc(ctx, 4 * Bn * 16, (void **)&d_pts));
  CP_TRY(transcript_step(ctx, T, {cap_seg(B[3])}, 2, d_zeta, 2));
  LAUNCH(ctx, "plonk_points", tr::k_plonk_points, dim3(blocks_for(Bn, 64)), dim3(64), d_zeta, (unsigned)Bn, GL_ROOTS[db], db, d_pts, t.d_flags);

  host_phase(ctx, "openings");
  gl::Ext *zpow, *d_open;
  std::vector<gl::Ext> open;
  CP_TRY(tail_openings(ctx, Bn, nc, D, t, B, d_pts, &zpow, &d_open, open));
  FriHostOut fri_out;
  CP_TRY(tail_fri(ctx, Bn, sh, D, t, B, zpow, d_open, T, use_pow, pow_ov, fri_out));

  host_phase(ctx, "drain");
  CP_TRY(fetch_flush(ctx));  // the one synchronisation of the call
  CP_TRY(fri_out.check(ctx));

  host_phase(ctx, "bincode");
  tail_encode(Bn, sh, D, B, open, fri_out, pis, n_pis, outs);
  return CP_OK;
}

// Argument checks shared by every proving entry point — run BEFORE anything is staged or allocated.
static int validate_batch(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs,
                          const size_t *n_public_inputs, bool need_gates, const int *use_pow_override, const uint64_t *pow_override,
                          std::vector<int> *up, std::vector<uint64_t> *ov, const cp_ctx *owner = nullptr) {
  // owner: the context the circuits must belong to when messages are NOT to be written to it (ctx == nullptr: cp_batcher_prove)
  if (!owner) owner = ctx;
  if (!circuits || !public_inputs || !n_public_inputs) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (!circuits[0]) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit 0 is NULL");
  const size_t cap = max_batch(circuits[0]->sh);
  if (n_proofs > cap)
    return set_error(ctx, CP_ERR_INVALID_ARG, "batch of %zu proofs is too large for this shape (max %zu: 65535 polynomials per launch, 4096 proofs)",
                     n_proofs, cap);
  if (up) up->assign(n_proofs, 0);
  if (ov) ov->assign(n_proofs, 0);
  for (size_t p = 0; p < n_proofs; p++) {
    if (!circuits[p]) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit %zu is NULL", p);
    if (!owns(owner, circuits[p])) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit %zu belongs to another context", p);
    if (need_gates && !circuits[p]->has_gates) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit %zu has no gate set (cp_circuit_set_gates)", p);
    if (!same_shape(circuits[p]->sh, circuits[0]->sh))
      return set_error(ctx, CP_ERR_INVALID_ARG, "circuit %zu has a different shape: one batch = one shape", p);
    if (need_gates && (circuits[p]->num_selectors != circuits[0]->num_selectors || circuits[p]->gates.size() != circuits[0]->gates.size() ||
                       (circuits[p]->gates.size() &&
                        memcmp(circuits[p]->gates.data(), circuits[0]->gates.data(), circuits[0]->gates.size() * sizeof(quot::Gate)) != 0)))
      return set_error(ctx, CP_ERR_INVALID_ARG, "circuit %zu has a different gate set: one batch = one shape", p);
    if (n_public_inputs[p] != (size_t)circuits[p]->sh.num_public_inputs)
      return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu: %zu public inputs given, the circuit has %d", p, n_public_inputs[p],
                       circuits[p]->sh.num_public_inputs);
    if (n_public_inputs[p] && !public_inputs[p]) return set_error(ctx, CP_ERR_INVALID_ARG, "public inputs %zu are NULL", p);
    for (size_t i = 0; i < n_public_inputs[p]; i++)
      if (public_inputs[p][i] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu: public input %zu is not canonical", p, i);
    if (use_pow_override && use_pow_override[p]) {
      if (!pow_override || pow_override[p] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "proof %zu: pow witness is not canonical", p);
      if (up) (*up)[p] = 1;
      if (ov) (*ov)[p] = pow_override[p];
    }
  }
  return CP_OK;
}

// proofs as malloc'd buffers (cp_free); all or nothing
static int copy_out(cp_ctx *ctx, size_t n_proofs, const std::vector<ByteBuf> &outs, uint8_t **proofs_out, size_t *proof_lens) {
  for (size_t p = 0; p < n_proofs; p++) { proofs_out[p] = nullptr; proof_lens[p] = 0; }
  for (size_t p = 0; p < n_proofs; p++) {
    uint8_t *buf = (uint8_t *)malloc(outs[p].v.size());
    if (!buf) {
      for (size_t q = 0; q < p; q++) { free(proofs_out[q]); proofs_out[q] = nullptr; proof_lens[q] = 0; }
      return set_error(ctx, CP_ERR_OOM, "out of host memory");
    }
    memcpy(buf, outs[p].v.data(), outs[p].v.size());
    proofs_out[p] = buf;
    proof_lens[p] = outs[p].v.size();
  }
  return CP_OK;
}

int cp_prove_tail_batch(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs,
                        const size_t *n_public_inputs, const uint64_t *wires_values_dev, const uint64_t *zs_pp_values_dev,
                        const uint64_t *quotient_coeffs_dev, const int *use_pow_override, const uint64_t *pow_override,
                        uint8_t **proofs_out, size_t *proof_lens) try {
  CHECK_CTX(ctx);
  if (n_proofs == 0) return CP_OK;
  if (!circuits || !public_inputs || !n_public_inputs || !wires_values_dev || !zs_pp_values_dev || !quotient_coeffs_dev ||
      !proofs_out || !proof_lens)
    return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  std::vector<int> up;
  std::vector<uint64_t> ov;
  CP_TRY(validate_batch(ctx, n_proofs, circuits, public_inputs, n_public_inputs, false, use_pow_override, pow_override, &up, &ov));
  std::vector<ByteBuf> outs;
  {
    ArenaScope arena_scope(ctx);
    CP_TRY(prove_tail_batch_impl(ctx, n_proofs, circuits, public_inputs, n_public_inputs, wires_values_dev, zs_pp_values_dev,
                                 quotient_coeffs_dev, up.data(), ov.data(), outs));
  }
  return copy_out(ctx, n_proofs, outs, proofs_out, proof_lens);
} CP_CATCH(ctx)

// ---- FRI primitives: the kernels the opening proof is built from, callable on their own -------------------------
int cp_fri_combine_dev(cp_ctx *ctx, const uint64_t *polys_dev, size_t k, size_t n, const uint64_t alpha[2], uint64_t *comp_dev) try {
  CHECK_CTX(ctx);
  if (k == 0 || n == 0) return CP_OK;
  if (!polys_dev || !alpha || !comp_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (k > (1u << 20) || n > ((size_t)1 << 32)) return set_error(ctx, CP_ERR_INVALID_ARG, "k / n out of range");
  if (alpha[0] >= gl::P || alpha[1] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "alpha is not canonical");
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);
  std::vector<gl::Ext> ap(k);
  gl::Ext acc{1, 0};
  const gl::Ext al{alpha[0], alpha[1]};
  for (size_t i = 0; i < k; i++) { ap[i] = acc; acc = gl::ext_mul(acc, al); }
  gl::Ext *d_ap;
  CP_TRY(arena_alloc(ctx, k * 16, (void **)&d_ap));
  CP_TRY(push(ctx, d_ap, ap.data(), k * 16));
  fri::BatchRefs refs;
  memset(&refs, 0, sizeof refs);
  refs.n = n;
  refs.base[0] = polys_dev;
  refs.n_ranges = 1;
  refs.r_oracle[0] = 0; refs.r_first[0] = 0; refs.r_count[0] = (int)k;
  LAUNCH(ctx, "fri_combine", fri::k_combine, dim3(blocks_for(n, 256), 1), dim3(256), refs, d_ap, k, (size_t)0, 0, (gl::Ext *)comp_dev);
  return CP_OK;
} CP_CATCH(ctx)

int cp_fri_fold_dev(cp_ctx *ctx, const uint64_t *coeffs_dev, size_t n_in, int arity_bits, const uint64_t beta[2], uint64_t *out_dev) try {
  CHECK_CTX(ctx);
  if (!coeffs_dev || !beta || !out_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (arity_bits < 1 || arity_bits > 5) return set_error(ctx, CP_ERR_INVALID_ARG, "arity_bits %d out of range [1, 5]", arity_bits);
  if (n_in == 0 || (n_in & ((size_t)(1 << arity_bits) - 1))) return set_error(ctx, CP_ERR_INVALID_ARG, "n_in must be a non-zero multiple of the arity");
  if (beta[0] >= gl::P || beta[1] >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "beta is not canonical");
  ArenaScope arena_scope(ctx, ctx->arena.used == 0);
  gl::Ext *d_beta;
  CP_TRY(arena_alloc(ctx, 16, (void **)&d_beta));
  const gl::Ext b{beta[0], beta[1]};
  CP_TRY(push(ctx, d_beta, &b, 16));
  const size_t n_out = n_in >> arity_bits;
  LAUNCH(ctx, "fri_fold", fri::k_fold, dim3(blocks_for(n_out, 256), 1), dim3(256), coeffs_dev, 2 * n_in, n_in, n_out, 1 << arity_bits, d_beta,
         out_dev, 2 * n_out);
  return CP_OK;
} CP_CATCH(ctx)

int cp_circuit_set_gates(cp_circuit *c, const cp_gate *gates, size_t n_gates, int num_selectors) try {
  if (!c) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_ctx *ctx = c->ctx;
  if ((!gates && n_gates) || n_gates > quot::MAX_GATES) return set_error(ctx, CP_ERR_INVALID_ARG, "bad gate list (max %d gates)", quot::MAX_GATES);
  if (num_selectors < 0 || num_selectors > c->sh.num_constants) return set_error(ctx, CP_ERR_INVALID_ARG, "num_selectors out of range");
  std::vector<quot::Gate> gs(n_gates);
  for (size_t i = 0; i < n_gates; i++) {
    const cp_gate &g = gates[i];
    if (g.type < 0 || g.type >= gates::N_TYPES) return set_error(ctx, CP_ERR_UNSUPPORTED, "gate %zu: unsupported gate type %d", i, g.type);
    if (g.selector_index < 0 || g.selector_index >= (num_selectors > 0 ? num_selectors : 1) || g.group_start < 0 ||
        g.group_end > (int)n_gates || g.group_start > g.group_end)
      return set_error(ctx, CP_ERR_INVALID_ARG, "gate %zu: bad selector group", i);
    const int consts_avail = c->sh.num_constants - num_selectors;
    if (g.param < 0 || g.param2 < 0 || g.param3 < 0 || g.param > 4096 || g.param2 > 4096 || g.param3 > 64)
      return set_error(ctx, CP_ERR_INVALID_ARG, "gate %zu: bad parameters", i);
    bool ok = true;
    switch (g.type) {
      case CP_GATE_COMPARISON: ok = g.param2 >= 1 && g.param >= g.param2 && (g.param + g.param2 - 1) / g.param2 <= 8; break;
      case CP_GATE_U32_ADD_MANY: ok = g.param2 >= 1 && g.param2 <= 24; break;
      case CP_GATE_BASE_SUM: ok = g.param >= 1 && g.param2 >= 2 && g.param2 <= 16; break;
      case CP_GATE_RANDOM_ACCESS: ok = g.param >= 1 && g.param <= gates::MAX_RANDOM_ACCESS_BITS && g.param2 >= 1; break;
      case CP_GATE_REDUCING: case CP_GATE_REDUCING_EXT: ok = g.param >= 1; break;
      case CP_GATE_COSET_INTERPOLATION: ok = g.param >= 1 && g.param <= gates::MAX_COSET_BITS && g.param2 >= 2; break;
      case CP_GATE_EXPONENTIATION: ok = g.param >= 1; break;
      default: break;
    }
    if (!ok) return set_error(ctx, CP_ERR_INVALID_ARG, "gate %zu: unsupported parameters (%d, %d, %d) for gate type %d", i, g.param, g.param2, g.param3, g.type);
    const quot::Gate qg{g.type, g.selector_index, g.group_start, g.group_end, g.param, g.param2, g.param3};
    if (gates::num_wires(qg) > c->sh.num_wires)
      return set_error(ctx, CP_ERR_INVALID_ARG, "gate %zu needs %d wires, the circuit has %d", i, gates::num_wires(qg), c->sh.num_wires);
    if (gates::num_constants(qg) > consts_avail)
      return set_error(ctx, CP_ERR_INVALID_ARG, "gate %zu: not enough constants columns", i);
    if (gates::num_constraints(qg) > 512) return set_error(ctx, CP_ERR_INVALID_ARG, "gate %zu: too many constraints", i);
    gs[i] = qg;
  }
  c->gates = gs;
  c->num_selectors = num_selectors;
  c->has_gates = true;
  return CP_OK;
} CP_CATCH(c ? c->ctx : nullptr)

// `validated`: the host-memory entry points have run validate_batch before staging their inputs
static int prove_batch_checked(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs,
                               const size_t *n_public_inputs, const uint64_t *wires_values_dev, const uint64_t *salts_dev,
                               const int *use_pow_override, const uint64_t *pow_override, uint8_t **proofs_out,
                               size_t *proof_lens) {
  CHECK_CTX(ctx);
  if (n_proofs == 0) return CP_OK;
  if (!circuits || !public_inputs || !n_public_inputs || !wires_values_dev || !proofs_out || !proof_lens)
    return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  std::vector<int> up;
  std::vector<uint64_t> ov;
  CP_TRY(validate_batch(ctx, n_proofs, circuits, public_inputs, n_public_inputs, true, use_pow_override, pow_override, &up, &ov));
  std::vector<ByteBuf> outs;
  {
    ArenaScope arena_scope(ctx);  // drains the stream and rewinds the arena on every exit path, exceptions included
    CP_TRY(prove_tail_batch_impl(ctx, n_proofs, circuits, public_inputs, n_public_inputs, wires_values_dev, nullptr, nullptr,
                                 up.data(), ov.data(), outs, true, salts_dev));
    host_phase(ctx, "copy_out");
  }
  const int rc = copy_out(ctx, n_proofs, outs, proofs_out, proof_lens);
  host_phase(ctx, nullptr);
  return rc;
}

int cp_prove_batch(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs,
                   const size_t *n_public_inputs, const uint64_t *wires_values_dev, const int *use_pow_override,
                   const uint64_t *pow_override, uint8_t **proofs_out, size_t *proof_lens) try {
  return prove_batch_checked(ctx, n_proofs, circuits, public_inputs, n_public_inputs, wires_values_dev, nullptr, use_pow_override,
                             pow_override, proofs_out, proof_lens);
} CP_CATCH(ctx)

// wires (and, for zero-knowledge circuits, salts) from host memory into the context's device staging buffer
static int stage_host_inputs(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *wires_values_host,
                             const uint64_t *const *salts_host, const uint64_t **wires_dev, const uint64_t **salts_dev) {
  if (!wires_values_host) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  const cp_shape &sh = circuits[0]->sh;  // the caller has run validate_batch: every circuit is valid and of this shape
  const size_t per = ((size_t)sh.num_wires << sh.degree_bits) * 8;
  const size_t per_salt = salts_host ? ((size_t)3 * CP_SALT_SIZE << (sh.degree_bits + sh.rate_bits)) * 8 : 0;
  const size_t need = (per + per_salt) * n_proofs;
  CP_TRY(alloc_status(ctx, ctx->wires_stage.grow(need), need));  // grows to the largest batch seen, then stays
  char *salt_base = ctx->wires_stage.get<char>() + per * n_proofs;
  for (size_t p = 0; p < n_proofs; p++) {
    if (!wires_values_host[p]) return set_error(ctx, CP_ERR_INVALID_ARG, "wires %zu are NULL", p);
    if (hipMemcpyAsync(ctx->wires_stage.get<char>() + p * per, wires_values_host[p], per, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      return set_error(ctx, CP_ERR_HIP, "host-to-device copy of wires %zu failed", p);
    if (salts_host) {
      if (!salts_host[p]) return set_error(ctx, CP_ERR_INVALID_ARG, "salts %zu are NULL", p);
      if (hipMemcpyAsync(salt_base + p * per_salt, salts_host[p], per_salt, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return set_error(ctx, CP_ERR_HIP, "host-to-device copy of salts %zu failed", p);
    }
  }
  *wires_dev = ctx->wires_stage.get<uint64_t>();
  *salts_dev = salts_host ? (const uint64_t *)salt_base : nullptr;
  return CP_OK;
}

// cp_ctx_set_lanes: the batch in contiguous parts, one per lane, each staged and proved by its own short-lived thread.
// Returns 1 when the call was not split (one lane, a small batch, or profiling: the per-kernel profile belongs to ctx).
static int prove_host_lanes(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs,
                            const size_t *n_public_inputs, const uint64_t *const *wires_values_host, const uint64_t *const *salts_host,
                            const int *use_pow_override, const uint64_t *pow_override, uint8_t **proofs_out, size_t *proof_lens) {
  size_t L = (size_t)ctx->n_lanes;
  if (L > n_proofs / 4) L = n_proofs / 4;
  if (L > 8) L = 8;
  if (L <= 1 || ctx->profiling || ctx->parent) return 1;
  if (!circuits || !public_inputs || !n_public_inputs || !wires_values_host || !proofs_out || !proof_lens)
    return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  CP_TRY(validate_batch(ctx, n_proofs, circuits, public_inputs, n_public_inputs, true, use_pow_override, pow_override, nullptr, nullptr));
  for (size_t p = 0; p < n_proofs; p++) { proofs_out[p] = nullptr; proof_lens[p] = 0; }
  int rc[8];
  hostu::Joiner th[8];  // joined on every exit path
  const size_t base = n_proofs / L, rem = n_proofs % L;
  auto part = [&](size_t l) noexcept {  // lane l's contiguous share of the batch
    size_t o = 0;
    for (size_t i = 0; i < l; i++) o += base + (i < rem ? 1 : 0);
    const size_t cnt = base + (l < rem ? 1 : 0);
    cp_ctx *lane = ctx->lanes[l];
    int r;
    try {
      const uint64_t *wd = nullptr, *sd = nullptr;
      r = hipSetDevice(lane->device) == hipSuccess ? CP_OK : set_error(lane, CP_ERR_HIP, "hipSetDevice failed");
      if (r == CP_OK) r = stage_host_inputs(lane, cnt, circuits + o, wires_values_host + o, salts_host ? salts_host + o : nullptr, &wd, &sd);
      if (r == CP_OK)
        r = prove_batch_checked(lane, cnt, circuits + o, public_inputs + o, n_public_inputs + o, wd, sd,
                                use_pow_override ? use_pow_override + o : nullptr, pow_override ? pow_override + o : nullptr,
                                proofs_out + o, proof_lens + o);
    } catch (...) {
      r = exception_status(lane);
    }
    rc[l] = r;
  };
  bool inline_part[8] = {false};
  for (size_t l = 1; l < L; l++) inline_part[l] = !hostu::try_spawn(th[l].t, [&part, l] { part(l); });
  part(0);  // the calling thread takes the first share, then whatever share found no thread
  for (size_t l = 1; l < L; l++)
    if (inline_part[l]) part(l);
  for (size_t l = 1; l < L; l++)
    if (th[l].t.joinable()) th[l].t.join();
  (void)hipSetDevice(ctx->device);
  for (size_t l = 0; l < L; l++)
    if (rc[l] != CP_OK) {  // all or nothing, like the unsplit call
      for (size_t p = 0; p < n_proofs; p++) { free(proofs_out[p]); proofs_out[p] = nullptr; proof_lens[p] = 0; }
      return set_error(ctx, rc[l], "%s", ctx->lanes[l]->error.c_str());
    }
  return CP_OK;
}

int cp_prove_batch_host(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs,
                        const size_t *n_public_inputs, const uint64_t *const *wires_values_host, const int *use_pow_override,
                        const uint64_t *pow_override, uint8_t **proofs_out, size_t *proof_lens) try {
  CHECK_CTX(ctx);
  if (n_proofs == 0) return CP_OK;
  const int split = prove_host_lanes(ctx, n_proofs, circuits, public_inputs, n_public_inputs, wires_values_host, nullptr,
                                     use_pow_override, pow_override, proofs_out, proof_lens);
  if (split != 1) return split;
  const uint64_t *wd, *sd;
  CP_TRY(validate_batch(ctx, n_proofs, circuits, public_inputs, n_public_inputs, true, use_pow_override, pow_override, nullptr, nullptr));
  CP_TRY(stage_host_inputs(ctx, n_proofs, circuits, wires_values_host, nullptr, &wd, &sd));
  return prove_batch_checked(ctx, n_proofs, circuits, public_inputs, n_public_inputs, wd, nullptr, use_pow_override, pow_override,
                             proofs_out, proof_lens);
} CP_CATCH(ctx)

int cp_prove_batch_zk_host(cp_ctx *ctx, size_t n_proofs, cp_circuit *const *circuits, const uint64_t *const *public_inputs,
                           const size_t *n_public_inputs, const uint64_t *const *wires_values_host,
                           const uint64_t *const *salts_host, const int *use_pow_override, const uint64_t *pow_override,
                           uint8_t **proofs_out, size_t *proof_lens) try {
  CHECK_CTX(ctx);
  if (n_proofs == 0) return CP_OK;
  if (!salts_host) return set_error(ctx, CP_ERR_INVALID_ARG, "salts are NULL");
  const int split = prove_host_lanes(ctx, n_proofs, circuits, public_inputs, n_public_inputs, wires_values_host, salts_host,
                                     use_pow_override, pow_override, proofs_out, proof_lens);
  if (split != 1) return split;
  const uint64_t *wd, *sd;
  CP_TRY(validate_batch(ctx, n_proofs, circuits, public_inputs, n_public_inputs, true, use_pow_override, pow_override, nullptr, nullptr));
  CP_TRY(stage_host_inputs(ctx, n_proofs, circuits, wires_values_host, salts_host, &wd, &sd));
  return prove_batch_checked(ctx, n_proofs, circuits, public_inputs, n_public_inputs, wd, sd, use_pow_override, pow_override,
                             proofs_out, proof_lens);
} CP_CATCH(ctx)

int cp_prove(cp_circuit *circuit, const uint64_t *wires_values_host, const uint64_t *public_inputs, size_t n_public_inputs,
             int use_pow_override, uint64_t pow_override, uint8_t **proof_out, size_t *proof_len) try {
  if (!circuit) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_circuit *cs[1] = {circuit};
  const uint64_t *pis[1] = {public_inputs}, *ws[1] = {wires_values_host};
  return cp_prove_batch_host(circuit->ctx, 1, cs, pis, &n_public_inputs, ws, &use_pow_override, &pow_override, proof_out, proof_len);
} CP_CATCH(circuit ? circuit->ctx : nullptr)

int cp_prove_tail(cp_circuit *circ, const uint64_t *public_inputs, size_t n_pi, const uint64_t *wires_values_dev,
                  const uint64_t *zs_pp_values_dev, const uint64_t *quotient_coeffs_dev, int use_pow_override,
                  uint64_t pow_override, uint8_t **proof_out, size_t *proof_len) try {
  if (!circ) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_circuit *cs[1] = {circ};
  const uint64_t *pi[1] = {public_inputs};
  size_t npi[1] = {n_pi};
  int up[1] = {use_pow_override};
  uint64_t ov[1] = {pow_override};
  return cp_prove_tail_batch(circ->ctx, 1, cs, pi, npi, wires_values_dev, zs_pp_values_dev, quotient_coeffs_dev, up, ov,
                             proof_out, proof_len);
} CP_CATCH(circ ? circ->ctx : nullptr)

}  // extern "C"
