// Host side of the F_r NTT (kernels: fr_ntt.h). Included by bls.hip after msm.inc.
namespace {

// twiddle table omega^i, i < n/2 (omega = the primitive n-th root, or its inverse), cached per context
int fr_twiddles(cp_ctx *ctx, int log_n, bool inverse, const blsfr::Fr **out) {
  const auto key = std::make_pair(log_n, inverse ? 1 : 0);
  auto it = ctx->fr_twiddles.find(key);
  if (it != ctx->fr_twiddles.end()) { *out = it->second.get<const blsfr::Fr>(); return CP_OK; }
  const size_t half = log_n ? ((size_t)1 << (log_n - 1)) : 1;
  DevBuf tab = ctx->buf();
  CP_TRY(alloc_status(ctx, tab.alloc(half * sizeof(blsfr::Fr)), half * sizeof(blsfr::Fr)));
  blsfr::Fr w = blsfr::fr_from_canonical(BLS_FR_ROOTS[log_n]);
  if (inverse) w = blsfr::fr_inv(w);
  LAUNCH(ctx, "fr_twiddles", frntt::k_powers, dim3(blocks_for(half, 256)), dim3(256), w, half, tab.get<blsfr::Fr>());
  *out = tab.get<const blsfr::Fr>();
  ctx->fr_twiddles[key] = std::move(tab);
  return CP_OK;
}

int fr_ntt_run(cp_ctx *ctx, uint64_t *data_dev, int log_n, unsigned flags, const uint64_t *shift) {
  if (log_n < 0 || log_n > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "F_r NTT: log_n %d out of range (0..28)", log_n);
  if (flags & ~(unsigned)(CP_NTT_INVERSE | CP_NTT_COSET)) return set_error(ctx, CP_ERR_INVALID_ARG, "F_r NTT: unsupported flags 0x%x", flags);
  const bool inverse = flags & CP_NTT_INVERSE, coset = flags & CP_NTT_COSET;
  if (coset && !shift) return set_error(ctx, CP_ERR_INVALID_ARG, "coset transform without a shift");
  const size_t n = (size_t)1 << log_n;
  blsfr::Fr *powers = nullptr;
  CP_TRY(alloc_status(ctx, ctx->fr_work.grow(n * sizeof(blsfr::Fr)), n * sizeof(blsfr::Fr)));  // grow-only: no hipMalloc / hipFree in the steady state
  blsfr::Fr *work = ctx->fr_work.get<blsfr::Fr>();
  const blsfr::Fr *tw = nullptr;
  if (log_n > 0) CP_TRY(fr_twiddles(ctx, log_n, inverse, &tw));
  if (coset) {
    if (!blsfr::fr_is_canonical((const uint32_t *)shift)) return set_error(ctx, CP_ERR_INVALID_ARG, "coset shift is not canonical");
    blsfr::Fr s = blsfr::fr_from_canonical((const uint32_t *)shift);
    bool zero = true;
    for (int i = 0; i < blsfr::NL; i++) zero = zero && s.l[i] == 0;
    if (zero) return set_error(ctx, CP_ERR_INVALID_ARG, "coset shift is zero");
    if (inverse) s = blsfr::fr_inv(s);
    // one fr_pow_u64 per element costs more than the transform itself: the table is kept until another size or
    // shift is asked for
    auto &cache = ctx->fr_pow[inverse ? 1 : 0];
    const bool hit = cache.tab && cache.log_n == log_n && memcmp(cache.shift, shift, 32) == 0;
    if (!hit) {
      cache.log_n = -1;
      CP_TRY(alloc_status(ctx, cache.tab.grow(n * sizeof(blsfr::Fr)), n * sizeof(blsfr::Fr)));
      LAUNCH(ctx, "fr_powers", frntt::k_powers, dim3(blocks_for(n, 256)), dim3(256), s, n, cache.tab.get<blsfr::Fr>());
      cache.log_n = log_n;
      memcpy(cache.shift, shift, 32);
    }
    powers = cache.tab.get<blsfr::Fr>();
  }
  const blsfr::Fr *in_pow = coset && !inverse ? powers : nullptr;
  frntt::StoreArgs sa;
  sa.data = (uint32_t *)data_dev;
  sa.powers = coset && inverse ? powers : nullptr;
  sa.scale = blsfr::fr_one();
  sa.use_scale = inverse ? 1 : 0;
  sa.log_n = log_n;
  if (inverse) {
    uint32_t nn[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
    sa.scale = blsfr::fr_inv(blsfr::fr_from_canonical(nn));
  }
  const int tile_stages = log_n < frntt::LOG_TILE ? log_n : frntt::LOG_TILE;
  // stages above the tile: passes of at most 7 stages each (columns of >= 8 elements = 320 contiguous bytes), split evenly
  const int top = log_n - tile_stages, passes = (top + 6) / 7;
  int s = log_n - 1;
  for (int k = 0; k < passes; k++) {
    const int g = top / passes + (k < top % passes ? 1 : 0);
    if (k == 0)
      LAUNCH(ctx, "fr_colpass", frntt::k_colpass<true>, dim3((unsigned)(n >> frntt::LOG_TILE)), dim3(512), work, (const uint32_t *)data_dev,
             in_pow, n, s, g, tw);
    else
      LAUNCH(ctx, "fr_colpass", frntt::k_colpass<false>, dim3((unsigned)(n >> frntt::LOG_TILE)), dim3(512), work, (const uint32_t *)nullptr,
             (const blsfr::Fr *)nullptr, n, s, g, tw);
    s -= g;
  }
  // The store permutes across tiles (data[rev(p)]), so it may only run once every input has been read: after a
  // column pass that is guaranteed (it read all of `data` into `work`); without one, n <= 2^LOG_TILE and the single
  // workgroup has read all of `data` before its first barrier.
  if (passes > 0)
    LAUNCH(ctx, "fr_tile", (frntt::k_tile<false, true>), dim3((unsigned)(n >> tile_stages)), dim3(512), work, (const uint32_t *)nullptr,
           (const blsfr::Fr *)nullptr, n, tile_stages, n >> tile_stages, tw, sa);
  else  // n <= 2^LOG_TILE: one workgroup, which has read all of `data` before it writes any of it
    LAUNCH(ctx, "fr_tile", (frntt::k_tile<true, true>), dim3(1), dim3(512), work, (const uint32_t *)data_dev, in_pow, n, tile_stages,
           (size_t)1, tw, sa);
  return CP_OK;  // asynchronous on the context stream, like the other _dev entry points
}

// h = (a b - c) / (x^n - 1) via the coset g<omega_n>, g = 7 (the multiplicative generator gnark's domain uses)
int groth16_quotient_run(cp_ctx *ctx, uint64_t *a, uint64_t *b, uint64_t *c, int log_n) {
  if (log_n < 1 || log_n > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "Groth16 quotient: log_n %d out of range (1..28)", log_n);
  const size_t n = (size_t)1 << log_n;
  const uint64_t g[4] = {7, 0, 0, 0};
  uint64_t *v[3] = {a, b, c};
  for (uint64_t *x : v) {
    CP_TRY(fr_ntt_run(ctx, x, log_n, CP_NTT_INVERSE, nullptr));
    CP_TRY(fr_ntt_run(ctx, x, log_n, CP_NTT_COSET, g));
  }
  const blsfr::Fr gn = blsfr::fr_pow_u64(blsfr::fr_from_canonical((const uint32_t *)g), n);
  const blsfr::Fr den = blsfr::fr_inv(blsfr::fr_sub(gn, blsfr::fr_one()));  // g^n != 1: g generates the whole group
  LAUNCH(ctx, "fr_quotient_pointwise", frntt::k_quotient_pointwise, dim3(blocks_for(n, 256)), dim3(256), (uint32_t *)a, (const uint32_t *)b,
         (const uint32_t *)c, den, n);
  return fr_ntt_run(ctx, a, log_n, CP_NTT_INVERSE | CP_NTT_COSET, g);
}

}  // namespace

extern "C" {

int cp_groth16_quotient_bls12381_dev(cp_ctx *ctx, uint64_t *a_dev, uint64_t *b_dev, uint64_t *c_dev, int log_n) try {
  CHECK_CTX(ctx);
  if (!a_dev || !b_dev || !c_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL pointer");
  if (a_dev == b_dev || a_dev == c_dev || b_dev == c_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "a, b, c must be distinct arrays");
  return groth16_quotient_run(ctx, a_dev, b_dev, c_dev, log_n);
} CP_CATCH(ctx)

int cp_groth16_quotient_bls12381(cp_ctx *ctx, uint64_t *a_host, const uint64_t *b_host, const uint64_t *c_host, int log_n) try {
  CHECK_CTX(ctx);
  if (!a_host || !b_host || !c_host) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL pointer");
  if (log_n < 1 || log_n > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "Groth16 quotient: log_n %d out of range (1..28)", log_n);
  const size_t n = (size_t)1 << log_n;
  const uint64_t *in[3] = {a_host, b_host, c_host};
  for (int k = 0; k < 3; k++)
    for (size_t i = 0; i < n; i++)
      if (!blsfr::fr_is_canonical((const uint32_t *)(in[k] + 4 * i)))
        return set_error(ctx, CP_ERR_INVALID_ARG, "%c[%zu] is not canonical (>= r)", "abc"[k], i);
  DevBag D = ctx->bag();
  uint64_t *d[3];
  for (int k = 0; k < 3; k++) {
    CP_TRY(alloc_status(ctx, D.alloc(&d[k], n * 32), n * 32));
    HIP_TRY(ctx, hipMemcpyAsync(d[k], in[k], n * 32, hipMemcpyHostToDevice, ctx->stream));
  }
  CP_TRY(groth16_quotient_run(ctx, d[0], d[1], d[2], log_n));
  HIP_TRY(ctx, hipMemcpyAsync(a_host, d[0], n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CP_OK;
} CP_CATCH(ctx)

int cp_ntt_bls12381_fr_dev(cp_ctx *ctx, uint64_t *data_dev, int log_n, unsigned flags, const uint64_t *coset_shift) try {
  CHECK_CTX(ctx);
  if (!data_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "data is NULL");
  return fr_ntt_run(ctx, data_dev, log_n, flags, coset_shift);
} CP_CATCH(ctx)

int cp_ntt_bls12381_fr(cp_ctx *ctx, uint64_t *data_host, int log_n, unsigned flags, const uint64_t *coset_shift) try {
  CHECK_CTX(ctx);
  if (!data_host) return set_error(ctx, CP_ERR_INVALID_ARG, "data is NULL");
  if (log_n < 0 || log_n > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "F_r NTT: log_n %d out of range (0..28)", log_n);
  const size_t n = (size_t)1 << log_n;
  for (size_t i = 0; i < n; i++)
    if (!blsfr::fr_is_canonical((const uint32_t *)(data_host + 4 * i))) return set_error(ctx, CP_ERR_INVALID_ARG, "element %zu is not canonical (>= r)", i);
  DevBag D = ctx->bag();
  uint64_t *d;
  CP_TRY(alloc_status(ctx, D.alloc(&d, n * 32), n * 32));
  HIP_TRY(ctx, hipMemcpyAsync(d, data_host, n * 32, hipMemcpyHostToDevice, ctx->stream));
  CP_TRY(fr_ntt_run(ctx, d, log_n, flags, coset_shift));
  HIP_TRY(ctx, hipMemcpyAsync(data_host, d, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return CP_OK;
} CP_CATCH(ctx)

}  // extern "C"
