// Host side of the point transforms (kernels: point_ntt.h), one template for G1 and G2. Included by bls.hip after fr_ntt.inc
// (the twiddle tables), groth16.inc (point_in) and fixed_base.inc (on_ctx_device).
namespace {

static_assert((2 * sizeof(bls::Jac) + 4 * pointntt::SCALAR_WORDS) * fixedbase::LANES<bls::Fp> <= 64 * 1024 &&
                  (2 * sizeof(bls::Jac2) + 4 * pointntt::SCALAR_WORDS) * fixedbase::LANES<bls::Fp2> <= 64 * 1024,
              "a partial sum, a product slot and a scalar per lane (g16srs::k_columns_chunk has the most) must fit the LDS of a workgroup");

template <class F> constexpr bool IS_G1 = sizeof(F) == sizeof(bls::Fp);

// the standard generator in the internal form: the entry under an infinity flag (fixed_base.h writes the same)
template <class F>
int generator_mont(cp_ctx *ctx, bls::AffineT<F> *out) {
  bls::JacT<F> g;
  if constexpr (IS_G1<F>) CP_TRY(point_in<F>(ctx, BLS_G1_GEN, "the G1 generator", &g));
  else CP_TRY(point_in<F>(ctx, BLS_G2_GEN, "the G2 generator", &g));
  *out = {g.x, g.y};
  return CP_OK;
}

int point_work(cp_ctx *ctx, size_t bytes, void **out) {
  CP_TRY(alloc_status(ctx, ctx->point_work.grow(bytes), bytes));
  *out = ctx->point_work.get<void>();
  return CP_OK;
}

// out[i] = scale * work[i] (scale != NULL; the work array is scaled in place) or work[i] for i < n, affine with flags: the one
// way out of a Jacobian work array
template <class F>
int point_finish(cp_ctx *ctx, bls::JacT<F> *work, size_t n, const uint64_t *scale, void *out, uint8_t *inf) {
  bls::AffineT<F> gen;
  CP_TRY(generator_mont<F>(ctx, &gen));
  const dim3 block(fixedbase::LANES<F>);
  if (scale) {
    pointntt::Scalar k;
    memcpy(k.w, scale, sizeof k.w);
    LAUNCH(ctx, IS_G1<F> ? "point_scale_g1" : "point_scale_g2", pointntt::k_scale<F>, dim3(blocks_for(n, fixedbase::LANES<F>)), block, work, n, k);
  }
  const size_t lanes = (n + pointntt::K - 1) / pointntt::K;
  LAUNCH(ctx, IS_G1<F> ? "point_affine_g1" : "point_affine_g2", pointntt::k_finish<F>, dim3(blocks_for(lanes, fixedbase::LANES<F>)), block, (const bls::JacT<F> *)work, n,
         gen, (bls::AffineT<F> *)out, inf);
  return CP_OK;
}

// in place over 2^log_n points and their flags; asynchronous on the context stream
template <class F>
int point_ntt_run(cp_ctx *ctx, void *pts, uint8_t *inf, int log_n, unsigned flags) {
  if (log_n < 0 || log_n > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "point NTT: log_n %d out of range (0..28)", log_n);
  if (flags & ~(unsigned)CP_NTT_INVERSE) return set_error(ctx, CP_ERR_INVALID_ARG, "point NTT: unsupported flags 0x%x (CP_NTT_INVERSE alone is known)", flags);
  const bool inverse = flags & CP_NTT_INVERSE;
  const size_t n = (size_t)1 << log_n;
  void *w = nullptr;
  CP_TRY(point_work(ctx, n * sizeof(bls::JacT<F>), &w));
  bls::JacT<F> *work = (bls::JacT<F> *)w;
  const blsfr::Fr *tw = nullptr;
  if (log_n > 0) CP_TRY(fr_twiddles(ctx, log_n, inverse, &tw));
  LAUNCH(ctx, "point_ntt_load", (pointntt::k_load<F, true>), dim3(blocks_for(n, 256)), dim3(256), (const bls::AffineT<F> *)pts, (const uint8_t *)inf, n, log_n, work);
  for (int s = 0; s < log_n; s++)
    LAUNCH(ctx, IS_G1<F> ? "point_ntt_stage_g1" : "point_ntt_stage_g2", pointntt::k_stage<F>, dim3(blocks_for(n / 2, fixedbase::LANES<F>)), dim3(fixedbase::LANES<F>),
           work, n / 2, s, log_n, tw);
  uint64_t scale[4];
  if (inverse && log_n > 0) {
    const uint32_t nn[8] = {(uint32_t)n, 0, 0, 0, 0, 0, 0, 0};
    blsfr::fr_to_canonical(blsfr::fr_inv(blsfr::fr_from_canonical(nn)), (uint32_t *)scale);
  }
  return point_finish<F>(ctx, work, n, inverse && log_n > 0 ? scale : nullptr, pts, inf);
}

template <class F>
int point_ntt_dev(cp_ctx *ctx, void *points_mont_dev, uint8_t *points_inf_dev, int log_n, unsigned flags) {
  CHECK_CTX(ctx);
  if (!points_mont_dev || !points_inf_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "point NTT: NULL argument");
  CP_TRY(on_ctx_device(ctx, points_mont_dev, "the point array"));
  CP_TRY(on_ctx_device(ctx, points_inf_dev, "the flag array"));
  return point_ntt_run<F>(ctx, points_mont_dev, points_inf_dev, log_n, flags);
}

}  // namespace

extern "C" {

int cp_point_ntt_bls12381_g1_dev(cp_ctx *ctx, void *points_mont_dev, uint8_t *points_inf_dev, int log_n, unsigned flags) try {
  return point_ntt_dev<bls::Fp>(ctx, points_mont_dev, points_inf_dev, log_n, flags);
} CP_CATCH(ctx)
int cp_point_ntt_bls12381_g2_dev(cp_ctx *ctx, void *points_mont_dev, uint8_t *points_inf_dev, int log_n, unsigned flags) try {
  return point_ntt_dev<bls::Fp2>(ctx, points_mont_dev, points_inf_dev, log_n, flags);
} CP_CATCH(ctx)

}  // extern "C"
