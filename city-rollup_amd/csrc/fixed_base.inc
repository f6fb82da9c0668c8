// Host side of the batched fixed-base multiplication (kernels: fixed_base.h), one template for G1 and G2.
// Included by bls.hip after groth16.inc (point_in).
namespace {

static_assert(sizeof(bls::Fp) * fixedbase::K * fixedbase::LANES<bls::Fp> <= 64 * 1024 && sizeof(bls::Fp2) * fixedbase::K * fixedbase::LANES<bls::Fp2> <= 64 * 1024,
              "the ZZ columns of a workgroup must fit its LDS");

// the window table of `base`: built on first use and kept by the context, per group, until another base is asked for
template <class F>
int fixed_base_table(cp_ctx *ctx, const uint64_t *base_xy, const bls::JacT<F> &base, const bls::AffineT<F> **out) {
  using J = bls::JacT<F>;
  constexpr size_t BASE_BYTES = 2 * bls::Field<F>::WORDS * 4;
  auto &cache = ctx->fixed_base[sizeof(F) == sizeof(bls::Fp) ? 0 : 1];
  *out = cache.tab.template get<const bls::AffineT<F>>();
  if (cache.valid && memcmp(cache.base, base_xy, BASE_BYTES) == 0) return CP_OK;
  cache.valid = false;
  const size_t bytes = fixedbase::TABLE_POINTS * sizeof(bls::AffineT<F>);
  CP_TRY(alloc_status(ctx, cache.tab.grow(bytes), bytes));
  *out = cache.tab.template get<const bls::AffineT<F>>();
  std::vector<J> bases(fixedbase::WINDOWS);  // 2^(8 w) * base: 256 doublings on the host
  J p = base;
  for (int w = 0; w < fixedbase::WINDOWS; w++) {
    bases[w] = p;
    for (int i = 0; i < fixedbase::WINDOW_BITS; i++) p = bls::jac_double(p);
  }
  DevBag tmp = ctx->bag();
  J *d_bases = nullptr;
  uint32_t *d_infinite = nullptr;
  CP_TRY(alloc_status(ctx, tmp.alloc(&d_bases, bases.size() * sizeof(J)), bases.size() * sizeof(J)));
  CP_TRY(alloc_status(ctx, tmp.alloc(&d_infinite, 4), 4));
  HIP_TRY(ctx, hipMemcpyAsync(d_bases, bases.data(), bases.size() * sizeof(J), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_infinite, 0, 4, ctx->stream));
  LAUNCH(ctx, "fixed_base_table", fixedbase::k_table<F>, dim3(blocks_for(fixedbase::TABLE_POINTS, 64)), dim3(64), (const J *)d_bases,
         cache.tab.template get<bls::AffineT<F>>(), d_infinite);
  uint32_t infinite = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&infinite, d_infinite, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (infinite)
    return set_error(ctx, CP_ERR_INVALID_ARG, "base has small order: %u of its window multiples are the point at infinity (it is not in the prime-order subgroup)", infinite);
  memcpy(cache.base, base_xy, BASE_BYTES);
  cache.valid = true;
  return CP_OK;
}

// out[i] = scalars[i] * base for i < n, flags in inf; everything device-resident, asynchronous once the table exists
template <class F>
int fixed_base_run(cp_ctx *ctx, const uint64_t *base_xy, const uint64_t *scalars_dev, size_t n, void *out, uint8_t *inf) {
  bls::JacT<F> base;
  CP_TRY(point_in<F>(ctx, base_xy, "base", &base));
  const bls::AffineT<F> *table = nullptr;
  CP_TRY(fixed_base_table<F>(ctx, base_xy, base, &table));
  const size_t lanes = (n + fixedbase::K - 1) / fixedbase::K;
  LAUNCH(ctx, sizeof(F) == sizeof(bls::Fp) ? "fixed_base_mul_g1" : "fixed_base_mul_g2", fixedbase::k_mul<F>, dim3(blocks_for(lanes, fixedbase::LANES<F>)),
         dim3(fixedbase::LANES<F>), table, (const uint8_t *)scalars_dev, n, bls::AffineT<F>{base.x, base.y}, (bls::AffineT<F> *)out, inf);
  return CP_OK;
}

// an array the runtime knows to live on another device than the context's is refused (anything else passes)
int on_ctx_device(cp_ctx *ctx, const void *p, const char *what) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return CP_OK; }
  if (a.type == hipMemoryTypeDevice && a.device != ctx->device)
    return set_error(ctx, CP_ERR_INVALID_ARG, "%s lives on device %d, the context on device %d", what, a.device, ctx->device);
  return CP_OK;
}

template <class F>
int fixed_base_dev(cp_ctx *ctx, const uint64_t *base_xy, const uint64_t *scalars_dev, size_t n, void *points_mont_dev_out,
                   uint8_t *points_inf_dev_out) {
  CHECK_CTX(ctx);
  if (!base_xy || !scalars_dev || !points_mont_dev_out || !points_inf_dev_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (n == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "fixed-base multiplication of no scalars (n = 0)");
  if (n > ((size_t)1 << 32)) return set_error(ctx, CP_ERR_INVALID_ARG, "fixed-base multiplication of %zu scalars is too large (max 2^32)", n);
  CP_TRY(on_ctx_device(ctx, scalars_dev, "scalars"));
  CP_TRY(on_ctx_device(ctx, points_mont_dev_out, "the point array"));
  CP_TRY(on_ctx_device(ctx, points_inf_dev_out, "the flag array"));
  return fixed_base_run<F>(ctx, base_xy, scalars_dev, n, points_mont_dev_out, points_inf_dev_out);
}

}  // namespace

extern "C" {

int cp_fixed_base_mul_bls12381_g1_dev(cp_ctx *ctx, const uint64_t base_xy[12], const uint64_t *scalars_dev, size_t n,
                                      void *points_mont_dev_out, uint8_t *points_inf_dev_out) try {
  return fixed_base_dev<bls::Fp>(ctx, base_xy, scalars_dev, n, points_mont_dev_out, points_inf_dev_out);
} CP_CATCH(ctx)
int cp_fixed_base_mul_bls12381_g2_dev(cp_ctx *ctx, const uint64_t base_xy[24], const uint64_t *scalars_dev, size_t n,
                                      void *points_mont_dev_out, uint8_t *points_inf_dev_out) try {
  return fixed_base_dev<bls::Fp2>(ctx, base_xy, scalars_dev, n, points_mont_dev_out, points_inf_dev_out);
} CP_CATCH(ctx)

}  // extern "C"
