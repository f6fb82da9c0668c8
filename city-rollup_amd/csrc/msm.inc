// Host side of the BLS12-381 MSMs (kernels: msm.h), one template for G1 (F = Fp) and G2 (F = Fp2).
// Included by cityprover.hip.
namespace {

static_assert(sizeof(bls::Affine) == CP_G1_AFFINE_BYTES, "CP_G1_AFFINE_BYTES out of date");
static_assert(sizeof(bls::Affine2) == CP_G2_AFFINE_BYTES, "CP_G2_AFFINE_BYTES out of date");

struct DevBufs {  // carves the context's grow-only MSM workspace: plan() every array, commit(), then take() in the same order
  size_t need = 0, at = 0;
  char *base = nullptr;
  static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
  void plan(size_t bytes) { need += pad(bytes); }
  int commit(cp_ctx *ctx) {
    CP_TRY(alloc_status(ctx, ctx->msm_ws.grow(need), need));
    base = ctx->msm_ws.get<char>();
    return CP_OK;
  }
  template <class T>
  T *take(size_t bytes) {
    T *p = (T *)(base + at);
    at += pad(bytes);
    return p;
  }
};

int ilog2_floor(size_t v) { int l = 0; while (v >>= 1) l++; return l; }

// sum_i scalars[i] * points[i]; everything device-resident, the result as a Jacobian point on the host
template <class F>
int msm_run(cp_ctx *ctx, const uint32_t *scalars, const bls::AffineT<F> *pts, const uint8_t *inf, size_t n, bls::JacT<F> *result) {
  using J = bls::JacT<F>;
  *result = bls::jac_inf<F>();
  if (n == 0) return CP_OK;
  // window width ~log2(n) - 3 balances the n additions per window against the bucket reductions; taken from the widths
  // whose top window, for scalars below the 255-bit group order r, neither has only a few significant bits (a 3-bit
  // top window piles n/8 points into each of its buckets) nor carries out (r >> 240 = 0x73ed: with c = 15 nearly half
  // of the scalars would carry into one bucket of an 18th window). 8, 13 and 16 leave top digits < 2^(c-1).
  const int lg = ilog2_floor(n);
  const int c = lg <= 9 ? 5 : (lg <= 12 ? 8 : (lg <= 15 ? 13 : 16));
  // signed digits |d| <= 2^(c-1): one more bit than the 256 of the scalar for the last carry
  const int windows = (32 * msm::SCALAR_WORDS + 1 + c - 1) / c;
  const size_t nb = ((size_t)1 << (c - 1)) + 1;                             // bucket indices 0 .. 2^(c-1)
  // buckets per k_segment_reduce lane: each lane pays ~22 point operations for its multiple of the run total on top
  // of 2 per bucket, and a point operation keeps a SIMD busy for ~27 us whatever the occupancy: 16 measured best once
  // there are more runs than SIMD lanes, 8 below
  const size_t seg_len = c >= 13 ? 16 : 8;
  const size_t nbs = (nb + seg_len - 1) / seg_len * seg_len, segs = nbs / seg_len;  // padded to whole runs
  const size_t total = (size_t)windows * nbs;
  // a bucket is "heavy" (summed by a workgroup) above HEAVY << hs points: at least 4x the mean n / 2^(c-1) of uniform scalars
  int hs = 0;
  while (((size_t)msm::HEAVY << hs) < 4 * (n >> (c - 1))) hs++;
  const size_t max_heavy = (size_t)windows * (n / ((size_t)msm::HEAVY << hs) + 1);  // ... so there are at most this many,
  const size_t max_chunks = (size_t)windows * (n / msm::HEAVY_CHUNK) + max_heavy;       // in at most this many chunks
  // point sets of 2^18 and more sort through LDS-privatised counters (msm.h): at least 16 tiles per window, tiles of
  // 2^18 scalars from 2^22 points on (measured faster than one global atomic per scalar and window from 2^18 up)
  const bool tiled = n >= ((size_t)1 << 18) && nbs <= (size_t)msm::TILE_NBS;
  const size_t tiles = tiled ? ((n >> 18) > 16 ? (n >> 18) : 16) : 0, tile = tiled ? (n + tiles - 1) / tiles : 0;
  const size_t sizes[] = {8, max_heavy * sizeof(msm::HeavyBucket), total * 4, total * 4, total * 4,
                          (size_t)windows * n * 4, 2 * msm::SIZE_BINS * 4, total * 4, total * sizeof(J), windows * segs * sizeof(J),
                          tiled ? (size_t)windows * n * 4 : 0, max_chunks * sizeof(msm::HeavyChunk), max_chunks * sizeof(J)};
  DevBufs D;
  for (size_t b : sizes) D.plan(b);
  CP_TRY(D.commit(ctx));
  uint32_t *heavy_head = D.take<uint32_t>(sizes[0]), *counts;
  msm::HeavyBucket *heavy = D.take<msm::HeavyBucket>(sizes[1]);
  counts = D.take<uint32_t>(sizes[2]);
  uint32_t *offsets = D.take<uint32_t>(sizes[3]), *cursor = D.take<uint32_t>(sizes[4]), *sorted = D.take<uint32_t>(sizes[5]);
  uint32_t *size_bins = D.take<uint32_t>(sizes[6]), *size_cursor = size_bins + msm::SIZE_BINS, *order = D.take<uint32_t>(sizes[7]);
  J *buckets = D.take<J>(sizes[8]), *seg = D.take<J>(sizes[9]);
  int32_t *digits = D.take<int32_t>(sizes[10]);
  msm::HeavyChunk *chunks = D.take<msm::HeavyChunk>(sizes[11]);
  J *chunk_sums = D.take<J>(sizes[12]);
  HIP_TRY(ctx, hipMemsetAsync(counts, 0, total * 4, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(heavy_head, 0, 8, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(size_bins, 0, 2 * msm::SIZE_BINS * 4, ctx->stream));
  if (tiled) {
    LAUNCH(ctx, "msm_digits", msm::k_digits, dim3(blocks_for(n, 256)), dim3(256), scalars, inf, n, c, windows, digits);
    LAUNCH(ctx, "msm_hist", msm::k_hist_tiled, dim3((unsigned)tiles, windows), dim3(1024), digits, n, tile, nbs, counts);
  } else {
    LAUNCH(ctx, "msm_hist", msm::k_hist, dim3(blocks_for(n, 256)), dim3(256), scalars, inf, n, c, windows, nbs, counts);
  }
  LAUNCH(ctx, "msm_scan", msm::k_scan, dim3(windows), dim3(1024), counts, nbs, offsets, cursor);
  if (tiled)
    LAUNCH(ctx, "msm_scatter", msm::k_scatter_tiled, dim3((unsigned)tiles, windows), dim3(1024), digits, n, tile, nbs, cursor, sorted);
  else
    LAUNCH(ctx, "msm_scatter", msm::k_scatter, dim3(blocks_for(n, 256)), dim3(256), scalars, inf, n, c, windows, nbs, cursor, sorted);
  LAUNCH(ctx, "msm_size_sort", msm::k_size_hist, dim3(blocks_for(total, 256)), dim3(256), counts, total, hs, size_bins);
  LAUNCH(ctx, "msm_size_sort", msm::k_size_scan, dim3(1), dim3(64), size_bins, size_cursor);
  LAUNCH(ctx, "msm_size_sort", msm::k_size_scatter, dim3(blocks_for(total, 256)), dim3(256), counts, total, hs, size_cursor, order);
  LAUNCH(ctx, "msm_bucket_sum", msm::k_bucket_sum<F>, dim3(blocks_for(total, 128)), dim3(128), pts, counts, offsets, sorted, order, total,
         n, nbs, hs, buckets);
  LAUNCH(ctx, "msm_heavy_list", msm::k_heavy_list, dim3(blocks_for(total, 256)), dim3(256), counts, total, hs, heavy_head, heavy, chunks);
  LAUNCH(ctx, "msm_heavy_sum", msm::k_heavy_sum<F>, dim3((unsigned)max_chunks), dim3(msm::HEAVY_LANES<F>), pts, offsets, sorted, n, nbs,
         heavy_head, chunks, chunk_sums);
  LAUNCH(ctx, "msm_heavy_sum", msm::k_heavy_combine<F>, dim3((unsigned)max_heavy), dim3(msm::HEAVY_LANES<F>), heavy_head, heavy, chunk_sums,
         buckets);
  LAUNCH(ctx, "msm_segment_reduce", msm::k_segment_reduce<F>, dim3(blocks_for(segs, 64), windows), dim3(64), buckets, nbs, (uint32_t)seg_len, seg);
  for (size_t m = segs; m > 1;) {
    const size_t half = (m + 1) / 2;
    LAUNCH(ctx, "msm_pair_reduce", msm::k_pair_reduce<F>, dim3(blocks_for(half, 64), windows), dim3(64), seg, (uint32_t)segs, (uint32_t)m,
           (uint32_t)half);
    m = half;
  }
  std::vector<J> win(windows);
  HIP_TRY(ctx, hipMemcpy2DAsync(win.data(), sizeof(J), seg, segs * sizeof(J), sizeof(J), windows, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // sum_w 2^(c w) S_w, Horner from the top window (a few hundred point operations: host)
  J r = win[windows - 1];
  for (int w = windows - 2; w >= 0; w--) {
    for (int i = 0; i < c; i++) r = bls::jac_double(r);
    r = bls::jac_add(r, win[w]);
  }
  *result = r;
  return CP_OK;
}

template <class F>
void jac_out(const bls::JacT<F> &r, uint64_t *out_xy, int *out_inf) {
  uint32_t w[2 * bls::Field<F>::WORDS];
  const bool inf = bls::jac_to_affine_canonical(r, w);
  memcpy(out_xy, w, 2 * bls::Field<F>::WORDS * 4);
  *out_inf = inf ? 1 : 0;
}

bool canonical_words(const uint32_t *w) {  // 12 words < p ?
  for (int k = 11; k >= 0; k--) {
    if (w[k] < BLS_P32[k]) return true;
    if (w[k] > BLS_P32[k]) return false;
  }
  return false;
}

template <class F>
int msm_prepare_dev(cp_ctx *ctx, const uint64_t *points_xy_dev, size_t n, void *points_mont_dev) {
  CHECK_CTX(ctx);
  if (n == 0) return CP_OK;
  if (!points_xy_dev || !points_mont_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL pointer");
  LAUNCH(ctx, "msm_points_to_mont", msm::k_points_to_mont<F>, dim3(blocks_for(n, 128)), dim3(128), (const uint32_t *)points_xy_dev, n,
         (bls::AffineT<F> *)points_mont_dev);
  return CP_OK;
}

template <class F>
int msm_dev(cp_ctx *ctx, const uint64_t *scalars_dev, const void *points_mont_dev, const uint8_t *inf_dev, size_t n, uint64_t *out_xy,
            int *out_is_infinity) {
  CHECK_CTX(ctx);
  if (!out_xy || !out_is_infinity) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL output");
  if (n > ((size_t)1 << 28)) return set_error(ctx, CP_ERR_INVALID_ARG, "MSM of %zu points is too large (max 2^28)", n);
  if (n && (!scalars_dev || !points_mont_dev)) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL pointer");
  bls::JacT<F> r;
  CP_TRY(msm_run<F>(ctx, (const uint32_t *)scalars_dev, (const bls::AffineT<F> *)points_mont_dev, inf_dev, n, &r));
  jac_out<F>(r, out_xy, out_is_infinity);
  return CP_OK;
}

template <class F>
int msm_host(cp_ctx *ctx, const uint64_t *scalars_host, const uint64_t *points_xy_host, const uint8_t *points_inf_host, size_t n,
             uint64_t *out_xy, int *out_is_infinity) {
  CHECK_CTX(ctx);
  if (!out_xy || !out_is_infinity) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL output");
  if (n > ((size_t)1 << 28)) return set_error(ctx, CP_ERR_INVALID_ARG, "MSM of %zu points is too large (max 2^28)", n);
  if (n && (!scalars_host || !points_xy_host)) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL pointer");
  constexpr size_t PW = 2 * bls::Field<F>::WORDS;  // 32-bit words per affine point at the API
  bls::JacT<F> r = bls::jac_inf<F>();
  if (n) {
    // coordinates must be canonical: a value >= p would silently alias another point
    for (size_t i = 0; i < n; i++) {
      if (points_inf_host && points_inf_host[i]) continue;
      const uint32_t *w = (const uint32_t *)points_xy_host + PW * i;
      for (size_t h = 0; h < PW / 12; h++)
        if (!canonical_words(w + 12 * h)) return set_error(ctx, CP_ERR_INVALID_ARG, "point %zu: coordinate is not canonical (>= p)", i);
    }
    DevBag D = ctx->bag();  // device copies of the host inputs: freed when the call ends, on every path
    uint64_t *d_s, *d_xy;
    bls::AffineT<F> *d_m;
    uint8_t *d_inf = nullptr;
    CP_TRY(alloc_status(ctx, D.alloc(&d_s, n * 32), n * 32));
    CP_TRY(alloc_status(ctx, D.alloc(&d_xy, n * PW * 4), n * PW * 4));
    CP_TRY(alloc_status(ctx, D.alloc(&d_m, n * sizeof(bls::AffineT<F>)), n * sizeof(bls::AffineT<F>)));
    HIP_TRY(ctx, hipMemcpyAsync(d_s, scalars_host, n * 32, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_xy, points_xy_host, n * PW * 4, hipMemcpyHostToDevice, ctx->stream));
    if (points_inf_host) {
      CP_TRY(alloc_status(ctx, D.alloc(&d_inf, n), n));
      HIP_TRY(ctx, hipMemcpyAsync(d_inf, points_inf_host, n, hipMemcpyHostToDevice, ctx->stream));
    }
    CP_TRY(msm_prepare_dev<F>(ctx, d_xy, n, d_m));
    CP_TRY(msm_run<F>(ctx, (const uint32_t *)d_s, d_m, d_inf, n, &r));
  }
  jac_out<F>(r, out_xy, out_is_infinity);
  return CP_OK;
}

template <class F>
int msm_synthetic(cp_ctx *ctx, const uint64_t *generator_xy, uint32_t a, uint32_t b, size_t n, void *points_mont_dev) {
  CHECK_CTX(ctx);
  if (n == 0) return CP_OK;
  if (!generator_xy || !points_mont_dev) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL pointer");
  if (a == 0 || a > 65535 || b == 0 || b > 65535 || n > ((size_t)1 << 28))
    return set_error(ctx, CP_ERR_INVALID_ARG, "synthetic points: a, b must be in [1, 65535], n <= 2^28 (a*i + b must stay far below the group order)");
  const bls::AffineT<F> g = bls::affine_from_canonical<F>((const uint32_t *)generator_xy);
  if (!bls::affine_on_curve(g)) return set_error(ctx, CP_ERR_INVALID_ARG, "generator is not on the curve");
  LAUNCH(ctx, "msm_synthetic_points", msm::k_synthetic_points<F>, dim3(blocks_for(n, 64)), dim3(64), g, a, b, n,
         (bls::AffineT<F> *)points_mont_dev);
  return CP_OK;
}

}  // namespace

extern "C" {

int cp_msm_bls12381_g1_prepare_dev(cp_ctx *ctx, const uint64_t *points_xy_dev, size_t n, void *points_mont_dev) try {
  return msm_prepare_dev<bls::Fp>(ctx, points_xy_dev, n, points_mont_dev);
} CP_CATCH(ctx)
int cp_msm_bls12381_g1_synthetic_points_dev(cp_ctx *ctx, const uint64_t generator_xy[12], uint32_t a, uint32_t b, size_t n,
                                            void *points_mont_dev) try {
  return msm_synthetic<bls::Fp>(ctx, generator_xy, a, b, n, points_mont_dev);
} CP_CATCH(ctx)
int cp_msm_bls12381_g1_dev(cp_ctx *ctx, const uint64_t *scalars_dev, const void *points_mont_dev, const uint8_t *inf_dev, size_t n,
                           uint64_t out_xy[12], int *out_is_infinity) try {
  return msm_dev<bls::Fp>(ctx, scalars_dev, points_mont_dev, inf_dev, n, out_xy, out_is_infinity);
} CP_CATCH(ctx)
int cp_msm_bls12381_g1(cp_ctx *ctx, const uint64_t *scalars_host, const uint64_t *points_xy_host, const uint8_t *points_inf_host,
                       size_t n, uint64_t out_xy[12], int *out_is_infinity) try {
  return msm_host<bls::Fp>(ctx, scalars_host, points_xy_host, points_inf_host, n, out_xy, out_is_infinity);
} CP_CATCH(ctx)

int cp_msm_bls12381_g2_prepare_dev(cp_ctx *ctx, const uint64_t *points_xy_dev, size_t n, void *points_mont_dev) try {
  return msm_prepare_dev<bls::Fp2>(ctx, points_xy_dev, n, points_mont_dev);
} CP_CATCH(ctx)
int cp_msm_bls12381_g2_synthetic_points_dev(cp_ctx *ctx, const uint64_t generator_xy[24], uint32_t a, uint32_t b, size_t n,
                                            void *points_mont_dev) try {
  return msm_synthetic<bls::Fp2>(ctx, generator_xy, a, b, n, points_mont_dev);
} CP_CATCH(ctx)
int cp_msm_bls12381_g2_dev(cp_ctx *ctx, const uint64_t *scalars_dev, const void *points_mont_dev, const uint8_t *inf_dev, size_t n,
                           uint64_t out_xy[24], int *out_is_infinity) try {
  return msm_dev<bls::Fp2>(ctx, scalars_dev, points_mont_dev, inf_dev, n, out_xy, out_is_infinity);
} CP_CATCH(ctx)
int cp_msm_bls12381_g2(cp_ctx *ctx, const uint64_t *scalars_host, const uint64_t *points_xy_host, const uint8_t *points_inf_host,
                       size_t n, uint64_t out_xy[24], int *out_is_infinity) try {
  return msm_host<bls::Fp2>(ctx, scalars_host, points_xy_host, points_inf_host, n, out_xy, out_is_infinity);
} CP_CATCH(ctx)

}  // extern "C"
