// Groth16 proof assembly over BLS12-381 from a proving key given as point sets (SURVEY.md §8(a) A12: what gnark's
// `groth16.Prove` does after the witness is solved; reached in the reference through
// `gnark_plonky2_wrapper::wrap_plonky2_proof`, city_rollup_circuit/src/worker/toolbox/root.rs:296-304).
// Restated from the Groth16 paper / gnark's prover (UPSTREAM-MEMORY; no proving key, circuit or vectors in the tree:
// parity unpinned — the tests check the proof against the trapdoor of a setup they generate themselves).
//   A  = alpha_1 + sum_i w_i A_i + r delta_1
//   B  = beta_2  + sum_i w_i B_i + s delta_2            (G2; B1 = the same in G1)
//   C  = sum_{i private} w_i K_i + sum_j h_j Z_j + s A + r B1 - r s delta_1
// h = (a o b - c) / (x^n - 1) from the evaluations of A w, B w, C w on the domain (cp_groth16_quotient).
// The five MSMs and the quotient run on the device; the dozen remaining point operations on the host.
// Included by cityprover.hip after msm.inc and fr_ntt.inc.
namespace {

template <class F>
bls::JacT<F> jac_mul_scalar(const bls::JacT<F> &p, const uint64_t k[4]) {  // double-and-add over 256 bits (host)
  bls::JacT<F> r = bls::jac_inf<F>();
  for (int i = 255; i >= 0; i--) {
    r = bls::jac_double(r);
    if ((k[i >> 6] >> (i & 63)) & 1) r = bls::jac_add(r, p);
  }
  return r;
}
template <class F>
int point_in(cp_ctx *ctx, const uint64_t *xy, const char *name, bls::JacT<F> *out) {
  constexpr size_t W = bls::Field<F>::WORDS;
  const uint32_t *w = (const uint32_t *)xy;
  for (size_t h = 0; h < 2 * W / 12; h++)
    if (!canonical_words(w + 12 * h)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: coordinate is not canonical (>= p)", name);
  const bls::AffineT<F> a = bls::affine_from_canonical<F>(w);
  if (!bls::affine_on_curve(a)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s is not on the curve", name);
  *out = {a.x, a.y, bls::Field<F>::one()};
  return CP_OK;
}

}  // namespace

extern "C" int cp_groth16_prove_bls12381(cp_ctx *ctx, const cp_groth16_pk *pk, const uint64_t *witness_dev, uint64_t *a_evals_dev,
                                         uint64_t *b_evals_dev, uint64_t *c_evals_dev, const uint64_t r[4], const uint64_t s[4],
                                         uint64_t out_a[12], uint64_t out_b[24], uint64_t out_c[12]) try {
  CHECK_CTX(ctx);
  if (!pk || !witness_dev || !a_evals_dev || !b_evals_dev || !c_evals_dev || !r || !s || !out_a || !out_b || !out_c)
    return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (!pk->a_g1 || !pk->b_g1 || !pk->b_g2 || !pk->k_g1 || !pk->z_g1) return set_error(ctx, CP_ERR_INVALID_ARG, "proving key: NULL point set");
  if (pk->log_domain < 1 || pk->log_domain > 28) return set_error(ctx, CP_ERR_INVALID_ARG, "proving key: log_domain %d out of range", pk->log_domain);
  if (pk->n_wires == 0 || pk->n_private > pk->n_wires) return set_error(ctx, CP_ERR_INVALID_ARG, "proving key: bad wire counts");
  if (!blsfr::fr_is_canonical((const uint32_t *)r) || !blsfr::fr_is_canonical((const uint32_t *)s))
    return set_error(ctx, CP_ERR_INVALID_ARG, "r / s are not canonical scalars");
  using J1 = bls::JacT<bls::Fp>;
  using J2 = bls::JacT<bls::Fp2>;
  J1 alpha1, beta1, delta1;
  J2 beta2, delta2;
  CP_TRY(point_in<bls::Fp>(ctx, pk->alpha_g1, "alpha_g1", &alpha1));
  CP_TRY(point_in<bls::Fp>(ctx, pk->beta_g1, "beta_g1", &beta1));
  CP_TRY(point_in<bls::Fp>(ctx, pk->delta_g1, "delta_g1", &delta1));
  CP_TRY(point_in<bls::Fp2>(ctx, pk->beta_g2, "beta_g2", &beta2));
  CP_TRY(point_in<bls::Fp2>(ctx, pk->delta_g2, "delta_g2", &delta2));
  const size_t n = (size_t)1 << pk->log_domain, n_pub = pk->n_wires - pk->n_private;
  // Two independent chains on two contexts (this one and a lane of it: own stream and MSM workspace), so that the
  // latency-bound reduction tails of one MSM (a few thousand waves) run under the bucket sums of the next:
  //   here:  A, B1, quotient, Z          lane:  B2 (G2), K
  J1 sa, sb1, sk, sz;
  J2 sb2;
  if (ctx->lanes.empty() && !ctx->parent) {
    cp_ctx *lane = cp_ctx_create(ctx->device);
    if (!lane) return lane_error(ctx);
    lane->parent = ctx;
    ctx->lanes.push_back(lane);
  }
  cp_ctx *side = ctx->parent ? nullptr : ctx->lanes[0];
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // inputs written on this stream are complete before the lane reads them
  int side_rc = CP_OK;
  auto side_chain = [&](cp_ctx *c) -> int {
    CP_TRY(msm_run<bls::Fp2>(c, (const uint32_t *)witness_dev, (const bls::Affine2 *)pk->b_g2, pk->b_inf, pk->n_wires, &sb2));
    CP_TRY(msm_run<bls::Fp>(c, (const uint32_t *)(witness_dev + 4 * n_pub), (const bls::Affine *)pk->k_g1, nullptr, pk->n_private, &sk));
    return CP_OK;
  };
  // the multiples of delta depend on the key and the blinding only: a host thread computes them under the MSMs
  J1 r_delta1, s_delta1, rs_delta1;
  J2 s_delta2;
  auto delta_work = [&]() noexcept {
    r_delta1 = jac_mul_scalar(delta1, r);
    s_delta1 = jac_mul_scalar(delta1, s);
    rs_delta1 = jac_mul_scalar(r_delta1, s);
    s_delta2 = jac_mul_scalar(delta2, s);
  };
  auto side_work = [&]() noexcept {
    try {
      side_rc = hipSetDevice(side->device) == hipSuccess ? side_chain(side) : CP_ERR_HIP;
    } catch (...) {
      side_rc = exception_status(side);
    }
  };
  // both helpers are joined on every exit path; one that cannot be started is run on this thread instead
  hostu::Joiner delta_thread, side_thread;
  const bool delta_started = hostu::try_spawn(delta_thread.t, delta_work);
  const bool side_started = side && hostu::try_spawn(side_thread.t, side_work);
  auto main_chain = [&]() -> int {
    CP_TRY(msm_run<bls::Fp>(ctx, (const uint32_t *)witness_dev, (const bls::Affine *)pk->a_g1, pk->a_inf, pk->n_wires, &sa));
    CP_TRY(msm_run<bls::Fp>(ctx, (const uint32_t *)witness_dev, (const bls::Affine *)pk->b_g1, pk->b_inf, pk->n_wires, &sb1));
    // h and its MSM over the powers-of-tau points Z_j = tau^j (tau^n - 1) / delta, j < n - 1
    CP_TRY(groth16_quotient_run(ctx, a_evals_dev, b_evals_dev, c_evals_dev, pk->log_domain));
    CP_TRY(msm_run<bls::Fp>(ctx, (const uint32_t *)a_evals_dev, (const bls::Affine *)pk->z_g1, nullptr, n - 1, &sz));
    return CP_OK;
  };
  const int main_rc = main_chain();
  if (side_started) side_thread.t.join();
  else if (side) { side_work(); (void)hipSetDevice(ctx->device); }
  else side_rc = side_chain(ctx);
  if (delta_started) delta_thread.t.join();
  else delta_work();
  if (main_rc != CP_OK) return main_rc;
  if (side_rc != CP_OK) return set_error(ctx, side_rc, "%s", side ? side->error.c_str() : ctx->error.c_str());
  // assembly
  const J1 A = bls::jac_add(bls::jac_add(alpha1, sa), r_delta1);
  const J2 B = bls::jac_add(bls::jac_add(beta2, sb2), s_delta2);
  const J1 B1 = bls::jac_add(bls::jac_add(beta1, sb1), s_delta1);
  J1 C = bls::jac_add(sk, sz);
  C = bls::jac_add(C, jac_mul_scalar(A, s));
  C = bls::jac_add(C, jac_mul_scalar(B1, r));
  C = bls::jac_add(C, bls::jac_neg(rs_delta1));
  int inf_a, inf_b, inf_c;
  jac_out<bls::Fp>(A, out_a, &inf_a);
  jac_out<bls::Fp2>(B, out_b, &inf_b);
  jac_out<bls::Fp>(C, out_c, &inf_c);
  if (inf_a || inf_b || inf_c) return set_error(ctx, CP_ERR_INTERNAL, "a proof element is the point at infinity");
  return CP_OK;
} CP_CATCH(ctx)
