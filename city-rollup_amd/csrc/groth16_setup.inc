// Groth16 setup over BLS12-381: from a constraint system and the five trapdoor scalars to a device-resident proving key and
// a verifying key (the step the reference takes once per circuit: `gnark_plonky2_wrapper::initialize`,
// city_rollup_core_worker/src/lib.rs:37-38; the arithmetic is gnark's `groth16.Setup`, outside the tree: parity unpinned, the
// tests hold every point against [its logarithm] G from the trapdoor). With the domain <omega> of 2^L >= n_constraints points:
//   L_j(tau)                          the inverse F_r transform of (tau^k)_k, since tau^k = sum_j L_j(tau) omega^(j k)
//   u_i, v_i, w_i = (A^T L)_i, ...    r1cs_eval of the system transposed on the host, with L as its witness
//   k_i, ic_i, z_j                    two element-wise kernels (groth16_setup.h)
//   the five point sets               fixed_base_run (fixed_base.inc) over the standard generators
// Included by bls.hip after fixed_base.inc and r1cs.inc. The handle itself is groth16_key.h: key files make one too.
#include "groth16_key.h"

namespace {

int trapdoor_scalar(cp_ctx *ctx, const uint64_t s[4], const char *name, blsfr::Fr *out) {
  if (!(s[0] | s[1] | s[2] | s[3])) return set_error(ctx, CP_ERR_INVALID_ARG, "trapdoor: %s is zero", name);
  if (!blsfr::fr_is_canonical((const uint32_t *)s)) return set_error(ctx, CP_ERR_INVALID_ARG, "trapdoor: %s is not canonical (>= r)", name);
  *out = blsfr::fr_from_canonical((const uint32_t *)s);
  return CP_OK;
}

template <class F>
void scalar_multiple_out(const bls::JacT<F> &g, const uint64_t k[4], uint64_t *out_xy) {
  int inf;
  jac_out<F>(jac_mul_scalar(g, k), out_xy, &inf);  // k is non-zero and below r, g has order r: never infinity
}

int groth16_setup_run(cp_ctx *ctx, const cp_r1cs_desc *sys, size_t n_public, const cp_groth16_trapdoor *td, cp_groth16_key *key) {
  using blsfr::Fr;
  // ---- every refusal that needs no device ----
  host_phase(ctx, "setup_validate");  // the host phases are clocked when profiling is on (cp_profile_begin)
  Fr tau, alpha, beta, gamma, delta;
  CP_TRY(trapdoor_scalar(ctx, td->tau, "tau", &tau));
  CP_TRY(trapdoor_scalar(ctx, td->alpha, "alpha", &alpha));
  CP_TRY(trapdoor_scalar(ctx, td->beta, "beta", &beta));
  CP_TRY(trapdoor_scalar(ctx, td->gamma, "gamma", &gamma));
  CP_TRY(trapdoor_scalar(ctx, td->delta, "delta", &delta));
  CP_TRY(r1cs_validate(ctx, sys));
  const size_t n = sys->n_constraints, m = sys->n_wires;
  if (n_public == 0 || n_public > m) return set_error(ctx, CP_ERR_INVALID_ARG, "setup: n_public %zu out of range (1 .. n_wires = %zu; it counts wire 0)", n_public, m);
  if (n < 2) return set_error(ctx, CP_ERR_INVALID_ARG, "setup: a system of one constraint has a domain of one point (log_domain 0), which the prover does not take");
  if (m > ((size_t)1 << 28)) return set_error(ctx, CP_ERR_INVALID_ARG, "setup: n_wires %zu out of range (1 .. 2^28)", m);
  int log_domain = 0;
  while (((size_t)1 << log_domain) < n) log_domain++;
  const size_t N = (size_t)1 << log_domain, n_private = m - n_public;
  const Fr zt = blsfr::fr_sub(blsfr::fr_pow_u64(tau, N), blsfr::fr_one());  // tau^N - 1
  bool zt_zero = true;
  for (int l = 0; l < blsfr::NL; l++) zt_zero = zt_zero && zt.l[l] == 0;
  if (zt_zero) return set_error(ctx, CP_ERR_INVALID_ARG, "trapdoor: tau^(2^%d) = 1: tau lies in the evaluation domain", log_domain);
  // ---- the three matrices transposed: rows are wires, columns constraints ----
  host_phase(ctx, "setup_transpose");
  g16setup::Csr T[3];
  const cp_r1cs_matrix *mats[3] = {&sys->a, &sys->b, &sys->c};
  for (int k = 0; k < 3; k++) g16setup::transpose_csr(mats[k]->row_ptr, mats[k]->col, mats[k]->coeff, n, m, T[k]);
  for (size_t i = n_public; i < m; i++)
    if (T[0].row_ptr[i] == T[0].row_ptr[i + 1] && T[1].row_ptr[i] == T[1].row_ptr[i + 1] && T[2].row_ptr[i] == T[2].row_ptr[i + 1])
      return set_error(ctx, CP_ERR_INVALID_ARG, "setup: private wire %zu occurs in no constraint: its key point would be the point at infinity", i);
  cp_r1cs_desc dT{};
  dT.n_constraints = m;
  dT.n_wires = n;
  dT.coeffs = sys->coeffs;
  dT.n_coeffs = sys->n_coeffs;
  dT.flags = sys->flags;
  cp_r1cs_matrix *mt[3] = {&dT.a, &dT.b, &dT.c};
  for (int k = 0; k < 3; k++) *mt[k] = cp_r1cs_matrix{T[k].row_ptr.data(), T[k].col.data(), T[k].coeff.data()};
  // ---- Lagrange values, QAP columns, key scalars: temporaries of this call ----
  host_phase(ctx, "setup_columns");
  DevBag tmp = ctx->bag();
  uint64_t *lag = nullptr, *uvw[3] = {nullptr, nullptr, nullptr}, *scal = nullptr;
  unsigned long long *zero_wire = nullptr;
  CP_TRY(alloc_status(ctx, tmp.alloc(&lag, N * 32), N * 32));
  LAUNCH(ctx, "setup_tau_powers", g16setup::k_scaled_powers, dim3(blocks_for(N, 256)), dim3(256), tau, blsfr::fr_one(), N, (uint32_t *)lag);
  CP_TRY(fr_ntt_run(ctx, lag, log_domain, CP_NTT_INVERSE, nullptr));
  {
    cp_r1cs_bls12381 *h = new cp_r1cs_bls12381(ctx->device);
    struct Guard { cp_r1cs_bls12381 *h; ~Guard() { r1cs_free(h); } } guard{h};  // gone before the point sets are allocated
    CP_TRY(r1cs_build(ctx, &dT, h));
    for (auto &t : T) t = g16setup::Csr();
    const size_t bytes = h->sys.n_pad * 32;
    for (auto &p : uvw) CP_TRY(alloc_status(ctx, tmp.alloc(&p, bytes), bytes));
    CP_TRY(r1cs_eval_run(ctx, h, lag, r1cs::Outputs{{(uint32_t *)uvw[0], (uint32_t *)uvw[1], (uint32_t *)uvw[2]}}, nullptr));
    HIP_TRY(ctx, sync_stream(ctx));  // the handle's arrays are no longer read
  }
  CP_TRY(alloc_status(ctx, tmp.alloc(&scal, m * 32), m * 32));
  CP_TRY(alloc_status(ctx, tmp.alloc(&zero_wire, 8), 8));
  HIP_TRY(ctx, hipMemsetAsync(zero_wire, 0xff, 8, ctx->stream));
  const Fr gamma_inv = blsfr::fr_inv(gamma), delta_inv = blsfr::fr_inv(delta);
  LAUNCH(ctx, "setup_key_scalars", g16setup::k_key_scalars, dim3(blocks_for(m, 256)), dim3(256), (const uint32_t *)uvw[0], (const uint32_t *)uvw[1],
         (const uint32_t *)uvw[2], beta, alpha, gamma_inv, delta_inv, n_public, m, (uint32_t *)scal, zero_wire);
  // the Lagrange values have been read (stream order): their array takes z_j = tau^j (tau^N - 1) / delta, j < N - 1
  LAUNCH(ctx, "setup_z_scalars", g16setup::k_scaled_powers, dim3(blocks_for(N - 1, 256)), dim3(256), tau, blsfr::fr_mul(zt, delta_inv), N - 1,
         (uint32_t *)lag);
  unsigned long long first_zero = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&first_zero, zero_wire, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (first_zero != ~0ull)
    return set_error(ctx, CP_ERR_INVALID_ARG, "setup: private wire %llu has beta u + alpha v + w = 0 at tau: its key point would be the point at infinity", first_zero);
  // ---- the point sets: buffers of the key ----
  host_phase(ctx, "setup_points");
  void *a_g1, *b_g1, *b_g2, *k_g1, *z_g1, *a_inf, *b_inf;
  uint8_t *no_inf = nullptr, *ic_inf = nullptr;
  void *ic_pts = nullptr;
  struct Want { void **p; size_t bytes; } wants[] = {{&a_g1, m * CP_G1_AFFINE_BYTES}, {&b_g1, m * CP_G1_AFFINE_BYTES}, {&b_g2, m * CP_G2_AFFINE_BYTES},
                                                     {&k_g1, (n_private ? n_private : 1) * CP_G1_AFFINE_BYTES}, {&z_g1, (N - 1) * CP_G1_AFFINE_BYTES},
                                                     {&a_inf, (m + 7) & ~(size_t)7}, {&b_inf, (m + 7) & ~(size_t)7}};  // whole u64: callers copy words
  for (const Want &w : wants) CP_TRY(alloc_status(ctx, key->mem.alloc(w.p, w.bytes), w.bytes));
  const size_t no_inf_bytes = n_private > N ? n_private : N;  // flags of the sets that have none (all zero: checked above, and z_j != 0)
  CP_TRY(alloc_status(ctx, tmp.alloc(&no_inf, no_inf_bytes), no_inf_bytes));
  CP_TRY(alloc_status(ctx, tmp.alloc(&ic_pts, n_public * CP_G1_AFFINE_BYTES), n_public * CP_G1_AFFINE_BYTES));
  CP_TRY(alloc_status(ctx, tmp.alloc(&ic_inf, n_public), n_public));
  HIP_TRY(ctx, hipMemsetAsync(a_inf, 0, (m + 7) & ~(size_t)7, ctx->stream));  // the padding of the last word
  HIP_TRY(ctx, hipMemsetAsync(b_inf, 0, (m + 7) & ~(size_t)7, ctx->stream));
  CP_TRY(fixed_base_run<bls::Fp>(ctx, BLS_G1_GEN, uvw[0], m, a_g1, (uint8_t *)a_inf));
  CP_TRY(fixed_base_run<bls::Fp>(ctx, BLS_G1_GEN, uvw[1], m, b_g1, (uint8_t *)b_inf));
  CP_TRY(fixed_base_run<bls::Fp2>(ctx, BLS_G2_GEN, uvw[1], m, b_g2, (uint8_t *)b_inf));  // the same flags again
  if (n_private) CP_TRY(fixed_base_run<bls::Fp>(ctx, BLS_G1_GEN, scal + 4 * n_public, n_private, k_g1, no_inf));
  CP_TRY(fixed_base_run<bls::Fp>(ctx, BLS_G1_GEN, lag, N - 1, z_g1, no_inf));
  CP_TRY(fixed_base_run<bls::Fp>(ctx, BLS_G1_GEN, scal, n_public, ic_pts, ic_inf));
  // the six single points on the host, under the kernels
  bls::Jac g1;
  bls::Jac2 g2;
  CP_TRY(point_in<bls::Fp>(ctx, BLS_G1_GEN, "the G1 generator", &g1));
  CP_TRY(point_in<bls::Fp2>(ctx, BLS_G2_GEN, "the G2 generator", &g2));
  cp_groth16_pk &pk = key->pk;
  cp_groth16_vk &vk = key->vk;
  scalar_multiple_out(g1, td->alpha, pk.alpha_g1);
  scalar_multiple_out(g1, td->beta, pk.beta_g1);
  scalar_multiple_out(g1, td->delta, pk.delta_g1);
  scalar_multiple_out(g2, td->beta, pk.beta_g2);
  scalar_multiple_out(g2, td->delta, pk.delta_g2);
  scalar_multiple_out(g2, td->gamma, vk.gamma_g2);
  memcpy(vk.alpha_g1, pk.alpha_g1, sizeof vk.alpha_g1);
  memcpy(vk.beta_g2, pk.beta_g2, sizeof vk.beta_g2);
  memcpy(vk.delta_g2, pk.delta_g2, sizeof vk.delta_g2);
  vk.n_public = n_public;
  pk.n_wires = m;
  pk.n_private = n_private;
  pk.log_domain = log_domain;
  pk.a_g1 = a_g1; pk.b_g1 = b_g1; pk.b_g2 = b_g2; pk.k_g1 = k_g1; pk.z_g1 = z_g1;
  pk.a_inf = (const uint8_t *)a_inf; pk.b_inf = (const uint8_t *)b_inf;
  std::vector<bls::Affine> ic(n_public);
  key->ic_inf.resize(n_public);
  key->ic_xy.resize(12 * n_public);
  HIP_TRY(ctx, hipMemcpyAsync(ic.data(), ic_pts, n_public * sizeof(bls::Affine), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(key->ic_inf.data(), ic_inf, n_public, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n_public; i++) {
    uint32_t w[24];
    bls::fp_to_canonical(ic[i].x, w);
    bls::fp_to_canonical(ic[i].y, w + 12);
    memcpy(&key->ic_xy[12 * i], w, sizeof w);
  }
  host_phase(ctx, nullptr);
  return CP_OK;
}

}  // namespace

extern "C" {

cp_groth16_key *cp_groth16_setup_bls12381(cp_ctx *ctx, const cp_r1cs_desc *system, size_t n_public, const cp_groth16_trapdoor *trapdoor) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  if (!system || !trapdoor) { set_error(ctx, CP_ERR_INVALID_ARG, "setup: NULL argument"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  cp_groth16_key *key = new cp_groth16_key(ctx->device);
  struct Guard { cp_groth16_key *k; ~Guard() { groth16_key_free(k); } } guard{key};
  if (groth16_setup_run(ctx, system, n_public, trapdoor, key) != CP_OK) return nullptr;
  guard.k = nullptr;
  return key;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

void cp_groth16_key_destroy(cp_groth16_key *key) try {
  groth16_key_free(key);
} catch (...) {
}

int cp_groth16_key_pk(const cp_groth16_key *key, cp_groth16_pk *out) try {
  if (!key || !out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  *out = key->pk;
  return CP_OK;
} CP_CATCH(nullptr)

int cp_groth16_key_vk(const cp_groth16_key *key, cp_groth16_vk *out, uint64_t *ic_xy_out, uint8_t *ic_inf_out) try {
  if (!key || !out) return set_error(nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  *out = key->vk;
  if (ic_xy_out) memcpy(ic_xy_out, key->ic_xy.data(), key->ic_xy.size() * 8);
  if (ic_inf_out) memcpy(ic_inf_out, key->ic_inf.data(), key->ic_inf.size());
  return CP_OK;
} CP_CATCH(nullptr)

}  // extern "C"
