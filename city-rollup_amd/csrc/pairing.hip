// libcityprover_hip.so, third translation unit: BLS12-381 pairing products and the Groth16 verifier, batched on the device
// (DESIGN.md section 4.6). The arithmetic is pairing.h; here are the kernels - one lane per item, like k_bucket_sum and
// fixedbase::k_mul - and the entry points. The work is split into several kernels, none of which holds more than one of
// the big loops: point checks, the public-input sum, the Miller loop, and the product with the final exponentiation. In front of
// them, for proofs in their stored 192-byte form, the decompression (bls_sqrt.h): one launch for the F_p roots, one for the F_p^2 roots.
// Beside them, for a batch under one final exponentiation: the short multiples of A, the weighted sums of the public inputs, and the
// product tree over the Miller values; its two point sums go through the MSM's device entry point (bls.hip).
#include "core.h"
#include "pairing.h"
#include "bls_sqrt.h"
#include "bls12_381_fr.h"

namespace pairing {

constexpr unsigned LANES = 64;  // one wave per workgroup: its F_p^12 column block in LDS is 168 x 64 x 4 B = 42 KB, three per CU

// Affine canonical points from the API -> Montgomery form and a status each (pairing::point_status). Point i is read at
// xy + i * in_stride (u64 words) and written to slot i * out_stride + out_off of `out` and `status`. A flagged point (inf)
// is not looked at: status 0.
template <class F>
__global__ __launch_bounds__(LANES) void k_points(const uint64_t *__restrict__ xy, size_t in_stride, const uint8_t *__restrict__ inf, size_t n,
                                                  int check_torsion, bls::AffineT<F> *__restrict__ out, uint8_t *__restrict__ status, size_t out_stride,
                                                  size_t out_off) {
  const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (i >= n) return;
  const size_t o = i * out_stride + out_off;
  bls::AffineT<F> a = {bls::Field<F>::zero(), bls::Field<F>::zero()};
  int st = 0;
  if (!(inf && inf[i])) st = point_status<F>((const uint32_t *)(xy + i * in_stride), check_torsion != 0, a);
  out[o] = a;
  status[o] = (uint8_t)st;
}

// L = IC_0 + sum_{i >= 1} x_i IC_i per proof, affine, into slot 3 t + 1 of the pair arrays; -gamma and -delta into slots
// 3 t + 1 and 3 t + 2 of the G2 side. pub_status[t] = 1 where a public input is not below r (L is then not computed).
__global__ __launch_bounds__(LANES) void k_public_sum(const bls::Affine *__restrict__ ic, const uint8_t *__restrict__ ic_inf, size_t n_public,
                                                      const uint64_t *__restrict__ publics, size_t n, const bls::Affine2 *__restrict__ neg_gamma_delta,
                                                      bls::Affine *__restrict__ g1, uint8_t *__restrict__ g1_inf, bls::Affine2 *__restrict__ g2,
                                                      uint8_t *__restrict__ pub_status) {
  const size_t t = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (t >= n) return;
  g2[3 * t + 1] = neg_gamma_delta[0];
  g2[3 * t + 2] = neg_gamma_delta[1];
  bls::Jac acc = bls::jac_inf<Fp>();
  if (!ic_inf[0]) acc = {ic[0].x, ic[0].y, bls::fp_one()};
  bool bad = false;
#pragma unroll 1
  for (size_t i = 1; i < n_public; i++) {
    const uint32_t *x = (const uint32_t *)(publics + (t * (n_public - 1) + (i - 1)) * 4);
    if (!blsfr::fr_is_canonical(x)) { bad = true; break; }
    if (ic_inf[i]) continue;
    const bls::Affine p = ic[i];
    bls::Jac m = bls::jac_inf<Fp>();
#pragma unroll 1
    for (int b = 254; b >= 0; b--) {
      m = bls::jac_double(m);
      if ((x[b >> 5] >> (b & 31)) & 1) m = bls::jac_add_mixed(m, p);
    }
    acc = bls::jac_add(acc, m);
  }
  pub_status[t] = bad ? 1 : 0;
  const bool inf = bad || bls::jac_is_inf(acc);
  g1_inf[3 * t + 1] = inf ? 1 : 0;
  g1[3 * t + 1] = inf ? bls::Affine{bls::fp_zero(), bls::fp_zero()} : bls::jac_to_affine(acc);
}

// One Miller loop per lane. The running F_p^12 value is the lane's column of the LDS block [coefficient limb][lane]; the
// square of each step goes through the lane's column of `tmp` in HBM, and the result to its column of `out` ([168][n] both).
// A pair with a flag or a status set contributes one.
__global__ __launch_bounds__(LANES) void k_miller(const bls::Affine *__restrict__ g1, const bls::Affine2 *__restrict__ g2, const uint8_t *__restrict__ inf1,
                                                  const uint8_t *__restrict__ inf2, const uint8_t *__restrict__ st1, const uint8_t *__restrict__ st2, size_t n,
                                                  uint32_t *__restrict__ out, uint32_t *__restrict__ tmp) {
  __shared__ uint32_t f_lds[F12_WORDS][LANES];
  const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (i >= n) return;
  const F12 o = {out + i, n};
  if ((inf1 && inf1[i]) || (inf2 && inf2[i]) || st1[i] || st2[i]) {
    f12_set_one(o);
    return;
  }
  const F12 f = {&f_lds[0][threadIdx.x], LANES};
  miller_loop(f, F12{tmp + i, n}, g1[i], g2[i]);
  f12_copy(o, f);
}

// One product per lane: the k Miller values of product j (columns j k .. j k + k - 1 of `miller`) multiplied, the final
// exponentiation, the comparison with `target` (168 Montgomery limbs; NULL: with one). The value lives in the lane's LDS column,
// the four scratch values in its columns of `work` ([4][168][n]).
//   products (verify = 0): status[j] = the first non-zero point status of its pairs, is_one[j], gt[j] (72 canonical words)
//   verifier (verify = 1): status[j] = the verdict: the largest of 2 (a point status 1 or 2), 3, 4 (pub_status) that applies,
//                          else 0 / 1 by the comparison
__global__ __launch_bounds__(LANES) void k_final(const uint32_t *__restrict__ miller, size_t n_pairs, size_t n, size_t k, uint32_t *__restrict__ work,
                                                 const uint32_t *__restrict__ target, const uint8_t *__restrict__ st1, const uint8_t *__restrict__ st2,
                                                 const uint8_t *__restrict__ pub_status, int verify, uint64_t *__restrict__ gt, uint8_t *__restrict__ is_one,
                                                 uint8_t *__restrict__ status) {
  __shared__ uint32_t f_lds[F12_WORDS][LANES];
  const size_t j = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (j >= n) return;
  int st = 0;
  for (size_t i = 0; i < k; i++) {
    const int a = st1[j * k + i], b = st2[j * k + i];
    if (verify) {
      const int va = a == 1 ? 2 : a, vb = b == 1 ? 2 : b;
      st = va > st ? va : st;
      st = vb > st ? vb : st;
    } else if (!st) {
      st = a ? a : b;
    }
  }
  if (verify && pub_status[j]) st = 4;
  if (st) {
    status[j] = (uint8_t)st;
    if (is_one) is_one[j] = 0;
    if (gt)
      for (int w = 0; w < CP_GT_WORDS; w++) gt[j * CP_GT_WORDS + w] = 0;
    return;
  }
  const F12 f = {&f_lds[0][threadIdx.x], LANES};
  F12 t[4];
  for (int s = 0; s < 4; s++) t[s] = {work + (size_t)s * F12_WORDS * n + j, n};
  f12_copy(f, F12{const_cast<uint32_t *>(miller) + j * k, n_pairs});
#pragma unroll 1
  for (size_t i = 1; i < k; i++) {
    f12_mul(t[0], f, F12{const_cast<uint32_t *>(miller) + j * k + i, n_pairs});
    f12_copy(f, t[0]);
  }
  final_exp(f, t[0], t[1], t[2], t[3]);
  const bool same = target ? f12_eq(f, F12{const_cast<uint32_t *>(target), 1}) : f12_is_one(f);
  status[j] = verify ? (same ? 0 : 1) : 0;
  if (is_one) is_one[j] = same ? 1 : 0;
  if (gt)
#pragma unroll 1
    for (int c = 0; c < 6; c++) bls::Field<Fp2>::to_canonical(f12_get(f, c), (uint32_t *)(gt + j * CP_GT_WORDS + 12 * c));
}

// ---- the whole batch under one final exponentiation (cp_groth16_verify_all_bls12381) ----
// One lane per proof closes the point and input checks and scales A. st_a / st_b / st_c: the point statuses of A, B, C as
// k_points left them; st_a doubles as the Miller kernel's skip flag of pair t and is rewritten as such.
//   pre[t]  = the verdict the checks alone give: the largest of 2 (a point status 1 or 2), 3, 4 (a public input >= r), else 0
//   dead[t] = 1 where pre[t] != 0: the proof takes no part in the aggregated equation (the MSM's infinity flag of C_t)
//   wide[t] = the weight as a 256-bit MSM scalar (zero where dead)
//   a[t]    = rho_t A_t, affine, where the proof is live; st_a[t] = 1 where pair t is to contribute one (dead, or rho_t A_t is
//             infinity: an A of small order, which only CP_PAIRING_TRUSTED lets through)
__global__ __launch_bounds__(LANES) void k_scale_g1(bls::Affine *__restrict__ a, uint8_t *__restrict__ st_a, const uint8_t *__restrict__ st_b,
                                                    const uint8_t *__restrict__ st_c, size_t n_public, const uint64_t *__restrict__ publics,
                                                    const uint64_t *__restrict__ weights, size_t n, uint8_t *__restrict__ pre, uint8_t *__restrict__ dead,
                                                    uint64_t *__restrict__ wide) {
  const size_t t = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (t >= n) return;
  int v = 0;
  const int st[3] = {st_a[t], st_b[t], st_c[t]};
  for (int k = 0; k < 3; k++) {
    const int c = st[k] == 1 ? 2 : st[k];
    v = c > v ? c : v;
  }
  for (size_t i = 1; i < n_public; i++)
    if (!blsfr::fr_is_canonical((const uint32_t *)(publics + (t * (n_public - 1) + (i - 1)) * 4))) v = 4;
  const bool live = v == 0;
  pre[t] = (uint8_t)v;
  dead[t] = live ? 0 : 1;
  wide[4 * t] = live ? weights[2 * t] : 0;
  wide[4 * t + 1] = live ? weights[2 * t + 1] : 0;
  wide[4 * t + 2] = 0;
  wide[4 * t + 3] = 0;
  bool skip = !live;
  if (live) {
    const bls::Jac m = g1_mul_u128(a[t], (const uint32_t *)(weights + 2 * t));
    skip = bls::jac_is_inf(m);
    if (!skip) a[t] = bls::jac_to_affine(m);
  }
  st_a[t] = skip ? 1 : 0;
}

// s_0 = sum_t rho_t, s_j = sum_t rho_t x_tj (j >= 1) mod r over the live proofs: workgroup j strides over t, each lane keeps
// a running sum in Montgomery form, and the lanes' sums meet in a tree through LDS. s: n_public canonical 256-bit scalars,
// what the MSM over the IC points reads.
constexpr unsigned SUM_LANES = 256;
__global__ __launch_bounds__(SUM_LANES) void k_fr_weighted_sums(const uint64_t *__restrict__ wide, const uint8_t *__restrict__ dead,
                                                                const uint64_t *__restrict__ publics, size_t n_public, size_t n,
                                                                uint64_t *__restrict__ s) {
  __shared__ blsfr::Fr part[SUM_LANES];
  const size_t j = blockIdx.x;
  blsfr::Fr acc = blsfr::fr_zero();
#pragma unroll 1
  for (size_t t = threadIdx.x; t < n; t += SUM_LANES) {
    if (dead[t]) continue;
    blsfr::Fr term = blsfr::fr_from_canonical((const uint32_t *)(wide + 4 * t));
    if (j) term = blsfr::fr_mul(term, blsfr::fr_from_canonical((const uint32_t *)(publics + (t * (n_public - 1) + (j - 1)) * 4)));
    acc = blsfr::fr_add(acc, term);
  }
  part[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll 1
  for (unsigned h = SUM_LANES / 2; h; h >>= 1) {
    if (threadIdx.x < h) part[threadIdx.x] = blsfr::fr_add(part[threadIdx.x], part[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) blsfr::fr_to_canonical(part[0], (uint32_t *)(s + 4 * j));
}

// One round of the product tree over the m values in columns 0 .. m - 1 of `vals` ([168][stride]): lane i < m - half
// multiplies column i by column i + half (half = ceil(m / 2)) in its LDS column and writes the product back to column i, which
// no other lane reads in this round; with m odd, column half - 1 has no partner and stays. The host halves m until one is left.
__global__ __launch_bounds__(LANES) void k_gt_product(uint32_t *__restrict__ vals, size_t stride, size_t m, size_t half) {
  __shared__ uint32_t f_lds[F12_WORDS][LANES];
  const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (i >= m - half) return;
  const F12 f = {&f_lds[0][threadIdx.x], LANES};
  const F12 lo = {vals + i, stride};
  f12_mul(f, lo, F12{vals + i + half, stride});
  f12_copy(lo, f);
}

// ---- the stored proof form: n x 192 bytes, pi_a | pi_b_a0 | pi_b_a1 | pi_c, each a compressed point (bls_sqrt.h) ----
// One lane per element, the F_p elements and the F_p^2 element in launches of their own: a wave never mixes the one
// exponentiation of a G1 root with the two of a G2 root. Lane e of k_unpack_g1 takes pi_a (e even) or pi_c (e odd) of proof
// e / 2 and writes x | y into words 0 .. 11 or 36 .. 47 of the proof's 48 u64 of `out` (A | B | C, affine canonical, what
// verify_run stages) and its status class into est[e].
__global__ __launch_bounds__(LANES) void k_unpack_g1(const uint32_t *__restrict__ city, size_t n, uint64_t *__restrict__ out, uint8_t *__restrict__ est) {
  const size_t e = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (e >= 2 * n) return;
  const size_t t = e >> 1, c = e & 1;
  est[e] = (uint8_t)blssqrt::g1_decompress(city + t * 48 + 36 * c, (uint32_t *)(out + t * 48 + 36 * c));
}
// Lane t takes pi_b of proof t into words 12 .. 35, then closes the proof (the G1 launch is before it on the stream):
// status[t] = the smallest class that applies to any of the three elements, and a proof whose status is not 0 gets 48 zero words.
__global__ __launch_bounds__(LANES) void k_unpack_g2(const uint32_t *__restrict__ city, size_t n, uint64_t *__restrict__ out, const uint8_t *__restrict__ est,
                                                     uint8_t *__restrict__ status) {
  const size_t t = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (t >= n) return;
  int st = blssqrt::g2_decompress(city + t * 48 + 12, (uint32_t *)(out + t * 48 + 12));
  for (int c = 0; c < 2; c++) {
    const int s = est[2 * t + c];
    if (s && (!st || s < st)) st = s;
  }
  status[t] = (uint8_t)st;
  if (st)
    for (int w = 0; w < 48; w++) out[t * 48 + w] = 0;
}

}  // namespace pairing

struct cp_groth16_verifier {
  explicit cp_groth16_verifier(int dev) : device(dev), mem(dev_pool(), dev) {}
  const int device;
  size_t n_public = 0;
  bls::Affine *ic = nullptr;             // n_public points, Montgomery form (a flagged entry is not read)
  uint8_t *ic_inf = nullptr;
  bls::Affine2 *neg_gamma_delta = nullptr;  // -gamma, -delta, -beta (the tail pairs of the aggregated equation, in this order)
  uint32_t *target = nullptr;            // e(alpha, beta)^c: 168 Montgomery limbs
  bls::Affine alpha = {};                // on the host: the aggregated equation takes a multiple of it per call
  DevBag mem;
};

namespace {

void verifier_free(cp_groth16_verifier *v) {
  if (!v) return;
  if (v->mem.size()) (void)hipSetDevice(v->device);
  delete v;
}

// the temporaries of one call: ONE allocation, carved at 256-byte boundaries (a size pass, then a pointer pass)
struct Carve {
  char *base = nullptr;
  size_t off = 0;
  template <class T> T *take(size_t bytes) {
    T *p = base ? (T *)(base + off) : nullptr;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  }
};
constexpr size_t MAX_PAIRS = (size_t)1 << 24;

// the device arrays of n proofs in their stored form
struct City {
  uint8_t *bytes = nullptr;   // n x 192, as they came
  uint8_t *est = nullptr;     // 2 n: the status classes of pi_a and pi_c
  uint8_t *status = nullptr;  // n: of the proof
  void carve(Carve &c, size_t n) {
    bytes = c.take<uint8_t>(n * 192);
    est = c.take<uint8_t>(2 * n);
    status = c.take<uint8_t>(n);
  }
};

// the device arrays of a batch of pairs and products
struct Batch {
  size_t n_pairs = 0, n = 0, k = 0;
  uint64_t *g1_xy = nullptr, *g2_xy = nullptr, *publics = nullptr;  // staged input
  uint8_t *inf1 = nullptr, *inf2 = nullptr;
  bls::Affine *g1 = nullptr;
  bls::Affine2 *g2 = nullptr;
  uint8_t *st1 = nullptr, *st2 = nullptr, *pub_status = nullptr;
  uint32_t *miller = nullptr, *tmp = nullptr, *work = nullptr;
  uint64_t *gt = nullptr;
  uint8_t *is_one = nullptr, *status = nullptr;
  City city;  // the verifier's proofs in their stored form (city_proofs of them), else unused
  void carve(Carve &c, size_t g1_words, size_t g2_words, size_t pub_words, bool flags1, bool flags2, bool want_gt, size_t city_proofs = 0) {
    g1_xy = c.take<uint64_t>(g1_words * 8);
    g2_xy = c.take<uint64_t>(g2_words * 8);
    publics = pub_words ? c.take<uint64_t>(pub_words * 8) : nullptr;
    inf1 = flags1 ? c.take<uint8_t>(n_pairs) : nullptr;
    inf2 = flags2 ? c.take<uint8_t>(n_pairs) : nullptr;
    g1 = c.take<bls::Affine>(n_pairs * sizeof(bls::Affine));
    g2 = c.take<bls::Affine2>(n_pairs * sizeof(bls::Affine2));
    st1 = c.take<uint8_t>(n_pairs);
    st2 = c.take<uint8_t>(n_pairs);
    pub_status = c.take<uint8_t>(n);
    miller = c.take<uint32_t>(n_pairs * pairing::F12_WORDS * 4);
    tmp = c.take<uint32_t>(n_pairs * pairing::F12_WORDS * 4);
    work = c.take<uint32_t>(n * 4 * pairing::F12_WORDS * 4);
    gt = want_gt ? c.take<uint64_t>(n * CP_GT_WORDS * 8) : nullptr;
    is_one = c.take<uint8_t>(n);
    status = c.take<uint8_t>(n);
    if (city_proofs) city.carve(c, city_proofs);
  }
};

int batch_alloc(cp_ctx *ctx, DevBag &bag, Batch &b, size_t g1_words, size_t g2_words, size_t pub_words, bool flags1, bool flags2, bool want_gt,
                size_t city_proofs = 0) {
  Carve size;
  b.carve(size, g1_words, g2_words, pub_words, flags1, flags2, want_gt, city_proofs);
  Carve c;
  CP_TRY(alloc_status(ctx, bag.alloc(&c.base, size.off), size.off));
  b.carve(c, g1_words, g2_words, pub_words, flags1, flags2, want_gt, city_proofs);
  return CP_OK;
}

// n stored proofs on the device (c.bytes) -> n x 48 u64 at `out` and c.status
int city_unpack(cp_ctx *ctx, const City &c, size_t n, uint64_t *out) {
  using namespace pairing;
  LAUNCH(ctx, "groth16_unpack_g1", k_unpack_g1, dim3(blocks_for(2 * n, LANES)), dim3(LANES), (const uint32_t *)c.bytes, n, out, c.est);
  LAUNCH(ctx, "groth16_unpack_g2", k_unpack_g2, dim3(blocks_for(n, LANES)), dim3(LANES), (const uint32_t *)c.bytes, n, out, (const uint8_t *)c.est, c.status);
  return CP_OK;
}

int city_unpack_run(cp_ctx *ctx, const uint8_t *proofs, size_t n, uint64_t *proofs_out, uint8_t *status_out) {
  if (!proofs || !proofs_out || !status_out) return set_error(ctx, CP_ERR_INVALID_ARG, "unpack: NULL argument");
  if (n == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "unpack: n_proofs must be at least 1");
  if (n > MAX_PAIRS / 3) return set_error(ctx, CP_ERR_INVALID_ARG, "unpack: more than 2^24 / 3 proofs in one call");
  City city;
  Carve size;  // one allocation, as in batch_alloc: a size pass, then a pointer pass
  city.carve(size, n);
  size.take<uint64_t>(n * 48 * 8);
  DevBag bag = ctx->bag();
  Carve c;
  CP_TRY(alloc_status(ctx, bag.alloc(&c.base, size.off), size.off));
  city.carve(c, n);
  uint64_t *out = c.take<uint64_t>(n * 48 * 8);
  HIP_TRY(ctx, hipMemcpyAsync(city.bytes, proofs, n * 192, hipMemcpyHostToDevice, ctx->stream));
  CP_TRY(city_unpack(ctx, city, n, out));
  HIP_TRY(ctx, hipMemcpyAsync(proofs_out, out, n * 48 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(status_out, city.status, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, sync_stream(ctx));
  return CP_OK;
}

// Miller loops and products of a batch whose points and statuses are on the device
int batch_run(cp_ctx *ctx, const Batch &b, const uint32_t *target, int verify) {
  using namespace pairing;
  LAUNCH(ctx, "pairing_miller", k_miller, dim3(blocks_for(b.n_pairs, LANES)), dim3(LANES), (const bls::Affine *)b.g1, (const bls::Affine2 *)b.g2,
         (const uint8_t *)b.inf1, (const uint8_t *)b.inf2, (const uint8_t *)b.st1, (const uint8_t *)b.st2, b.n_pairs, b.miller, b.tmp);
  LAUNCH(ctx, "pairing_final", k_final, dim3(blocks_for(b.n, LANES)), dim3(LANES), (const uint32_t *)b.miller, b.n_pairs, b.n, b.k, b.work, target,
         (const uint8_t *)b.st1, (const uint8_t *)b.st2, (const uint8_t *)b.pub_status, verify, b.gt, b.is_one, b.status);
  return CP_OK;
}

int pairing_product_run(cp_ctx *ctx, const uint64_t *g1_xy, const uint8_t *g1_inf, const uint64_t *g2_xy, const uint8_t *g2_inf, size_t n, size_t k,
                        unsigned flags, uint64_t *gt_out, uint8_t *is_one_out, uint8_t *status_out) {
  using namespace pairing;
  if (!g1_xy || !g2_xy) return set_error(ctx, CP_ERR_INVALID_ARG, "pairing product: NULL point array");
  if (n == 0 || k == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "pairing product: n_products and k must be at least 1");
  if (!gt_out && !is_one_out) return set_error(ctx, CP_ERR_INVALID_ARG, "pairing product: both outputs are NULL");
  if (flags & ~CP_PAIRING_TRUSTED) return set_error(ctx, CP_ERR_INVALID_ARG, "pairing product: unknown flag bits 0x%x", flags);
  if (n > MAX_PAIRS || k > MAX_PAIRS || n * k > MAX_PAIRS) return set_error(ctx, CP_ERR_INVALID_ARG, "pairing product: more than 2^24 pairs in one call");
  Batch b;
  b.n = n; b.k = k; b.n_pairs = n * k;
  DevBag bag = ctx->bag();
  CP_TRY(batch_alloc(ctx, bag, b, b.n_pairs * 12, b.n_pairs * 24, 0, g1_inf != nullptr, g2_inf != nullptr, gt_out != nullptr));
  HIP_TRY(ctx, hipMemcpyAsync(b.g1_xy, g1_xy, b.n_pairs * 96, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(b.g2_xy, g2_xy, b.n_pairs * 192, hipMemcpyHostToDevice, ctx->stream));
  if (g1_inf) HIP_TRY(ctx, hipMemcpyAsync(b.inf1, g1_inf, b.n_pairs, hipMemcpyHostToDevice, ctx->stream));
  if (g2_inf) HIP_TRY(ctx, hipMemcpyAsync(b.inf2, g2_inf, b.n_pairs, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(b.pub_status, 0, n, ctx->stream));
  const int torsion = (flags & CP_PAIRING_TRUSTED) ? 0 : 1;
  LAUNCH(ctx, "pairing_points_g1", k_points<Fp>, dim3(blocks_for(b.n_pairs, LANES)), dim3(LANES), (const uint64_t *)b.g1_xy, (size_t)12,
         (const uint8_t *)b.inf1, b.n_pairs, torsion, b.g1, b.st1, (size_t)1, (size_t)0);
  LAUNCH(ctx, "pairing_points_g2", k_points<Fp2>, dim3(blocks_for(b.n_pairs, LANES)), dim3(LANES), (const uint64_t *)b.g2_xy, (size_t)24,
         (const uint8_t *)b.inf2, b.n_pairs, torsion, b.g2, b.st2, (size_t)1, (size_t)0);
  CP_TRY(batch_run(ctx, b, nullptr, 0));
  if (gt_out) HIP_TRY(ctx, hipMemcpyAsync(gt_out, b.gt, n * CP_GT_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (is_one_out) HIP_TRY(ctx, hipMemcpyAsync(is_one_out, b.is_one, n, hipMemcpyDeviceToHost, ctx->stream));
  if (status_out) HIP_TRY(ctx, hipMemcpyAsync(status_out, b.status, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, sync_stream(ctx));
  return CP_OK;
}

// a key point on the host: the curve and the r-torsion, always
template <class F>
int key_point(cp_ctx *ctx, const uint64_t *xy, const char *name, size_t index, bls::AffineT<F> *out) {
  const int st = pairing::point_status<F>((const uint32_t *)xy, true, *out);
  if (st == 0) return CP_OK;
  char who[64];
  if (index == (size_t)-1) snprintf(who, sizeof who, "%s", name);
  else snprintf(who, sizeof who, "%s[%zu]", name, index);
  return set_error(ctx, CP_ERR_INVALID_ARG, "verifying key: %s %s", who,
                   st == 1 ? "has a coordinate that is not canonical (>= p)" : st == 2 ? "is not on the curve" : "is not in the r-torsion subgroup");
}

int verifier_build(cp_ctx *ctx, const cp_groth16_vk *vk, const uint64_t *ic_xy, const uint8_t *ic_inf, cp_groth16_verifier *v) {
  const size_t np = vk->n_public;
  if (np == 0 || np > ((size_t)1 << 20)) return set_error(ctx, CP_ERR_INVALID_ARG, "verifying key: n_public %zu out of range (1 .. 2^20; it counts wire 0)", np);
  bls::Affine alpha;
  bls::Affine2 gd[3];  // gamma, delta, beta
  CP_TRY(key_point<bls::Fp>(ctx, vk->alpha_g1, "alpha_g1", (size_t)-1, &alpha));
  CP_TRY(key_point<bls::Fp2>(ctx, vk->beta_g2, "beta_g2", (size_t)-1, &gd[2]));
  CP_TRY(key_point<bls::Fp2>(ctx, vk->gamma_g2, "gamma_g2", (size_t)-1, &gd[0]));
  CP_TRY(key_point<bls::Fp2>(ctx, vk->delta_g2, "delta_g2", (size_t)-1, &gd[1]));
  for (auto &q : gd) q.y = pairing::fp2_neg(q.y);
  std::vector<bls::Affine> ic(np);
  std::vector<uint8_t> inf(np, 0);
  for (size_t i = 0; i < np; i++) {
    inf[i] = ic_inf && ic_inf[i] ? 1 : 0;
    if (inf[i]) ic[i] = {bls::fp_zero(), bls::fp_zero()};
    else CP_TRY(key_point<bls::Fp>(ctx, ic_xy + 12 * i, "ic", i, &ic[i]));
  }
  // e(alpha, beta)^c through the batch path, then back to Montgomery limbs
  uint64_t gt[CP_GT_WORDS];
  CP_TRY(pairing_product_run(ctx, vk->alpha_g1, nullptr, vk->beta_g2, nullptr, 1, 1, CP_PAIRING_TRUSTED, gt, nullptr, nullptr));
  uint32_t target[pairing::F12_WORDS];
  for (int c = 0; c < 12; c++) {
    const bls::Fp e = bls::fp_from_canonical((const uint32_t *)(gt + 6 * c));
    memcpy(target + c * bls::NL, e.l, sizeof e.l);
  }
  CP_TRY(alloc_status(ctx, v->mem.alloc(&v->ic, np * sizeof(bls::Affine)), np * sizeof(bls::Affine)));
  CP_TRY(alloc_status(ctx, v->mem.alloc(&v->ic_inf, np), np));
  CP_TRY(alloc_status(ctx, v->mem.alloc(&v->neg_gamma_delta, sizeof gd), sizeof gd));
  CP_TRY(alloc_status(ctx, v->mem.alloc(&v->target, sizeof target), sizeof target));
  HIP_TRY(ctx, hipMemcpyAsync(v->ic, ic.data(), np * sizeof(bls::Affine), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(v->ic_inf, inf.data(), np, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(v->neg_gamma_delta, gd, sizeof gd, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(v->target, target, sizeof target, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, sync_stream(ctx));  // the host arrays die with this call
  v->n_public = np;
  v->alpha = alpha;
  return CP_OK;
}

// proofs: n x 48 u64 of coordinates (city = false) or n x 192 bytes in the stored form (city = true), which are decompressed on
// the device into the same staging array: a proof refused there is 48 zero words, on neither the curve nor the twist, and
// gets verdict 2 from the point checks like any other bad point.
// the refusals that both forms of the verifier share
int verify_args(cp_ctx *ctx, const cp_groth16_verifier *v, const void *proofs, const uint64_t *publics, size_t n, unsigned flags, const uint8_t *verdict_out) {
  if (!v) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: the verifier is NULL");
  if (v->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: the verifier lives on device %d, the context on device %d", v->device, ctx->device);
  if (!proofs || !verdict_out) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: NULL argument");
  if (n == 0) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: n_proofs must be at least 1");
  if (v->n_public > 1 && !publics) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: the key has %zu public inputs and public_inputs_host is NULL", v->n_public - 1);
  if (flags & ~CP_PAIRING_TRUSTED) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: unknown flag bits 0x%x", flags);
  if (n > MAX_PAIRS / 3) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: more than 2^24 / 3 proofs in one call");
  if ((v->n_public - 1) > (((size_t)1 << 40) / n)) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: n_proofs x public inputs is too large");
  return CP_OK;
}

int verify_run(cp_ctx *ctx, const cp_groth16_verifier *v, const void *proofs, bool city, const uint64_t *publics, size_t n, unsigned flags, uint8_t *verdict_out) {
  using namespace pairing;
  CP_TRY(verify_args(ctx, v, proofs, publics, n, flags, verdict_out));
  Batch b;
  b.n = n; b.k = 3; b.n_pairs = 3 * n;
  const size_t pub_words = n * (v->n_public - 1) * 4;
  DevBag bag = ctx->bag();
  CP_TRY(batch_alloc(ctx, bag, b, n * 48, 0, pub_words, true, false, false, city ? n : 0));
  uint64_t *pr = b.g1_xy;  // the proofs as coordinates: A | B | C
  if (city) {
    HIP_TRY(ctx, hipMemcpyAsync(b.city.bytes, proofs, n * 192, hipMemcpyHostToDevice, ctx->stream));
    CP_TRY(city_unpack(ctx, b.city, n, pr));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(pr, proofs, n * 48 * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (pub_words) HIP_TRY(ctx, hipMemcpyAsync(b.publics, publics, pub_words * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(b.inf1, 0, b.n_pairs, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(b.st1, 0, b.n_pairs, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(b.st2, 0, b.n_pairs, ctx->stream));
  const int torsion = (flags & CP_PAIRING_TRUSTED) ? 0 : 1;
  const dim3 grid(blocks_for(n, LANES)), block(LANES);
  LAUNCH(ctx, "pairing_points_g1", k_points<Fp>, grid, block, (const uint64_t *)pr, (size_t)48, (const uint8_t *)nullptr, n, torsion, b.g1, b.st1, (size_t)3, (size_t)0);
  LAUNCH(ctx, "pairing_points_g1", k_points<Fp>, grid, block, (const uint64_t *)(pr + 36), (size_t)48, (const uint8_t *)nullptr, n, torsion, b.g1, b.st1, (size_t)3, (size_t)2);
  LAUNCH(ctx, "pairing_points_g2", k_points<Fp2>, grid, block, (const uint64_t *)(pr + 12), (size_t)48, (const uint8_t *)nullptr, n, torsion, b.g2, b.st2, (size_t)3, (size_t)0);
  LAUNCH(ctx, "pairing_public_sum", k_public_sum, grid, block, (const bls::Affine *)v->ic, (const uint8_t *)v->ic_inf, v->n_public, (const uint64_t *)b.publics, n,
         (const bls::Affine2 *)v->neg_gamma_delta, b.g1, b.inf1, b.g2, b.pub_status);
  CP_TRY(batch_run(ctx, b, v->target, 1));
  HIP_TRY(ctx, hipMemcpyAsync(verdict_out, b.status, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, sync_stream(ctx));
  return CP_OK;
}

// the device arrays of one aggregated check: n pairs (rho_t A_t, B_t) and the three tail pairs behind them
struct AllBatch {
  size_t n = 0, n_pairs = 0;
  uint64_t *proofs = nullptr, *publics = nullptr, *weights = nullptr, *wide = nullptr, *s = nullptr;
  bls::Affine *g1 = nullptr, *c = nullptr;  // g1: n + 3 (A, then the tails); c: n, dense, what the MSM reads
  bls::Affine2 *g2 = nullptr;
  uint8_t *st1 = nullptr, *st2 = nullptr, *st_c = nullptr, *pre = nullptr, *dead = nullptr, *zero = nullptr, *status = nullptr;
  uint32_t *miller = nullptr, *tmp = nullptr, *work = nullptr;
  City city;
  void carve(Carve &k, size_t pub_words, size_t n_public, bool stored) {
    proofs = k.take<uint64_t>(n * 48 * 8);
    publics = pub_words ? k.take<uint64_t>(pub_words * 8) : nullptr;
    weights = k.take<uint64_t>(n * 16);
    wide = k.take<uint64_t>(n * 32);
    s = k.take<uint64_t>(n_public * 32);
    g1 = k.take<bls::Affine>(n_pairs * sizeof(bls::Affine));
    c = k.take<bls::Affine>(n * sizeof(bls::Affine));
    g2 = k.take<bls::Affine2>(n_pairs * sizeof(bls::Affine2));
    st1 = k.take<uint8_t>(n_pairs);
    st2 = k.take<uint8_t>(n_pairs);
    st_c = k.take<uint8_t>(n);
    pre = k.take<uint8_t>(n);
    dead = k.take<uint8_t>(n);
    zero = k.take<uint8_t>(1);
    status = k.take<uint8_t>(1);
    miller = k.take<uint32_t>(n_pairs * pairing::F12_WORDS * 4);
    tmp = k.take<uint32_t>(n_pairs * pairing::F12_WORDS * 4);
    work = k.take<uint32_t>(4 * pairing::F12_WORDS * 4);
    if (stored) city.carve(k, n);
  }
};

// The aggregated equation over the proofs that pass the point and input checks (pre[t] = 0):
//   prod_t e(rho_t A_t, B_t) . e(sum_j s_j IC_j, -gamma) . e(sum_t rho_t C_t, -delta) . e(s_0 alpha, -beta) = 1.
// *holds: whether it does (true as well when no proof is live: nothing is left to check). pre: n bytes on the host.
int aggregate_run(cp_ctx *ctx, const cp_groth16_verifier *v, const void *proofs, bool city, const uint64_t *publics, const uint64_t *weights, size_t n,
                  unsigned flags, uint8_t *pre, bool *holds) {
  using namespace pairing;
  AllBatch b;
  b.n = n; b.n_pairs = n + 3;
  const size_t np = v->n_public, pub_words = n * (np - 1) * 4;
  DevBag bag = ctx->bag();
  Carve size;
  b.carve(size, pub_words, np, city);
  Carve k;
  CP_TRY(alloc_status(ctx, bag.alloc(&k.base, size.off), size.off));
  b.carve(k, pub_words, np, city);
  if (city) {
    HIP_TRY(ctx, hipMemcpyAsync(b.city.bytes, proofs, n * 192, hipMemcpyHostToDevice, ctx->stream));
    CP_TRY(city_unpack(ctx, b.city, n, b.proofs));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(b.proofs, proofs, n * 48 * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (pub_words) HIP_TRY(ctx, hipMemcpyAsync(b.publics, publics, pub_words * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(b.weights, weights, n * 16, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(b.st1, 0, b.n_pairs, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(b.st2, 0, b.n_pairs, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(b.zero, 0, 1, ctx->stream));
  const int torsion = (flags & CP_PAIRING_TRUSTED) ? 0 : 1;
  const dim3 grid(blocks_for(n, LANES)), block(LANES);
  LAUNCH(ctx, "pairing_points_g1", k_points<Fp>, grid, block, (const uint64_t *)b.proofs, (size_t)48, (const uint8_t *)nullptr, n, torsion, b.g1, b.st1, (size_t)1, (size_t)0);
  LAUNCH(ctx, "pairing_points_g1", k_points<Fp>, grid, block, (const uint64_t *)(b.proofs + 36), (size_t)48, (const uint8_t *)nullptr, n, torsion, b.c, b.st_c, (size_t)1, (size_t)0);
  LAUNCH(ctx, "pairing_points_g2", k_points<Fp2>, grid, block, (const uint64_t *)(b.proofs + 12), (size_t)48, (const uint8_t *)nullptr, n, torsion, b.g2, b.st2, (size_t)1, (size_t)0);
  LAUNCH(ctx, "groth16_scale_g1", k_scale_g1, grid, block, b.g1, b.st1, (const uint8_t *)b.st2, (const uint8_t *)b.st_c, np, (const uint64_t *)b.publics,
         (const uint64_t *)b.weights, n, b.pre, b.dead, b.wide);
  LAUNCH(ctx, "groth16_weighted_sums", k_fr_weighted_sums, dim3((unsigned)np), dim3(SUM_LANES), (const uint64_t *)b.wide, (const uint8_t *)b.dead,
         (const uint64_t *)b.publics, np, n, b.s);
  uint64_t s0[4];
  HIP_TRY(ctx, hipMemcpyAsync(pre, b.pre, n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(s0, b.s, sizeof s0, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, sync_stream(ctx));
  size_t live = 0;
  for (size_t t = 0; t < n; t++) live += pre[t] == 0;
  *holds = true;
  if (!live) return CP_OK;
  // the three tail points: two sums through the MSM on the device (k_points left C in the form the MSM reads, the IC points
  // are held in it), the multiple of alpha on the host; tail[i] pairs with entry i of the verifier's -gamma, -delta, -beta
  uint64_t sum_xy[2][12];
  int sum_inf[2];
  CP_TRY(cp_msm_bls12381_g1_dev(ctx, b.s, v->ic, v->ic_inf, np, sum_xy[0], &sum_inf[0]));
  CP_TRY(cp_msm_bls12381_g1_dev(ctx, b.wide, b.c, b.dead, n, sum_xy[1], &sum_inf[1]));
  bls::Affine tail[3];
  uint8_t tail_inf[3];
  for (int i = 0; i < 2; i++) {
    tail_inf[i] = sum_inf[i] ? 1 : 0;
    tail[i] = bls::affine_from_canonical<Fp>((const uint32_t *)sum_xy[i]);
  }
  bls::Jac sa = bls::jac_inf<Fp>();
  for (int i = 254; i >= 0; i--) {
    sa = bls::jac_double(sa);
    if ((s0[i >> 6] >> (i & 63)) & 1) sa = bls::jac_add_mixed(sa, v->alpha);
  }
  tail_inf[2] = bls::jac_is_inf(sa) ? 1 : 0;
  tail[2] = tail_inf[2] ? bls::Affine{bls::fp_zero(), bls::fp_zero()} : bls::jac_to_affine(sa);
  HIP_TRY(ctx, hipMemcpyAsync(b.g1 + n, tail, sizeof tail, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(b.st1 + n, tail_inf, sizeof tail_inf, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(b.g2 + n, v->neg_gamma_delta, 3 * sizeof(bls::Affine2), hipMemcpyDeviceToDevice, ctx->stream));
  LAUNCH(ctx, "pairing_miller", k_miller, dim3(blocks_for(b.n_pairs, LANES)), block, (const bls::Affine *)b.g1, (const bls::Affine2 *)b.g2, (const uint8_t *)nullptr,
         (const uint8_t *)nullptr, (const uint8_t *)b.st1, (const uint8_t *)b.st2, b.n_pairs, b.miller, b.tmp);
  for (size_t m = b.n_pairs; m > 1;) {
    const size_t half = (m + 1) / 2;
    LAUNCH(ctx, "groth16_gt_product", k_gt_product, dim3(blocks_for(m - half, LANES)), block, b.miller, b.n_pairs, m, half);
    m = half;
  }
  // one lane: the final exponentiation of column 0 and the comparison with one
  LAUNCH(ctx, "pairing_final", k_final, dim3(1), block, (const uint32_t *)b.miller, b.n_pairs, (size_t)1, (size_t)1, b.work, (const uint32_t *)nullptr,
         (const uint8_t *)b.zero, (const uint8_t *)b.zero, (const uint8_t *)b.zero, 1, (uint64_t *)nullptr, (uint8_t *)nullptr, b.status);
  uint8_t status = 1;
  HIP_TRY(ctx, hipMemcpyAsync(&status, b.status, 1, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, sync_stream(ctx));
  *holds = status == 0;
  return CP_OK;
}

int verify_all_run(cp_ctx *ctx, const cp_groth16_verifier *v, const void *proofs, bool city, const uint64_t *publics, size_t n, const uint64_t *weights,
                   unsigned flags, uint8_t *verdict_out, int *path_out) {
  CP_TRY(verify_args(ctx, v, proofs, publics, n, flags, verdict_out));
  if (!weights) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: weights_host is NULL");
  for (size_t t = 0; t < n; t++)
    if (!(weights[2 * t] | weights[2 * t + 1])) return set_error(ctx, CP_ERR_INVALID_ARG, "verify: weight %zu is zero", t);
  std::vector<uint8_t> pre(n);
  bool holds = false;
  CP_TRY(aggregate_run(ctx, v, proofs, city, publics, weights, n, flags, pre.data(), &holds));  // its device memory is released here
  if (holds) {
    memcpy(verdict_out, pre.data(), n);
  } else {
    // some live proof is bad: the per-proof check over the whole batch says which (and repeats the verdicts of the checks)
    CP_TRY(verify_run(ctx, v, proofs, city, publics, n, flags, verdict_out));
  }
  if (path_out) *path_out = holds ? 0 : 1;
  return CP_OK;
}

}  // namespace

extern "C" {

int cp_pairing_product_bls12381(cp_ctx *ctx, const uint64_t *g1_xy_host, const uint8_t *g1_inf_host, const uint64_t *g2_xy_host, const uint8_t *g2_inf_host,
                                size_t n_products, size_t k, unsigned flags, uint64_t *gt_out_host, uint8_t *is_one_out_host, uint8_t *status_out_host) try {
  CHECK_CTX(ctx);
  return pairing_product_run(ctx, g1_xy_host, g1_inf_host, g2_xy_host, g2_inf_host, n_products, k, flags, gt_out_host, is_one_out_host, status_out_host);
} CP_CATCH(ctx)

cp_groth16_verifier *cp_groth16_verifier_create_bls12381(cp_ctx *ctx, const cp_groth16_vk *vk, const uint64_t *ic_xy, const uint8_t *ic_inf) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  if (!vk || !ic_xy) { set_error(ctx, CP_ERR_INVALID_ARG, "verifier: NULL argument"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  cp_groth16_verifier *v = new cp_groth16_verifier(ctx->device);
  struct Guard { cp_groth16_verifier *v; ~Guard() { verifier_free(v); } } guard{v};
  if (verifier_build(ctx, vk, ic_xy, ic_inf, v) != CP_OK) return nullptr;
  guard.v = nullptr;
  return v;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

void cp_groth16_verifier_destroy(cp_groth16_verifier *v) try {
  verifier_free(v);
} catch (...) {
}

int cp_groth16_verify_bls12381(cp_ctx *ctx, const cp_groth16_verifier *v, const uint64_t *proofs_host, const uint64_t *public_inputs_host, size_t n_proofs,
                               unsigned flags, uint8_t *verdict_out_host) try {
  CHECK_CTX(ctx);
  return verify_run(ctx, v, proofs_host, false, public_inputs_host, n_proofs, flags, verdict_out_host);
} CP_CATCH(ctx)

int cp_groth16_verify_city_bls12381(cp_ctx *ctx, const cp_groth16_verifier *v, const uint8_t *proofs_host, const uint64_t *public_inputs_host, size_t n_proofs,
                                    unsigned flags, uint8_t *verdict_out_host) try {
  CHECK_CTX(ctx);
  return verify_run(ctx, v, proofs_host, true, public_inputs_host, n_proofs, flags, verdict_out_host);
} CP_CATCH(ctx)

int cp_groth16_verify_all_bls12381(cp_ctx *ctx, const cp_groth16_verifier *v, const uint64_t *proofs_host, const uint64_t *public_inputs_host, size_t n_proofs,
                                   const uint64_t *weights_host, unsigned flags, uint8_t *verdict_out_host, int *path_out) try {
  CHECK_CTX(ctx);
  return verify_all_run(ctx, v, proofs_host, false, public_inputs_host, n_proofs, weights_host, flags, verdict_out_host, path_out);
} CP_CATCH(ctx)

int cp_groth16_verify_all_city_bls12381(cp_ctx *ctx, const cp_groth16_verifier *v, const uint8_t *proofs_host, const uint64_t *public_inputs_host, size_t n_proofs,
                                        const uint64_t *weights_host, unsigned flags, uint8_t *verdict_out_host, int *path_out) try {
  CHECK_CTX(ctx);
  return verify_all_run(ctx, v, proofs_host, true, public_inputs_host, n_proofs, weights_host, flags, verdict_out_host, path_out);
} CP_CATCH(ctx)

int cp_groth16_proofs_unpack_city_bls12381(cp_ctx *ctx, const uint8_t *proofs_host, size_t n_proofs, uint64_t *proofs_out_host, uint8_t *status_out_host) try {
  CHECK_CTX(ctx);
  return city_unpack_run(ctx, proofs_host, n_proofs, proofs_out_host, status_out_host);
} CP_CATCH(ctx)

}  // extern "C"
