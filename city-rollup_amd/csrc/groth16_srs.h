// Kernels of the Groth16 setup from a powers-of-tau SRS (host side: groth16_srs.inc): the linear algebra
// that groth16_setup.inc does on logarithms, done on points. With [L_j]_* the Lagrange-basis points (the inverse point transform
// of the SRS powers, point_ntt.h):
//
//   k_columns_short                    for each wire i, sum over up to three products of sum_j M[j][i] * P_j, over the
//                                      transposed matrices: one lane per wire
//   k_columns_chunk / k_columns_combine  a wire of more kept terms than r1cs::LONG_ROW_THRESHOLD instead: workgroups whose lanes
//                                      take a term each and meet in an LDS tree, then one workgroup that adds their sums
//   k_z                                Z_j = [tau^(j+N)]_1 - [tau^j]_1
//   k_check_points                     the curve equation and, if asked, [r]P = infinity, for the points of an SRS
//   k_first_flag / k_differs           the lowest set flag of an array; whether two arrays differ
//   k_scale_each                       phase 1: every point of an SRS array times its own scalar c t^k
//   k_fill / k_canonical               the unit SRS; an SRS array as affine canonical words for the host
//
// A term's class (r1cs.h) chooses its action: +1 / -1 one mixed addition, a one-limb constant a short multiple, anything else
// the full multiple. All results are Jacobian points in a work array; pointntt::k_finish makes them affine with flags.
#pragma once
#include "point_ntt.h"
#include "r1cs.h"

namespace g16srs {

using bls::AffineT;
using bls::Field;
using bls::JacT;
using fixedbase::LANES;
using fixedbase::WAVES;
using pointntt::SCALAR_WORDS;

// *dst = *a + *q or *a - *q, q affine and not infinity; complete (a at infinity, a = q, a = -q); dst may be a
template <class F> PNTT_CALL void jac_add_mixed_at(JacT<F> *dst, const JacT<F> *a, const AffineT<F> *q, bool negate) {
  AffineT<F> t = *q;
  if (negate) t.y = bls::f_sub(Field<F>::zero(), t.y);
  *dst = bls::jac_add_mixed(*a, t);
}
// *r = k * *q for an affine q (not infinity), k in memory (8 words): pointntt::jac_mul_u256_at with the mixed addition
template <class F> GL_HD void affine_mul_u256_at(JacT<F> *r, const AffineT<F> *q, const uint32_t *k) {
  *r = bls::jac_inf<F>();
  for (int i = pointntt::top_bit(k); i >= 0; i--) {
    pointntt::jac_double_at<F>(r, r);
    if ((k[i >> 5] >> (i & 31)) & 1) jac_add_mixed_at<F>(r, r, q, false);
  }
}

// one product of a job: a transposed matrix (rows are wires, a term's col is a constraint) over one point vector
template <class F> struct Product {
  const uint64_t *row_ptr;
  const r1cs::Term *terms;  // zero coefficients dropped, sorted by class inside a row
  const AffineT<F> *pts;
  const uint8_t *inf;
};
template <class F> struct Job {
  Product<F> p[3];
  int n_products;
  const uint32_t *coeffs;  // canonical, 8 words each: the scalars of the general terms
  size_t n_wires;
};

// *acc += coefficient * P_col; prod and k are the lane's slots for a multiple and its scalar
template <class F>
GL_HD void apply_term(JacT<F> *acc, JacT<F> *prod, uint32_t *k, const Product<F> &P, const r1cs::Term t, const uint32_t *coeffs) {
  if (P.inf[t.col]) return;
  const AffineT<F> *q = P.pts + t.col;
  const uint32_t cls = t.tag & r1cs::TAG_MASK, payload = t.tag >> r1cs::TAG_BITS;
  if (cls == r1cs::CLS_ADD || cls == r1cs::CLS_SUB) {
    jac_add_mixed_at<F>(acc, acc, q, cls == r1cs::CLS_SUB);
    return;
  }
  for (int w = 0; w < SCALAR_WORDS; w++) k[w] = cls == r1cs::CLS_GENERAL ? coeffs[(size_t)SCALAR_WORDS * payload + w] : (w == 0 ? payload : 0u);
  affine_mul_u256_at<F>(prod, q, k);
  if (cls == r1cs::CLS_NEG_SMALL) prod->y = bls::f_sub(Field<F>::zero(), prod->y);
  pointntt::jac_add_at<F>(acc, acc, prod);
}
template <class F> GL_HD size_t kept_terms(const Job<F> &J, size_t i) {
  size_t total = 0;
  for (int p = 0; p < J.n_products; p++) total += J.p[p].row_ptr[i + 1] - J.p[p].row_ptr[i];
  return total;
}

// a lane per wire; the sum grows in the wire's own entry of the work array. Long wires are left to k_columns_chunk.
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_columns_short(Job<F> J, JacT<F> *work) {
  __shared__ JacT<F> prod[LANES<F>];
  __shared__ uint32_t ks[LANES<F>][SCALAR_WORDS];
  const size_t i = (size_t)blockIdx.x * LANES<F> + threadIdx.x;
  if (i >= J.n_wires) return;  // no barrier below
  if (kept_terms(J, i) > r1cs::LONG_ROW_THRESHOLD) return;
  JacT<F> *acc = work + i;
  *acc = bls::jac_inf<F>();
  for (int p = 0; p < J.n_products; p++) {
    const Product<F> &P = J.p[p];
    for (size_t t = P.row_ptr[i], end = P.row_ptr[i + 1]; t < end; t++) apply_term<F>(acc, &prod[threadIdx.x], ks[threadIdx.x], P, P.terms[t], J.coeffs);
  }
}
// Long wires: wire 0 in every row of A is a column of n terms, and a term is a scalar multiplication - ten thousand times a
// field product - so a long column is cut into chunks of CHUNK_TERMS terms that run side by side: a workgroup per chunk, a lane
// per term, an LDS tree of complete additions (k_columns_chunk); then a workgroup per wire adds the wire's chunk sums the same
// way (k_columns_combine). A chunk is (wire, index of its first term in the wire's kept terms, the products one after another).
constexpr unsigned CHUNK_TERMS = 64;
struct Chunk { uint32_t wire, first; };
template <class F>
__global__ __launch_bounds__(CHUNK_TERMS, WAVES<F>) void k_columns_chunk(Job<F> J, const Chunk *__restrict__ chunks, JacT<F> *partial) {
  __shared__ JacT<F> part[CHUNK_TERMS];
  __shared__ JacT<F> prod[CHUNK_TERMS];
  __shared__ uint32_t ks[CHUNK_TERMS][SCALAR_WORDS];
  const Chunk c = chunks[blockIdx.x];
  JacT<F> *acc = &part[threadIdx.x];
  *acc = bls::jac_inf<F>();
  size_t g = (size_t)c.first + threadIdx.x;  // this lane's term among the wire's kept terms
  for (int p = 0; p < J.n_products; p++) {
    const Product<F> &P = J.p[p];
    const size_t beg = P.row_ptr[c.wire], len = P.row_ptr[c.wire + 1] - beg;
    if (g < len) {
      apply_term<F>(acc, &prod[threadIdx.x], ks[threadIdx.x], P, P.terms[beg + g], J.coeffs);
      break;
    }
    g -= len;  // past the last product: the lane of a last chunk that has no term
  }
  __syncthreads();
  for (unsigned half = CHUNK_TERMS / 2; half > 0; half >>= 1) {  // idle lanes hold infinity
    if (threadIdx.x < half) pointntt::jac_add_at<F>(&part[threadIdx.x], &part[threadIdx.x], &part[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = part[0];
}
// chunk_ptr[w] .. chunk_ptr[w + 1]: the chunks of long wire w (long_wires: ascending)
template <class F>
__global__ __launch_bounds__(CHUNK_TERMS, WAVES<F>) void k_columns_combine(const uint32_t *__restrict__ long_wires, const uint32_t *__restrict__ chunk_ptr,
                                                                           const JacT<F> *partial, JacT<F> *work) {
  __shared__ JacT<F> part[CHUNK_TERMS];
  JacT<F> *acc = &part[threadIdx.x];
  *acc = bls::jac_inf<F>();
  for (uint32_t c = chunk_ptr[blockIdx.x] + threadIdx.x, end = chunk_ptr[blockIdx.x + 1]; c < end; c += CHUNK_TERMS) pointntt::jac_add_at<F>(acc, acc, partial + c);
  __syncthreads();
  for (unsigned half = CHUNK_TERMS / 2; half > 0; half >>= 1) {
    if (threadIdx.x < half) pointntt::jac_add_at<F>(&part[threadIdx.x], &part[threadIdx.x], &part[threadIdx.x + half]);
    __syncthreads();
  }
  if (threadIdx.x == 0) work[long_wires[blockIdx.x]] = part[0];
}

// work[j] = tau[j + N] - tau[j] for j < count (= N - 1)
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_z(const AffineT<F> *__restrict__ tau, size_t N, size_t count, JacT<F> *work) {
  const size_t j = (size_t)blockIdx.x * LANES<F> + threadIdx.x;
  if (j >= count) return;
  const AffineT<F> hi = tau[j + N];
  work[j] = {hi.x, hi.y, Field<F>::one()};
  jac_add_mixed_at<F>(work + j, work + j, tau + j, true);
}

// first_bad[0]: the lowest index of a point off the curve, first_bad[1]: of a point on it with [order]P != infinity (both
// initialised to ~0; the second is looked for only with check_torsion)
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_check_points(const AffineT<F> *__restrict__ pts, size_t n, int check_torsion, pointntt::Scalar order,
                                                                     unsigned long long *first_bad) {
  __shared__ JacT<F> prod[LANES<F>];
  __shared__ uint32_t ks[LANES<F>][SCALAR_WORDS];
  const size_t i = (size_t)blockIdx.x * LANES<F> + threadIdx.x;
  if (i >= n) return;
  const AffineT<F> q = pts[i];
  if (!bls::affine_on_curve(q)) {
    atomicMin(&first_bad[0], (unsigned long long)i);
    return;
  }
  if (!check_torsion) return;
  for (int w = 0; w < SCALAR_WORDS; w++) ks[threadIdx.x][w] = order.w[w];
  affine_mul_u256_at<F>(&prod[threadIdx.x], pts + i, ks[threadIdx.x]);
  if (!bls::jac_is_inf(prod[threadIdx.x])) atomicMin(&first_bad[1], (unsigned long long)i);
}

// ---- phase 1: the SRS itself (cp_groth16_srs_unit / _contribute / _points) ----
// The scalar of entry k of an array under a contribution (t, a, b): powers[k] = t^k, times the array's constant where it has
// one (a for alpha_tau_g1, b for beta_tau_g1; the two tau arrays have none). One table of t^k, k < 2n - 1, serves all four.
struct EachScalar {
  const blsfr::Fr *powers;  // Montgomery
  blsfr::Fr c;              // Montgomery; read only with has_c
  int has_c;
};
GL_HD void each_scalar(const EachScalar &S, size_t k, uint32_t *out) {
  blsfr::Fr s = S.powers[k];
  if (S.has_c) s = blsfr::fr_mul(s, S.c);
  blsfr::fr_to_canonical(s, out);
}
// what a lane of k_scale_each does: *prod = (c t^k) * pts[k], the scalar through the lane's eight words at ks
template <class F> GL_HD void scale_each_lane(JacT<F> *prod, uint32_t *ks, const AffineT<F> *pts, size_t k, const EachScalar &S) {
  each_scalar(S, k, ks);
  affine_mul_u256_at<F>(prod, pts + k, ks);
}
// work[k] = scalar(k) * pts[k]: a lane per point, each under its OWN scalar, so the conditional addition diverges inside a
// wave (255 doublings and up to 255 mixed additions per wave, where pointntt::k_scale pays the additions of one scalar). The
// source is the affine array itself: the mixed addition, and no load pass.
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_scale_each(const AffineT<F> *__restrict__ pts, size_t n, EachScalar S, JacT<F> *__restrict__ work) {
  __shared__ JacT<F> prod[LANES<F>];
  __shared__ uint32_t ks[LANES<F>][SCALAR_WORDS];
  const size_t k = (size_t)blockIdx.x * LANES<F> + threadIdx.x;
  if (k >= n) return;  // no barrier below: a lane reads only what it wrote
  scale_each_lane<F>(&prod[threadIdx.x], ks[threadIdx.x], pts, k, S);
  work[k] = prod[threadIdx.x];
}
// out[i] = p for every i < n: the unit SRS
template <class F>
__global__ __launch_bounds__(256) void k_fill(AffineT<F> p, size_t n, AffineT<F> *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = p;
}
// the internal form -> affine canonical words (x then y, Field<F>::WORDS each): what cp_groth16_srs_desc holds
template <class F>
__global__ __launch_bounds__(256) void k_canonical(const AffineT<F> *__restrict__ pts, size_t n, uint32_t *__restrict__ out) {
  constexpr int W = Field<F>::WORDS;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AffineT<F> a = pts[i];
  Field<F>::to_canonical(a.x, out + 2 * W * i);
  Field<F>::to_canonical(a.y, out + 2 * W * i + W);
}

__global__ void k_first_flag(const uint8_t *__restrict__ inf, size_t n, unsigned long long *first) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && inf[i]) atomicMin(first, (unsigned long long)i);
}
__global__ void k_differs(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, size_t n, uint32_t *differs) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && a[i] != b[i]) *differs = 1;
}

}  // namespace g16srs
