// Transforms and scalar multiples of POINT vectors over BLS12-381 G1 and G2 (a Groth16 key from a
// powers-of-tau SRS needs the Lagrange-basis points [L_j(tau)], the inverse transform of [tau^k] in the exponent). Templates
// over the coordinate field like msm.h and fixed_base.h:
//
//   jac_mul_u256_at   k * P for a 256-bit k, double-and-add from the top set bit with the COMPLETE addition; any integer k
//                     (k >= r included), P or the result at infinity. Host and device (tests/pointsim/pointsim.hip).
//   k_load            affine points + infinity flags -> Jacobian work array (optionally in bit-reversed order)
//   k_stage           one radix-2 decimation-in-time stage: (P, Q) -> (P + w Q, P - w Q), w = omega_n^twiddle_index; the
//                     multiplication is skipped where w = 1
//   k_scale           every point of the work array times one scalar shared by the launch
//   k_finish          Jacobian work array -> affine points + flags, K points of a lane through ONE inversion (Montgomery's
//                     trick, as fixedbase::k_mul)
//
// Every point operation is a call on operands in memory (a lane's LDS slot and the work array), not inlined: an addition
// that carries its doubling for the equal-points case, a doubling and two or three points held across them do not fit the
// registers of a lane over F_p^2 (msm.h, k_segment_reduce), and a point operation is several thousand instructions against
// the hundred that move its operands. So neither instance spills, and the scalar's bits steer calls, not inlined bodies.
#pragma once
#include "bls12_381_fr.h"
#include "fixed_base.h"

namespace pointntt {

using bls::AffineT;
using bls::Field;
using bls::JacT;
using fixedbase::LANES;
using fixedbase::WAVES;

constexpr int K = 4;           // results of a lane that share one inversion
constexpr int SCALAR_WORDS = 8;  // 256-bit scalars, little-endian 32-bit words
struct Scalar { uint32_t w[SCALAR_WORDS]; };

#define PNTT_CALL __host__ __device__ __noinline__

// dst may be one of the operands: the result is complete before it is stored
template <class F> PNTT_CALL void jac_double_at(JacT<F> *dst, const JacT<F> *a) { *dst = bls::jac_double(*a); }
template <class F> PNTT_CALL bool jac_add_distinct_at(JacT<F> *dst, const JacT<F> *a, const JacT<F> *b) {
  JacT<F> r;
  if (!bls::jac_add_distinct(*a, *b, r)) return false;
  *dst = r;
  return true;
}
// the complete addition: either operand at infinity, a = -b (infinity) and a = b (the doubling, its own call)
template <class F> GL_HD void jac_add_at(JacT<F> *dst, const JacT<F> *a, const JacT<F> *b) {
  if (!jac_add_distinct_at<F>(dst, a, b)) jac_double_at<F>(dst, a);
}

// index of the top set bit of k, -1 for k = 0
GL_HD int top_bit(const uint32_t *k) {
  for (int w = SCALAR_WORDS - 1; w >= 0; w--) {
    const uint32_t v = k[w];
    if (!v) continue;
    int b = 31;
    while (!(v >> b)) b--;
    return 32 * w + b;
  }
  return -1;
}
// *r = k * *p; r and p distinct objects, k in memory (8 words). The integer multiple: no reduction of k mod r is assumed.
template <class F> GL_HD void jac_mul_u256_at(JacT<F> *r, const JacT<F> *p, const uint32_t *k) {
  *r = bls::jac_inf<F>();
  for (int i = top_bit(k); i >= 0; i--) {
    jac_double_at<F>(r, r);
    if ((k[i >> 5] >> (i & 31)) & 1) jac_add_at<F>(r, r, p);
  }
}

// Butterfly t (< n / 2) of stage s (< log_n) of the decimation-in-time transform on bit-reversed input: the pair
// (lo, lo + 2^s) and the power of omega_n its second entry is multiplied by, omega_(2^(s+1))^j = omega_n^(j 2^(log_n-1-s))
struct Butterfly { size_t lo, hi, twiddle; };
GL_HD Butterfly butterfly(size_t t, int s, int log_n) {
  const size_t half = (size_t)1 << s, j = t & (half - 1), lo = ((t - j) << 1) + j;
  return {lo, lo + half, j << (log_n - 1 - s)};
}
GL_HD size_t bit_reverse(size_t i, int log_n) {
  size_t r = 0;
  for (int b = 0; b < log_n; b++) r |= ((i >> b) & 1) << (log_n - 1 - b);
  return r;
}

// work[rev(i)] (BITREV) or work[i] = points[i], infinity where flagged (inf = NULL: no point is)
template <class F, bool BITREV>
__global__ __launch_bounds__(256) void k_load(const AffineT<F> *__restrict__ pts, const uint8_t *__restrict__ inf, size_t n, int log_n,
                                              JacT<F> *__restrict__ work) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const AffineT<F> a = pts[i];
  work[BITREV ? bit_reverse(i, log_n) : i] = inf && inf[i] ? bls::jac_inf<F>() : JacT<F>{a.x, a.y, Field<F>::one()};
}

// one lane per butterfly; tw[e] = omega^e (Montgomery), e < n / 2
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_stage(JacT<F> *work, size_t n_half, int s, int log_n,
                                                              const blsfr::Fr *__restrict__ tw) {
  __shared__ JacT<F> prod[LANES<F>];
  __shared__ uint32_t ks[LANES<F>][SCALAR_WORDS];
  const size_t t = (size_t)blockIdx.x * LANES<F> + threadIdx.x;
  if (t >= n_half) return;  // no barrier below: a lane reads only what it wrote
  const Butterfly bf = butterfly(t, s, log_n);
  JacT<F> *P = work + bf.lo, *Q = work + bf.hi, *wq = &prod[threadIdx.x];
  if (bf.twiddle == 0) {
    *wq = *Q;
  } else {
    uint32_t *k = ks[threadIdx.x];
    blsfr::fr_to_canonical(tw[bf.twiddle], k);
    jac_mul_u256_at<F>(wq, Q, k);
  }
  *Q = bls::jac_neg(*wq);
  jac_add_at<F>(Q, P, Q);   // P - w Q
  jac_add_at<F>(P, P, wq);  // P + w Q
}

// work[i] = scale * work[i] for one scalar shared by the launch (the 1/n of an inverse transform, a contribution to a key): a
// lane per point, so that the bits of the scalar steer every lane of a wave the same way
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_scale(JacT<F> *work, size_t n, Scalar scale) {
  __shared__ JacT<F> prod[LANES<F>];
  __shared__ uint32_t ks[LANES<F>][SCALAR_WORDS];
  const size_t i = (size_t)blockIdx.x * LANES<F> + threadIdx.x;
  if (i >= n) return;  // no barrier below: a lane reads only what it wrote
  for (int w = 0; w < SCALAR_WORDS; w++) ks[threadIdx.x][w] = scale.w[w];
  jac_mul_u256_at<F>(&prod[threadIdx.x], work + i, ks[threadIdx.x]);
  work[i] = prod[threadIdx.x];
}

// out[i] = work[i], affine, Montgomery coordinates fully reduced; inf[i] = 1 where that is the point at infinity, and the entry
// then holds `gen`. Lane t owns the points t K .. t K + K - 1: it keeps X and Y in the output entry and Z in its LDS column,
// inverts the product of its Z once and writes x = X / Z^2, y = Y / Z^3.
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_finish(const JacT<F> *__restrict__ work, size_t n, AffineT<F> gen, AffineT<F> *__restrict__ out,
                                                               uint8_t *__restrict__ inf) {
  __shared__ F zs[K][LANES<F>];
  const size_t first = ((size_t)blockIdx.x * LANES<F> + threadIdx.x) * K;
  if (first >= n) return;
  const int cnt = n - first < (size_t)K ? (int)(n - first) : K;
  for (int j = 0; j < cnt; j++) {
    JacT<F> p = work[first + j];
    const bool is_inf = bls::jac_is_inf(p);
    if (is_inf) p = {gen.x, gen.y, Field<F>::one()};
    inf[first + j] = is_inf ? 1 : 0;
    out[first + j] = {p.x, p.y};
    zs[j][threadIdx.x] = p.z;
  }
  F run = zs[0][threadIdx.x];
  for (int j = 1; j < cnt; j++) run = bls::f_mul(run, zs[j][threadIdx.x]);
  F inv = bls::f_inv(run);  // 1 / (Z_0 ... Z_(cnt-1)): no Z is zero
  for (int j = cnt - 1; j >= 0; j--) {
    F zi = inv;  // 1 / Z_j = inv * Z_0 ... Z_(j-1); the prefix is multiplied up again instead of being kept
    if (j > 0) {
      F pre = zs[0][threadIdx.x];
      for (int i = 1; i < j; i++) pre = bls::f_mul(pre, zs[i][threadIdx.x]);
      zi = bls::f_mul(inv, pre);
      inv = bls::f_mul(inv, zs[j][threadIdx.x]);
    }
    const F zi2 = bls::f_sqr(zi);
    const AffineT<F> a = out[first + j];
    out[first + j] = {bls::f_mul(a.x, zi2), bls::f_mul(a.y, bls::f_mul(zi2, zi))};
  }
}

}  // namespace pointntt
