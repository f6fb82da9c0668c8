// Batched fixed-base scalar multiplication over BLS12-381 G1 and G2 (the point sets of a Groth16
// proving key are n multiples of ONE base), templates over the coordinate field like msm.h:
//
//   k_table    affine multiples d * 2^(8 w) * base, 1 <= d <= 128, w < 33: once per base
//   k_mul      one lane per K scalars: each scalar is walked through its 33 signed byte digits with the XYZZ mixed addition of
//              the bucket sums (msm::bucket_add), then the K results are brought to the affine form the MSMs read with ONE
//              inversion (Montgomery's trick)
//
// Signed digits: k = sum_w 2^(8 w) d_w with |d_w| <= 128 - a byte above 128 becomes byte - 256 and carries into the next
// window - so a window needs 128 table entries, not 255; 256 bits and the last carry make 33 windows. A digit is a byte of
// the little-endian scalar: no shifts across words. Exact integer arithmetic on any 256-bit scalar.
#pragma once
#include "msm.h"

namespace fixedbase {

using bls::AffineT;
using bls::Field;
using bls::JacT;

constexpr int WINDOW_BITS = 8;
constexpr int WINDOWS = 33;                                // 32 bytes and the carry out of the last one
constexpr int HALF = 1 << (WINDOW_BITS - 1);               // table entries per window: d = 1 .. 128
constexpr size_t TABLE_POINTS = (size_t)WINDOWS * HALF;
constexpr int K = 4;                                       // results that share one inversion
// lanes of a workgroup and waves per SIMD asked of the compiler: G1 is held to 256 registers (two waves per SIMD, where
// k_bucket_sum<Fp> runs), G2 needs the whole register file
template <class F> constexpr unsigned LANES = sizeof(F) == sizeof(bls::Fp) ? 128 : 64;
template <class F> constexpr unsigned WAVES = sizeof(F) == sizeof(bls::Fp) ? 2 : 1;

// signed digit of window w of the scalar at k (32 little-endian bytes), given the carry of the window below; updates the carry
GL_HD int signed_digit(const uint8_t *k, int w, uint32_t &carry) {
  const uint32_t raw = (w < 32 ? k[w] : 0u) + carry;
  if (raw > (uint32_t)HALF) { carry = 1; return (int)raw - 2 * HALF; }
  carry = 0;
  return (int)raw;
}
// all the digits of a scalar (the CPU tests re-sum them)
GL_HD void recode(const uint8_t *k, int digits[WINDOWS]) {
  uint32_t carry = 0;
  for (int w = 0; w < WINDOWS; w++) digits[w] = signed_digit(k, w, carry);
}

// table[w][d - 1] = d * bases[w], bases[w] = 2^(8 w) * base (Jacobian, from the host). A multiple that is the point at infinity
// (a base of small order, outside the prime-order subgroup) cannot be an affine entry: it is counted, and the host refuses.
template <class F>
__global__ __launch_bounds__(64) void k_table(const JacT<F> *__restrict__ bases, AffineT<F> *__restrict__ table,
                                              uint32_t *__restrict__ n_infinite) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= TABLE_POINTS) return;
  const JacT<F> p = bls::jac_mul_small(bases[t / HALF], (uint32_t)(t % HALF) + 1);
  if (bls::jac_is_inf(p)) {
    atomicAdd(n_infinite, 1u);
    table[t] = {Field<F>::zero(), Field<F>::zero()};
    return;
  }
  table[t] = bls::jac_to_affine(p);
}

// out[i] = scalars[i] * base, affine, Montgomery coordinates; inf[i] = 1 where that is the point at infinity, and the entry then
// holds the base (a valid point that the MSMs skip). Lane t owns the scalars t K .. t K + K - 1. Of a result (X, Y, ZZ, ZZZ) the
// lane keeps X and Y ZZZ in the output entry itself and ZZ in its LDS column; after the last scalar it inverts the product of
// its ZZ and writes x = X / ZZ, y = Y ZZZ / ZZ^3 (ZZZ^2 = ZZ^3). No barrier: a lane reads only what it wrote.
template <class F>
__global__ __launch_bounds__(LANES<F>, WAVES<F>) void k_mul(const AffineT<F> *__restrict__ table, const uint8_t *__restrict__ scalars, size_t n,
                                               AffineT<F> base, AffineT<F> *__restrict__ out, uint8_t *__restrict__ inf) {
  __shared__ F zz[K][LANES<F>];
  const size_t first = ((size_t)blockIdx.x * LANES<F> + threadIdx.x) * K;
  if (first >= n) return;
  const int cnt = n - first < (size_t)K ? (int)(n - first) : K;
  for (int j = 0; j < cnt; j++) {
    const uint8_t *k = scalars + 32 * (first + j);
    bls::XyzzT<F> acc = bls::xyzz_inf<F>();
    uint32_t carry = 0;
    for (int w = 0; w < WINDOWS; w++) {
      const int d = signed_digit(k, w, carry);
      if (d == 0) continue;
      AffineT<F> q = table[(size_t)w * HALF + (d < 0 ? -d : d) - 1];
      if (d < 0) q.y = bls::f_sub(Field<F>::zero(), q.y);
      acc = msm::bucket_add(acc, q);
    }
    const bool is_inf = bls::f_is_zero(acc.zz);  // exactly zero: set by xyzz_inf alone
    if (is_inf) acc = {base.x, base.y, Field<F>::one(), Field<F>::one()};
    inf[first + j] = is_inf ? 1 : 0;
#if !defined(BLS_CANONICAL_ACCUMULATION)
    acc = bls::xyzz_canon(acc);
#endif
    out[first + j] = {acc.x, bls::f_mul(acc.y, acc.zzz)};
    zz[j][threadIdx.x] = acc.zz;
  }
  F run = zz[0][threadIdx.x];
  for (int j = 1; j < cnt; j++) run = bls::f_mul(run, zz[j][threadIdx.x]);
  F inv = bls::f_inv(run);  // 1 / (ZZ_0 ... ZZ_(cnt-1)): no ZZ is zero
  for (int j = cnt - 1; j >= 0; j--) {
    // 1 / ZZ_j = inv * ZZ_0 ... ZZ_(j-1); the prefix is multiplied up again (at most K - 2 products) instead of being kept
    F zi = inv;
    if (j > 0) {
      F pre = zz[0][threadIdx.x];
      for (int i = 1; i < j; i++) pre = bls::f_mul(pre, zz[i][threadIdx.x]);
      zi = bls::f_mul(inv, pre);
      inv = bls::f_mul(inv, zz[j][threadIdx.x]);
    }
    const F zi3 = bls::f_mul(bls::f_sqr(zi), zi);
    const AffineT<F> a = out[first + j];
    out[first + j] = {bls::f_mul(a.x, zi), bls::f_mul(a.y, zi3)};
  }
}

}  // namespace fixedbase
