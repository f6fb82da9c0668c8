// Register radix-16 DIF passes for the Goldilocks NTT (gfx950).
//
// Same pass decomposition as ntt.h (one pass = L butterfly stages over index bits [q, q+L) of a
// 4096-element tile, then the inter-pass twiddle), but the stages run in REGISTERS: every thread
// owns 16 elements and executes up to four radix-2 DIF stages on them per round, so the tile
// crosses LDS once per round (<= 2 exchanges per pass) instead of once per stage, and the first
// load / last store go straight between HBM and registers.
//
// Twiddles inside a round split into (a) a power of omega_16, which in Goldilocks is +-2^(12k)
// (2 has order 192 mod p and omega_16 = 2^156): a shift, never a multiplication; and (b) one
// thread-uniform factor per stage, omega_{2^(f+b+1)}^(r_lo): one table lookup and three squarings
// per round. The last round of a pass (f = 0) needs no multiplications at all.
#pragma once
#include <type_traits>

#include "gl.h"
#include "ntt.h"

namespace ntt16 {

// x * 2^K mod p for a compile-time 0 <= K < 96, x canonical -> canonical
template <int K>
GL_HD uint64_t mul_pow2(uint64_t x) {
  static_assert(K >= 0 && K < 96, "shift out of range");
  if constexpr (K == 0) {
    return x;
  } else if constexpr (K < 64) {
    return gl::reduce128(x << K, x >> (64 - K));
  } else {
    constexpr int J = K - 64;  // x*2^K = (x << J) * 2^64 ;  x << J = y0 + y1*2^64
    uint64_t y0 = J ? (x << J) : x;
    uint64_t y1 = J ? (x >> (64 - J)) : 0;           // < 2^J <= 2^31
    uint64_t t = gl::reduce128(0, y0);               // y0 * 2^64
    return gl::sub(t, y1 << 32);                     // y1 * 2^128 == -y1 * 2^32
  }
}

// (u - v) * omega_16^E  (forward: omega_16 = 2^156, inverse: omega_16^-1 = 2^36), canonical
template <bool INV, int E>
GL_HD uint64_t diff_times_w16(uint64_t u, uint64_t v) {
  constexpr int SH = ((INV ? 36 : 156) * (E & 15)) % 192;
  constexpr bool NEG = SH >= 96;  // 2^96 == -1
  constexpr int K = SH % 96;
  uint64_t d = NEG ? gl::sub(v, u) : gl::sub(u, v);
  return mul_pow2<K>(d);
}

// One DIF stage on the 16 registers at field bit B (pairs m, m + 2^B), with the thread-uniform
// twiddle T (skipped when UNIT_T).
template <bool INV, int B, bool UNIT_T>
GL_HD void stage(uint64_t (&x)[16], uint64_t T) {
#pragma unroll
  for (int m = 0; m < 16; m++) {
    if (m & (1 << B)) continue;
    const int i = m & ((1 << B) - 1);  // position inside the half block
    uint64_t u = x[m], v = x[m + (1 << B)];
    x[m] = gl::add(u, v);
    uint64_t d;
    // omega_{2^(B+1)}^i = omega_16^(i << (3 - B))
    switch (i << (3 - B)) {
      case 0: d = diff_times_w16<INV, 0>(u, v); break;
      case 1: d = diff_times_w16<INV, 1>(u, v); break;
      case 2: d = diff_times_w16<INV, 2>(u, v); break;
      case 3: d = diff_times_w16<INV, 3>(u, v); break;
      case 4: d = diff_times_w16<INV, 4>(u, v); break;
      case 5: d = diff_times_w16<INV, 5>(u, v); break;
      case 6: d = diff_times_w16<INV, 6>(u, v); break;
      default: d = diff_times_w16<INV, 7>(u, v); break;
    }
    x[m + (1 << B)] = UNIT_T ? d : gl::mul(d, T);
  }
}

// ---- the same arithmetic with independent chains issued in PAIRS -----------------------------------------------------------------
// A lone `gl::mul` is three basic blocks and three `s_nop 1`, a lone `mul_pow2` two and a branch; with between one and two waves of a
// SIMD ready to issue, those wait states are the wave's own. The passes below hand two independent chains at a time to
// `gl::mul_lazy2` / `gl::reduce128_lazy2` (one branch, the siblings' instructions as wait states): the same field elements, bit for
// bit, in the same number of VALU instructions. NTT16_SINGLE_CHAINS restores the one-chain forms for the A/B (and
// NTT16_STAGE_TWIDDLES, the older A/B, implies them).
#if defined(NTT16_SINGLE_CHAINS) || defined(NTT16_STAGE_TWIDDLES)
#define NTT16_PAIRS 0
#else
#define NTT16_PAIRS 1
#endif

// x <- x 2^K0, y <- y 2^K1, both shifts in the same form of `mul_pow2` (both below 64, or both from 64 on)
template <int K0, int K1>
GL_HD void mul_pow2_2(uint64_t &x, uint64_t &y) {
  static_assert(K0 > 0 && K0 < 96 && K1 > 0 && K1 < 96 && (K0 < 64) == (K1 < 64), "two shifts of one form");
  if constexpr (K0 < 64) {
    gl::reduce128_2(x << K0, x >> (64 - K0), y << K1, y >> (64 - K1), x, y);
  } else {
    constexpr int J0 = K0 - 64, J1 = K1 - 64;
    const uint64_t x0 = J0 ? (x << J0) : x, x1 = J0 ? (x >> (64 - J0)) : 0;
    const uint64_t y0 = J1 ? (y << J1) : y, y1 = J1 ? (y >> (64 - J1)) : 0;
    uint64_t t, u;
    gl::reduce128_2(0, x0, 0, y0, t, u);
    x = gl::sub(t, x1 << 32);
    y = gl::sub(u, y1 << 32);
  }
}

// omega_16^E = +-2^K: the shift in [0, 192), 2^96 == -1
template <bool INV>
constexpr int w16_shift(int E) { return ((INV ? 36 : 156) * (E & 15)) % 192; }

// Which differences of the stage at field bit B are shifted together: registers a[i], b[i] (b[i] < 0: a lone one), in register order,
// a shift pairing with the next one of its form.
struct ShiftPlan {
  int a[8], b[8], n;
};
template <bool INV, int B>
constexpr ShiftPlan shift_plan() {
  ShiftPlan p{};
  int pend[2] = {-1, -1};
  for (int m = 0; m < 16; m++) {
    if (m & (1 << B)) continue;
    const int K = w16_shift<INV>((m & ((1 << B) - 1)) << (3 - B)) % 96;
    if (K == 0) continue;
    const int form = K >= 64, reg = m + (1 << B);
    if (pend[form] < 0) {
      pend[form] = reg;
    } else {
      p.a[p.n] = pend[form];
      p.b[p.n++] = reg;
      pend[form] = -1;
    }
  }
  for (int form = 0; form < 2; form++)
    if (pend[form] >= 0) {
      p.a[p.n] = pend[form];
      p.b[p.n++] = -1;
    }
  return p;
}
// the shift of the difference held in register `reg` (bit B set)
template <bool INV, int B>
constexpr int reg_shift(int reg) { return w16_shift<INV>((reg & ((1 << B) - 1)) << (3 - B)) % 96; }

template <bool INV, int B, int I = 0>
GL_HD void apply_shifts(uint64_t (&x)[16]) {
  constexpr ShiftPlan p = shift_plan<INV, B>();
  if constexpr (I < p.n) {
    constexpr int ra = p.a[I], rb = p.b[I];
    if constexpr (rb < 0) x[ra] = mul_pow2<reg_shift<INV, B>(ra)>(x[ra]);
    else mul_pow2_2<reg_shift<INV, B>(ra), reg_shift<INV, B>(rb)>(x[ra], x[rb]);
    apply_shifts<INV, B, I + 1>(x);
  }
}

// `stage<INV, B, true>` with its non-trivial shifts two at a time: all sums and signed differences first, then the shifts
template <bool INV, int B>
GL_HD void stage_pairs(uint64_t (&x)[16]) {
#pragma unroll
  for (int m = 0; m < 16; m++) {
    if (m & (1 << B)) continue;
    const bool neg = w16_shift<INV>((m & ((1 << B) - 1)) << (3 - B)) >= 96;
    const uint64_t u = x[m], v = x[m + (1 << B)];
    x[m] = gl::add(u, v);
    x[m + (1 << B)] = neg ? gl::sub(v, u) : gl::sub(u, v);
  }
  apply_shifts<INV, B>(x);
}

// e(m) of `round16`, and the K-th register (in register order) whose e(m) is E
constexpr int round_exp(int NSTAGES, int m) {
  int em = 0;  // bit B of m (B = 3 .. 4 - NSTAGES) weighs 2^(3 - B)
  for (int B = 3; B >= 4 - NSTAGES; B--) em += ((m >> B) & 1) << (3 - B);
  return em;
}
constexpr int round_reg(int NSTAGES, int E, int K) {
  for (int m = 0; m < 16; m++)
    if (round_exp(NSTAGES, m) == E && K-- == 0) return m;
  return -1;
}
// registers K, K + 1, ... of exponent E times pw, two at a time; an odd one out stays single
template <int NSTAGES, int E, int K>
GL_HD void apply_power(uint64_t (&x)[16], uint64_t pw) {
  constexpr int CNT = 16 >> NSTAGES;
  if constexpr (K + 1 < CNT) {
    constexpr int m0 = round_reg(NSTAGES, E, K), m1 = round_reg(NSTAGES, E, K + 1);
    gl::mul2(x[m0], pw, x[m1], pw, x[m0], x[m1]);
    apply_power<NSTAGES, E, K + 2>(x, pw);
  } else if constexpr (K < CNT) {
    constexpr int m0 = round_reg(NSTAGES, E, K);
    x[m0] = gl::mul(x[m0], pw);
  }
}
// The walk of `round16`: pw = T3^E. The step to T3^(E + 1) and the first application of T3^E read the same pw and form a pair; what is
// left of this exponent's applications pairs among itself. 14 + 15 products for four stages, as in the one-chain walk.
template <int NSTAGES, int E = 1>
GL_HD void walk_powers(uint64_t (&x)[16], uint64_t pw, uint64_t T3) {
  constexpr int LAST = (1 << NSTAGES) - 1;
  if constexpr (E < LAST) {
    constexpr int m0 = round_reg(NSTAGES, E, 0);
    uint64_t next, r;
    gl::mul_lazy2(pw, T3, x[m0], pw, next, r);
    x[m0] = gl::canon(r);
    apply_power<NSTAGES, E, 1>(x, pw);
    walk_powers<NSTAGES, E + 1>(x, next, T3);
  } else {
    apply_power<NSTAGES, E, 0>(x, pw);
  }
}

// NSTAGES DIF stages on the top bits of the 4-bit register field. T3 = omega_{2^(f+4)}^(r_lo).
// The thread-uniform factor of stage B is T_B = T3^(2^(3-B)), and it multiplies ALL the differences of its stage: every later butterfly
// pairs two values that carry the same T_B, so the factor commutes with the rest of the round. The stages therefore run with their
// shift twiddles only, and register m is multiplied ONCE at the end by T3^e(m), e(m) = sum over the round's stages of m_B 2^(3-B) —
// the powers T3^1 .. T3^(2^NSTAGES - 1) walked in order by one lazy product each: 14 + 15 products for four stages where the
// factor-per-stage form took 3 squarings + 32 (NTT16_STAGE_TWIDDLES restores it for the A/B). Same field elements, bit for bit.
template <bool INV, int NSTAGES, bool UNIT_T>
GL_HD void round16(uint64_t (&x)[16], uint64_t T3) {
#if defined(NTT16_STAGE_TWIDDLES)
  uint64_t T2 = UNIT_T ? 1 : gl::sqr(T3);
  stage<INV, 3, UNIT_T>(x, T3);
  if constexpr (NSTAGES >= 2) {
    stage<INV, 2, UNIT_T>(x, T2);
  }
  if constexpr (NSTAGES >= 3) {
    uint64_t T1 = UNIT_T ? 1 : gl::sqr(T2);
    stage<INV, 1, UNIT_T>(x, T1);
    if constexpr (NSTAGES >= 4) {
      uint64_t T0 = UNIT_T ? 1 : gl::sqr(T1);
      stage<INV, 0, UNIT_T>(x, T0);
    }
  }
#elif NTT16_PAIRS
  stage_pairs<INV, 3>(x);
  if constexpr (NSTAGES >= 2) stage_pairs<INV, 2>(x);
  if constexpr (NSTAGES >= 3) stage_pairs<INV, 1>(x);
  if constexpr (NSTAGES >= 4) stage_pairs<INV, 0>(x);
  if constexpr (!UNIT_T) walk_powers<NSTAGES>(x, T3, T3);
#else
  stage<INV, 3, true>(x, 1);
  if constexpr (NSTAGES >= 2) stage<INV, 2, true>(x, 1);
  if constexpr (NSTAGES >= 3) stage<INV, 1, true>(x, 1);
  if constexpr (NSTAGES >= 4) stage<INV, 0, true>(x, 1);
  if constexpr (!UNIT_T) {
    uint64_t pw = T3;  // T3^e, lazy from the second on (a product takes any u64)
#pragma unroll
    for (int e = 1; e < (1 << NSTAGES); e++) {
      if (e > 1) pw = gl::mul_lazy(pw, T3);
#pragma unroll
      for (int m = 0; m < 16; m++) {
        int em = 0;  // e(m): bit B of m (B = 3 .. 4 - NSTAGES) weighs 2^(3 - B)
        for (int B = 3; B >= 4 - NSTAGES; B--) em += ((m >> B) & 1) << (3 - B);
        if (em == e) x[m] = gl::mul(x[m], pw);
      }
    }
  }
#endif
}

constexpr int LOG_TILE = 12;
constexpr int THREADS = 1 << (LOG_TILE - 4);  // 256

__device__ __forceinline__ int pad(int p) { return p + (p >> 4); }

// Two ways for the tile to cross LDS between rounds.
// HALF = false: all 4096 elements at once (34 KB per workgroup: four workgroups per CU, four waves per SIMD) and one barrier.
// HALF = true: one 32-bit half at a time (17 KB; low words, barrier, high words) — with 85-89 VGPRs that is five waves per
// SIMD, at the price of two more barriers and 32-bit LDS accesses. A pass that has the GPU to itself is bound by that
// occupancy (56-66 % of every wave's cycles are memory waits; with the LDS of a workgroup grown so that only three fit, the
// passes run 20-22 % slower; with HALF the 135 x 2^20 passes go 0.85 -> 0.74 ms and 1.05 -> 0.89 ms). The 2^12-2^15 transforms of
// a proof run beside the kernels of the other contexts, which hide the waits anyway; there the extra barriers only cost
// (three contexts x batch 32: 1 963 -> 1 918 proofs/s with HALF everywhere), so cityprover.hip picks HALF by transform size.
// x[m] sits at tile position Pw + (m << Fw) and is needed at Pr + (m << Fr). P has zeros in bits [F, F + 4) (that is where m
// goes), so pad(P + (m << F)) = pad(P) + pad(m << F): one address register per side and sixteen compile-time offsets.
template <bool HALF, typename T>
__device__ __forceinline__ void exchange(T *tile, uint64_t (&x)[16], int Pw, int Fw, int Pr, int Fr) {
  T *w = tile + pad(Pw), *r = tile + pad(Pr);
  if constexpr (HALF) {
    uint32_t lo[16];
#pragma unroll
    for (int m = 0; m < 16; m++) w[pad(m << Fw)] = gl::lo32(x[m]);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 16; m++) lo[m] = r[pad(m << Fr)];
    __syncthreads();  // every low word has been read before a high word takes its place
#pragma unroll
    for (int m = 0; m < 16; m++) w[pad(m << Fw)] = gl::hi32(x[m]);
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 16; m++) x[m] = gl::pack(lo[m], r[pad(m << Fr)]);
  } else {
#pragma unroll
    for (int m = 0; m < 16; m++) w[pad(m << Fw)] = x[m];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 16; m++) x[m] = r[pad(m << Fr)];
  }
  // no barrier at the end: the next writes of a thread go to the positions it has just read (its own set)
}

// global element index of tile position `pos`
template <int L, int C, bool ROWS>
__device__ __forceinline__ size_t gidx(int pos, uint32_t tile_id, int q) {
  if (ROWS) return ((size_t)tile_id << LOG_TILE) + pos;  // q == 0: the tile is contiguous
  uint32_t r = pos >> C, o = (tile_id << C) + (pos & ((1 << C) - 1));
  return ((size_t)(o >> q) << (q + L)) | ((size_t)r << q) | (o & ((1u << q) - 1));
}

// One pass, L stages, tile = 2^L rows x 2^C outer indices (L + C == 12).
// HALF passes ask for five waves per SIMD: 96 VGPRs, which they fit without spilling (85 / 89) now that the LDS and row
// addresses are a base plus compile-time offsets; at six (80 VGPRs) 10-20 registers spill and the passes are slower again
// (0.79 / 1.02 ms per 135-column step against 0.74 / 0.89). The one-round column pass (L = 4: no exchange, 16 + 15 epilogue
// twiddles live at once) would spill a dozen registers at five and keeps the default.
#ifndef NTT16_MIN_WAVES
#define NTT16_MIN_WAVES 5
#endif
template <int L, int C, bool ROWS, bool INV, bool HALF>
__global__ __launch_bounds__(THREADS, (HALF && !(L == 4 && !ROWS)) ? NTT16_MIN_WAVES : 1) void k_dif_pass16(ntt::PassArgs a) {
  static_assert(L + C == LOG_TILE && L >= 4, "tile shape");
  using tile_t = typename std::conditional<HALF, uint32_t, uint64_t>::type;
  __shared__ tile_t tile[(1 << LOG_TILE) + (1 << (LOG_TILE - 4))];
  constexpr int B0 = ((L - 1) % 4) + 1;       // stages of the first round; the rest are full rounds
  constexpr int NROUNDS = 1 + (L - B0) / 4;
  const int t = threadIdx.x;
  const int q = a.q;
  uint64_t *poly = a.data + (size_t)blockIdx.y * a.stride + (size_t)blockIdx.z * a.block_stride;
  const uint64_t *in = (a.first && a.src) ? a.src + (size_t)blockIdx.y * a.src_stride : poly;
  const uint64_t *ptab =
      (a.first && a.ptab) ? a.ptab + ((size_t)ntt::bitrev(blockIdx.z, a.block_bits) << a.log_n) : nullptr;
  uint64_t x[16];

  // ---- round 0: field = r-bits [L-4, L) --------------------------------------------------
  {
    constexpr int f = L - 4;                  // r-bit position of the field
    constexpr int F = ROWS ? f : C + f;       // position in tile-position space
    const int P = ((t >> F) << (F + 4)) | (t & ((1 << F) - 1));
    // ROWS: the tile is contiguous — a wave-uniform base and a 32-bit position instead of a 64-bit index per element
    const uint64_t *in_t = ROWS ? in + ((size_t)blockIdx.x << LOG_TILE) : in;
    const uint64_t *ptab_t = (ROWS && ptab) ? ptab + ((size_t)blockIdx.x << LOG_TILE) : ptab;
#if !NTT16_PAIRS
#pragma unroll
    for (int m = 0; m < 16; m++) {
      const size_t idx = gidx<L, C, ROWS>(P + (m << F), blockIdx.x, q);
      uint64_t v = ROWS ? in_t[P + (m << F)] : in[idx];
      if (ptab) v = gl::mul(v, ROWS ? ptab_t[P + (m << F)] : ptab[idx]);
      else if (a.coset_pre && a.first) v = gl::mul(v, ntt::pow_table(a.stab, idx));
      x[m] = v;
    }
#else
#pragma unroll
    for (int m = 0; m < 16; m += 2) {  // the products on load, two registers at a time
      const int p0 = P + (m << F), p1 = P + ((m + 1) << F);
      const size_t idx0 = gidx<L, C, ROWS>(p0, blockIdx.x, q), idx1 = gidx<L, C, ROWS>(p1, blockIdx.x, q);
      uint64_t v0 = ROWS ? in_t[p0] : in[idx0], v1 = ROWS ? in_t[p1] : in[idx1];
      if (ptab) gl::mul2(v0, ROWS ? ptab_t[p0] : ptab[idx0], v1, ROWS ? ptab_t[p1] : ptab[idx1], v0, v1);
      else if (a.coset_pre && a.first) gl::mul2(v0, ntt::pow_table(a.stab, idx0), v1, ntt::pow_table(a.stab, idx1), v0, v1);
      x[m] = v0;
      x[m + 1] = v1;
    }
#endif
    if constexpr (f == 0) {
      round16<INV, B0, true>(x, 1);
    } else {
      const int r = ROWS ? (P & ((1 << L) - 1)) : (P >> C);
      const uint32_t r_lo = r & ((1 << f) - 1);
      uint64_t T3 = ntt::pow_table(a.wtab, (uint64_t)r_lo << (a.log_n - f - 4));
      round16<INV, B0, false>(x, T3);
    }
  }
  // ---- middle / last rounds -----------------------------------------------------------------
  constexpr int Flast = ROWS ? 0 : C;
  constexpr int F0 = ROWS ? (L - 4) : C + (L - 4);
  int Plast = ((t >> F0) << (F0 + 4)) | (t & ((1 << F0) - 1));  // round 0's positions; the last round's after the loop
  int Fprev = F0;
#pragma unroll
  for (int k = 1; k < NROUNDS; k++) {
    const int f = L - B0 - 4 * k;             // compile-time after unrolling
    const int F = ROWS ? f : C + f;
    const int P = ((t >> F) << (F + 4)) | (t & ((1 << F) - 1));
    exchange<HALF>(tile, x, Plast, Fprev, P, F);
    if (f == 0) {
      round16<INV, 4, true>(x, 1);
    } else {
      const int r = ROWS ? (P & ((1 << L) - 1)) : (P >> C);
      const uint32_t r_lo = r & ((1 << f) - 1);
      uint64_t T3 = ntt::pow_table(a.wtab, (uint64_t)r_lo << (a.log_n - f - 4));
      round16<INV, 4, false>(x, T3);
    }
    Plast = P;
    Fprev = F;
  }
  // ---- epilogue: inter-pass twiddle, scaling, store -----------------------------------------
  // the thread holds r = r_base + m (m = 0..15) for one (cc): k_loc(m) = rev_L(r_base) + rev4(m) << (L-4)
  {
    const int P = Plast;
    if (!ROWS && q > 0) {
      const uint32_t cc = P & ((1 << C) - 1);
      const uint32_t r_base = P >> C;
      const uint32_t o = (blockIdx.x << C) + cc;
      const uint32_t lo = o & ((1u << q) - 1);
      if (lo) {
        // omega_{2^(q+L)}^(lo * k_loc) = W0 * G^rev4(m),  W0 = w^(lo*rev_L(r_base)),  G = w^(lo << (L-4))
        const int sh = a.log_n - q - L;
        uint64_t W0 = ntt::pow_table(a.wtab, ((uint64_t)lo * ntt::bitrev(r_base, L)) << sh);
        uint64_t G = ntt::pow_table(a.wtab, ((uint64_t)lo << (L - 4)) << sh);
        // walk j = 0..15 and apply to register m = rev4(j)
        uint64_t w = W0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
          const int m = ((j & 1) << 3) | ((j & 2) << 1) | ((j & 4) >> 1) | ((j & 8) >> 3);
#if NTT16_PAIRS
          if (j < 15) {  // the application and the walk step read the same w: a pair
            uint64_t r, next;
            gl::mul_lazy2(x[m], w, w, G, r, next);
            x[m] = gl::canon(r);
            w = next;
          } else {
            x[m] = gl::mul(x[m], w);
          }
#else
          x[m] = gl::mul(x[m], w);
          if (j < 15) w = gl::mul_lazy(w, G);  // the running power stays lazy: a product takes any u64
#endif
        }
      }
    }
    if (a.last && a.scale) {
#if NTT16_PAIRS
#pragma unroll
      for (int m = 0; m < 16; m += 2) gl::mul2(x[m], a.scale, x[m + 1], a.scale, x[m], x[m + 1]);
#else
#pragma unroll
      for (int m = 0; m < 16; m++) x[m] = gl::mul(x[m], a.scale);
#endif
    }
    if (ROWS && a.natural_out) {
      // single-pass transform: position r holds X[rev_L(r)]; un-permute through LDS (HALF: low words, then high words), store coalesced
      __syncthreads();
      if constexpr (HALF) {
        uint32_t lo[16];
#pragma unroll
        for (int m = 0; m < 16; m++) tile[pad((int)ntt::bitrev((uint32_t)(P + m), L))] = gl::lo32(x[m]);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) lo[m] = tile[pad(t + (m << (LOG_TILE - 4)))];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) tile[pad((int)ntt::bitrev((uint32_t)(P + m), L))] = gl::hi32(x[m]);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) {
          int pos = t + (m << (LOG_TILE - 4));
          poly[((size_t)blockIdx.x << LOG_TILE) + pos] = gl::pack(lo[m], tile[pad(pos)]);
        }
      } else {
#pragma unroll
        for (int m = 0; m < 16; m++) tile[pad((int)ntt::bitrev((uint32_t)(P + m), L))] = x[m];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) {
          int pos = t + (m << (LOG_TILE - 4));
          poly[((size_t)blockIdx.x << LOG_TILE) + pos] = tile[pad(pos)];
        }
      }
      return;
    }
    if (ROWS && a.staged_store) {
      // The last round leaves every thread 16 CONSECUTIVE elements: stored directly, one instruction of a wave writes 8 bytes
      // into each of 64 different 128-byte lines. Through LDS (same positions, read back lane-contiguous) a wave writes 512
      // contiguous bytes per instruction.
      uint64_t *out_t = poly + ((size_t)blockIdx.x << LOG_TILE);
      __syncthreads();
      if constexpr (HALF) {
        uint32_t lo[16];
        tile_t *w = tile + pad(P);
#pragma unroll
        for (int m = 0; m < 16; m++) w[pad(m)] = gl::lo32(x[m]);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) lo[m] = tile[pad(t + (m << (LOG_TILE - 4)))];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) w[pad(m)] = gl::hi32(x[m]);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) {
          const int pos = t + (m << (LOG_TILE - 4));
          out_t[pos] = gl::pack(lo[m], tile[pad(pos)]);
        }
      } else {
        tile_t *w = tile + pad(P);
#pragma unroll
        for (int m = 0; m < 16; m++) w[pad(m)] = x[m];
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 16; m++) {
          const int pos = t + (m << (LOG_TILE - 4));
          out_t[pos] = tile[pad(pos)];
        }
      }
    } else if (ROWS) {
      uint64_t *out_t = poly + ((size_t)blockIdx.x << LOG_TILE) + P;
#pragma unroll
      for (int m = 0; m < 16; m++) out_t[m << Flast] = x[m];
    } else {
#pragma unroll
      for (int m = 0; m < 16; m++) poly[gidx<L, C, ROWS>(P + (m << Flast), blockIdx.x, q)] = x[m];
    }
  }
}

// pre-scale table for the LDE: T[r][j] = (shift * omega_N^r)^j, r < 2^rate_bits, j < n
__global__ void k_fill_prescale(uint64_t *__restrict__ T, int log_n, int rate_bits,
                                const uint64_t *__restrict__ stab, const uint64_t *__restrict__ wtabN) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> (log_n + rate_bits)) return;
  uint64_t j = i & (((size_t)1 << log_n) - 1), r = i >> log_n;
  T[i] = gl::mul(ntt::pow_table(stab, j), ntt::pow_table(wtabN, (r * j) & (((uint64_t)1 << (log_n + rate_bits)) - 1)));
}

}  // namespace ntt16
