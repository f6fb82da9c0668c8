// Host build of the paired forms the radix-16 NTT passes use (their portable forms) for tests/test_gl_reduce_pairs.py: the lazy
// words of gl::reduce128_lazy2 next to the ones of two reduce128_lazy, the canonical wrappers, and ntt16::mul_pow2_2 next to two
// mul_pow2.
#include "../../city-rollup_amd/csrc/ntt16.h"

namespace {
template <int KA, int KB>
void run_pow2(const uint64_t *x, const uint64_t *y, uint64_t *px, uint64_t *py, uint64_t *sx, uint64_t *sy, size_t n) {
  for (size_t i = 0; i < n; i++) {
    px[i] = x[i];
    py[i] = y[i];
    ntt16::mul_pow2_2<KA, KB>(px[i], py[i]);
    sx[i] = ntt16::mul_pow2<KA>(x[i]);
    sy[i] = ntt16::mul_pow2<KB>(y[i]);
  }
}
}  // namespace

extern "C" {

// r: reduce128_lazy2; s: two reduce128_lazy; c: reduce128_2 (canonical)
void np_reduce2(const uint64_t *lo_a, const uint64_t *hi_a, const uint64_t *lo_b, const uint64_t *hi_b, uint64_t *r0, uint64_t *r1,
                uint64_t *s0, uint64_t *s1, uint64_t *c0, uint64_t *c1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    gl::reduce128_lazy2(lo_a[i], hi_a[i], lo_b[i], hi_b[i], r0[i], r1[i]);
    s0[i] = gl::reduce128_lazy(lo_a[i], hi_a[i]);
    s1[i] = gl::reduce128_lazy(lo_b[i], hi_b[i]);
    gl::reduce128_2(lo_a[i], hi_a[i], lo_b[i], hi_b[i], c0[i], c1[i]);
  }
}

// r: mul2 (canonical); s: two mul
void np_mul2(const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *d, uint64_t *r0, uint64_t *r1, uint64_t *s0,
             uint64_t *s1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    gl::mul2(a[i], b[i], c[i], d[i], r0[i], r1[i]);
    s0[i] = gl::mul(a[i], b[i]);
    s1[i] = gl::mul(c[i], d[i]);
  }
}

// p: mul_pow2_2<ka, kb>(x, y); s: mul_pow2<ka>(x), mul_pow2<kb>(y). 0, or -1 for a pair of shifts that is not one form
int np_pow2_2(int ka, int kb, const uint64_t *x, const uint64_t *y, uint64_t *px, uint64_t *py, uint64_t *sx, uint64_t *sy, size_t n) {
#define CASE(A, B)                                   \
  if (ka == A && kb == B) {                          \
    run_pow2<A, B>(x, y, px, py, sx, sy, n);         \
    return 0;                                        \
  }
#define ROW(A) CASE(A, 12) CASE(A, 24) CASE(A, 36) CASE(A, 48) CASE(A, 60)
  ROW(12) ROW(24) ROW(36) ROW(48) ROW(60)
  CASE(72, 72) CASE(72, 84) CASE(84, 72) CASE(84, 84)
#undef ROW
#undef CASE
  return -1;
}
}
