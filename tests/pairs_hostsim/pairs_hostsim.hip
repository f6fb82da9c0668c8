// Host build of the paired product of csrc/gl.h (its portable form) for tests/test_gl_product_pairs.py: the lazy words of
// mul_lazy2 next to the ones of two mul_lazy, and the paired S-boxes of poseidon.h next to the single one.
#include "../../city-rollup_amd/csrc/poseidon.h"

extern "C" {

// r0, r1: mul_lazy2(a, b, c, d); m0, m1: mul_lazy(a, b), mul_lazy(c, d)
void pairs_mul_lazy2(const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *d, uint64_t *r0, uint64_t *r1, uint64_t *m0,
                     uint64_t *m1, size_t n) {
  for (size_t i = 0; i < n; i++) {
    gl::mul_lazy2(a[i], b[i], c[i], d[i], r0[i], r1[i]);
    m0[i] = gl::mul_lazy(a[i], b[i]);
    m1[i] = gl::mul_lazy(c[i], d[i]);
  }
}

// x, y <- sbox_lazy2(x, y), canonical; sx, sy <- sbox_lazy of each, canonical
void pairs_sbox(uint64_t *x, uint64_t *y, uint64_t *sx, uint64_t *sy, size_t n) {
  for (size_t i = 0; i < n; i++) {
    sx[i] = gl::canon(poseidon::sbox_lazy(x[i]));
    sy[i] = gl::canon(poseidon::sbox_lazy(y[i]));
    poseidon::sbox_lazy2(x[i], y[i]);
    x[i] = gl::canon(x[i]);
    y[i] = gl::canon(y[i]);
  }
}
}
