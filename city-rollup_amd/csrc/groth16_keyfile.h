// One point of a Groth16 key file (keyfile.hip has the file's layout): from the key's internal form to the file's and back.
// __host__ __device__ throughout, like bls_sqrt.h, on which it stands: the kernels of keyfile.hip are one call of these per
// lane, and tests/keyfilesim runs this very text on the CPU against Python integers.
// In the file a point of the five sets is a compressed element - W 32-bit words, W = 12 (G1) or 24 (G2: a0, then a1 with the
// flags on a1): x little-endian, 0x80 on the last byte where y is the larger root, 0x40 alone for infinity - or, in a raw file,
// 2 W words of affine canonical coordinates, all zero for infinity.
#pragma once
#include "pairing.h"
#include "bls_sqrt.h"

namespace keyfile {

using bls::AffineT;
using bls::Field;
using bls::Fp;
using bls::Fp2;

// why a point of a file is refused: 1 .. 3 are the classes of bls_sqrt.h
enum { ST_OK = 0, ST_FLAG = 1, ST_RANGE = 2, ST_NO_POINT = 3, ST_INFINITY = 4, ST_DISAGREE = 5, ST_TORSION = 6 };

GL_HD bool f_sqrt(const Fp &a, Fp *r) { return blssqrt::fp_sqrt(a, r); }
GL_HD bool f_sqrt(const Fp2 &a, Fp2 *r) { return blssqrt::fp2_sqrt(a, r); }
GL_HD bool f_is_larger(const Fp &y) { return blssqrt::fp_is_larger(y); }
GL_HD bool f_is_larger(const Fp2 &y) { return blssqrt::fp2_is_larger(y); }
GL_HD Fp f_neg(const Fp &a) { return blssqrt::fp_neg(a); }
GL_HD Fp2 f_neg(const Fp2 &a) { return pairing::fp2_neg(a); }

// internal form plus flag -> the file's form at o (W words, or 2 W raw)
template <class F>
GL_HD void pack_point(const AffineT<F> &a, bool is_inf, bool raw, uint32_t *o) {
  constexpr int W = Field<F>::WORDS;
  if (is_inf) {
    for (int k = 0; k < (raw ? 2 * W : W); k++) o[k] = 0;
    if (!raw) o[W - 1] = 0x40000000u;
    return;
  }
  uint32_t x[W];
  Field<F>::to_canonical(a.x, x);
  if (raw) {
    uint32_t y[W];
    Field<F>::to_canonical(a.y, y);
    for (int k = 0; k < W; k++) o[k] = x[k];
    for (int k = 0; k < W; k++) o[W + k] = y[k];
  } else {
    if (f_is_larger(a.y)) x[W - 1] |= 0x80000000u;
    for (int k = 0; k < W; k++) o[k] = x[k];
  }
}

// one compressed element -> the point in the internal form, or infinity: x from its words, y the root the 0x80 bit names
template <class F>
GL_HD int decompress(const uint32_t *src, AffineT<F> &a, bool &is_inf) {
  constexpr int W = Field<F>::WORDS;
  uint32_t w[W];
  for (int k = 0; k < W; k++) w[k] = src[k];
  const uint32_t flags = w[W - 1] >> 30;  // 0x80, 0x40 of the last byte
  w[W - 1] &= 0x3FFFFFFFu;
  is_inf = false;
  if (flags & 1) {
    uint32_t rest = flags & 2;
    for (int k = 0; k < W; k++) rest |= w[k];
    if (rest) return ST_FLAG;  // 0x40 with anything else set
    is_inf = true;
    return ST_OK;
  }
  if (W == 24 && (w[11] >> 30) != 0) return ST_FLAG;  // a0 of a G2 element carries no flags
  for (int h = 0; h < W / 12; h++)
    if (!pairing::words_below_p(w + 12 * h)) return ST_RANGE;
  a.x = Field<F>::from_canonical(w);
  if (!f_sqrt(bls::f_add(bls::f_mul(bls::f_sqr(a.x), a.x), Field<F>::curve_b()), &a.y)) return ST_NO_POINT;
  if (f_is_larger(a.y) != ((flags & 2) != 0)) a.y = f_neg(a.y);
  return ST_OK;
}

// the file's form at s -> ST_OK with the point in `a` or with is_inf set, else ST_FLAG, ST_RANGE or ST_NO_POINT. A raw point
// gets the curve equation in place of the root.
template <class F>
GL_HD int unpack_point(const uint32_t *s, bool raw, AffineT<F> &a, bool &is_inf) {
  constexpr int W = Field<F>::WORDS;
  if (!raw) return decompress<F>(s, a, is_inf);
  uint32_t any = 0;
  for (int k = 0; k < 2 * W; k++) any |= s[k];
  is_inf = any == 0;
  if (is_inf) return ST_OK;
  const int ps = pairing::point_status<F>(s, false, a);  // 1 a coordinate >= p, 2 not on the curve
  return ps == 1 ? ST_RANGE : ps == 2 ? ST_NO_POINT : ST_OK;
}

}  // namespace keyfile
