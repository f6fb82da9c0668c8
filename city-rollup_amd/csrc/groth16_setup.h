// The F_r side of the Groth16 setup (host side: groth16_setup.inc): the two element-wise kernels that
// turn the QAP columns u, v, w at tau into the logarithms of the key's points, and the host transposition that makes the QAP
// columns a job for the R1CS kernels (A^T L is r1cs_eval of the transposed system with the Lagrange values as its witness).
#pragma once
#include <vector>

#include "r1cs.h"

namespace g16setup {

using blsfr::Fr;

struct Csr {
  std::vector<uint64_t> row_ptr;
  std::vector<uint32_t> col, coeff;
};
// The transpose of a validated CSR matrix of n_rows x n_cols: a counting sort of the terms by column, O(terms). Row i of the
// result holds the terms of column i in the order of the rows they came from; a wire named twice in a row is two terms.
inline void transpose_csr(const uint64_t *row_ptr, const uint32_t *col, const uint32_t *coeff, size_t n_rows, size_t n_cols, Csr &out) {
  const size_t nnz = row_ptr[n_rows];
  out.row_ptr.assign(n_cols + 1, 0);
  for (size_t t = 0; t < nnz; t++) out.row_ptr[(size_t)col[t] + 1]++;
  for (size_t i = 0; i < n_cols; i++) out.row_ptr[i + 1] += out.row_ptr[i];
  out.col.resize(nnz);
  out.coeff.resize(nnz);
  std::vector<uint64_t> next(out.row_ptr.begin(), out.row_ptr.end() - 1);
  for (size_t j = 0; j < n_rows; j++)
    for (size_t t = row_ptr[j]; t < row_ptr[j + 1]; t++) {
      const uint64_t pos = next[col[t]]++;
      out.col[pos] = (uint32_t)j;
      out.coeff[pos] = coeff[t];
    }
}

// out[j] = scale * base^j for j < count, canonical (base, scale in Montgomery form): the powers of tau the Lagrange values are
// the inverse transform of (scale = 1), and the logarithms tau^j (tau^n - 1) / delta of the Z set
__global__ void k_scaled_powers(Fr base, Fr scale, size_t count, uint32_t *__restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  blsfr::fr_to_canonical(blsfr::fr_mul(blsfr::fr_pow_u64(base, j), scale), out + 8 * j);
}

// out[i] = (beta u_i + alpha v_i + w_i) / gamma for the public wires i < n_public, / delta for the private ones: the logarithms
// of the IC and the K points. Canonical in and out; the four constants in Montgomery form, so every product is canonical again
// (r1cs.h). first_zero_private (initialised to ~0): the lowest private wire whose value is zero - the K set has no infinity flags.
__global__ void k_key_scalars(const uint32_t *__restrict__ u, const uint32_t *__restrict__ v, const uint32_t *__restrict__ w, Fr beta, Fr alpha,
                              Fr gamma_inv, Fr delta_inv, size_t n_public, size_t n_wires, uint32_t *__restrict__ out,
                              unsigned long long *__restrict__ first_zero_private) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_wires) return;
  Fr s = blsfr::fr_add(blsfr::fr_mul(beta, r1cs::load_canonical(u, i)), blsfr::fr_mul(alpha, r1cs::load_canonical(v, i)));
  s = blsfr::fr_add(s, r1cs::load_canonical(w, i));
  s = blsfr::fr_mul(i < n_public ? gamma_inv : delta_inv, s);
  r1cs::store_canonical(out, i, s);
  uint32_t any = 0;
  for (int l = 0; l < blsfr::NL; l++) any |= s.l[l];
  if (i >= n_public && any == 0) atomicMin(first_zero_private, (unsigned long long)i);
}

}  // namespace g16setup
