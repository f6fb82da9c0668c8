// TEST-ONLY: the host-callable pieces of the Groth16 setup (city-rollup_amd/csrc/fixed_base.h: the signed byte digits of the
// fixed-base multiplication; groth16_setup.h: the transposition of a CSR matrix) built for the CPU, so that the exact code the
// library runs is checked against Python integers without a GPU. Never loaded by the product path.
#include "../../city-rollup_amd/csrc/fixed_base.h"
#include "../../city-rollup_amd/csrc/groth16_setup.h"

extern "C" {
int ss_windows(void) { return fixedbase::WINDOWS; }
int ss_window_bits(void) { return fixedbase::WINDOW_BITS; }
int ss_half(void) { return fixedbase::HALF; }
int ss_results_per_lane(void) { return fixedbase::K; }
// digits[w], w < ss_windows(), of the 256-bit scalar k (4 little-endian u64)
void ss_recode(const uint64_t *k, int32_t *digits) {
  int d[fixedbase::WINDOWS];
  fixedbase::recode((const uint8_t *)k, d);
  for (int w = 0; w < fixedbase::WINDOWS; w++) digits[w] = d[w];
}
// the transpose of an n_rows x n_cols CSR matrix into caller-allocated arrays (n_cols + 1, nnz, nnz)
void ss_transpose(const uint64_t *row_ptr, const uint32_t *col, const uint32_t *coeff, size_t n_rows, size_t n_cols, uint64_t *out_row_ptr,
                  uint32_t *out_col, uint32_t *out_coeff) {
  g16setup::Csr t;
  g16setup::transpose_csr(row_ptr, col, coeff, n_rows, n_cols, t);
  for (size_t i = 0; i <= n_cols; i++) out_row_ptr[i] = t.row_ptr[i];
  for (size_t i = 0; i < t.col.size(); i++) { out_col[i] = t.col[i]; out_coeff[i] = t.coeff[i]; }
}
}
