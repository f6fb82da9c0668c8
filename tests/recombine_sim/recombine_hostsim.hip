// TEST-ONLY: host instantiation of `recombine_s` / `repair_s`, of the b block in the basis of the partial rounds, and of the
// permutation forms with a count of the rare repairs. Built twice by recombine_sim_build.py: as the product compiles it, and with
// -DPOSEIDON_RECOMBINE_V1 -DPOSEIDON_BBLOCK_DENSE (the forms kept for the A/B). Never loaded by the product path.
#include "recombine_sim.h"

using namespace poseidon;

extern "C" {
// bit 0 SMALL_TOP, bit 1 B_TRI, bit 2 UNITS32
int rs_flags() { return (SMALL_TOP ? 1 : 0) | (B_TRI ? 2 : 0) | (UNITS32 ? 4 : 0); }
// the literals and tables as the header holds them. table: 0 POSEIDON_RCS (361 entries, literal FULL), 1 POSEIDON_DOMS_K (22, PARTIAL),
// 2 POSEIDON_DOMS_LAST (12, PARTIAL), 3 POSEIDON_DOMS32_K (22, PARTIAL32), 4 POSEIDON_DOMS32_LAST (12, PARTIAL32)
uint32_t rs_top0(int table) { return table == 0 ? POSEIDON_TOP0_FULL : table <= 2 ? POSEIDON_TOP0_PARTIAL : POSEIDON_TOP0_PARTIAL32; }
// one recombination with entry i of a table, limbs in the table's unit. *wrap: whether the fold wrapped (the repair is applied)
uint64_t rs_recombine(int table, int i, double l, double h, int *wrap) {
  const uint64_t *t = table == 0 ? POSEIDON_RCS : table == 1 ? POSEIDON_DOMS_K : table == 2 ? POSEIDON_DOMS_LAST : table == 3 ? POSEIDON_DOMS32_K : POSEIDON_DOMS32_LAST;
  const Magic m{__builtin_bit_cast(double, t[2 * i]), __builtin_bit_cast(double, t[2 * i + 1])};
  uint64_t w = 0, r;
  if (table == 0) r = recombine_s<POSEIDON_TOP0_FULL>(l, h, m, w);
  else if (table <= 2) r = recombine_s<POSEIDON_TOP0_PARTIAL>(l, h, m, w);
  else r = recombine_s<POSEIDON_TOP0_PARTIAL32>(l, h, m, w);
  *wrap = (int)w;
  return gl::fold_repair(r, w);
}
// the top word alone (before the fold), for the bounds: hi32(a1) + carry - T0 as `recombine_s` forms it
uint32_t rs_top(int table, int i, double l, double h) {
  const uint64_t *t = table == 0 ? POSEIDON_RCS : table == 1 ? POSEIDON_DOMS_K : table == 2 ? POSEIDON_DOMS_LAST : table == 3 ? POSEIDON_DOMS32_K : POSEIDON_DOMS32_LAST;
  const uint64_t a0 = __builtin_bit_cast(uint64_t, l + __builtin_bit_cast(double, t[2 * i])), a1 = __builtin_bit_cast(uint64_t, h + __builtin_bit_cast(double, t[2 * i + 1]));
  uint32_t w1;
  const uint32_t carry = __builtin_add_overflow(gl::hi32(a0), gl::lo32(a1), &w1);
  return gl::hi32(a1) + carry - rs_top0(table);
}
// n elements of one site (rsim::recombine_site): l, h n x 12 (site 1 reads [0] of each row), out n x 12
void rs_site(int site, int idx, const double *l, const double *h, uint64_t *out, size_t n) {
  for (size_t i = 0; i < n; i++) rsim::recombine_site(site, idx, l + 12 * i, h + 12 * i, out + 12 * i);
}
// states: n x 12 in place. form: 0 permute, 1 permute_absorb, 2 permute_squeeze, 3 permute_node, 4 permute_textbook
int rs_permute(uint64_t *states, size_t n, int form) {
  if (form < 0 || form > 4) return -1;
  for (size_t i = 0; i < n; i++) {
    uint64_t s[12];
    for (int k = 0; k < 12; k++) s[k] = states[12 * i + k];
    if (form == 0) permute(s);
    else if (form == 1) permute_absorb(s);
    else if (form == 2) permute_squeeze(s);
    else if (form == 3) permute_node(s);
    else permute_textbook(s);
    for (int k = 0; k < 12; k++) states[12 * i + k] = s[k];
  }
  return 0;
}
// runs of the rare path per site since the last reset
void rs_wrap_runs(unsigned long long *out, int reset) {
  for (int k = 0; k < 3; k++) {
    out[k] = rsim::wrap_runs[k];
    if (reset) rsim::wrap_runs[k] = 0;
  }
}
// the matrices of the b block: 0 K (dense basis), 1 K^2, 2 T K T^-1, 3 its square, 4 T, 5 T^-1 (36 doubles, row-major);
// 6 the b part of l K and 7 of K t in the basis compiled (6 doubles), 8 the square compiled (36)
int rs_matrix(int which, double *out) {
  const DomMat<6> *m = which == 0 ? &DOM_K_B : which == 1 ? &DOM_K_B2 : which == 2 ? &DOM_K_BT : which == 3 ? &DOM_K_BT2 : which == 4 ? &DOM_B_T : which == 5 ? &DOM_B_TINV : which == 8 ? &DOM_B2 : nullptr;
  if (m) {
    for (int i = 0; i < 36; i++) out[i] = m->a[i / 6][i % 6];
    return 36;
  }
  if (which != 6 && which != 7) return -1;
  for (int i = 0; i < 6; i++) out[i] = which == 6 ? DOM_B_CZ.a[i] : DOM_B_KT.a[i];
  return 6;
}
// one plane (s: 13 doubles, y: 12): 0 dom_mul2_b with d = s[12], 1 dom_next_z_b (y[0]), 2 dom_mul2_d, 3 dom_next_z (y[0]),
// 4 dom_b_to_tri, 5 dom_b_from_tri, 6 dom_read_z (y[0])
void rs_dom(int op, const double *s, double *y) {
  double a[12], b[12];
  for (int i = 0; i < 12; i++) a[i] = s[i], b[i] = 0;
  if (op == 0) dom_mul2_b(a, s[12], b);
  else if (op == 1) b[0] = dom_next_z_b(a);
  else if (op == 2) dom_mul2_d(a, s[12], b);
  else if (op == 3) b[0] = dom_next_z(a);
  else if (op == 6) b[0] = dom_read_z(a);
  else {
    if (op == 4) dom_b_to_tri(a); else dom_b_from_tri(a);
    for (int i = 0; i < 12; i++) b[i] = a[i];
  }
  for (int i = 0; i < 12; i++) y[i] = b[i];
}
// The linear part of one trip of `partial_rounds` on both planes, in the basis compiled (tri 1) or the dense one (tri 0): W (wl, wh:
// products at the top of the trip), the change d1 of element 0 in round i, normalisation, z' = element 0 one layer ahead, the
// squared layer with the change d2. out: wl'' (12), wh'' (12), z'l, z'h
void rs_trip(int tri, const double *wl, const double *wh, const double *d1, const double *d2, double *out) {
  double al[12], ah[12], bl[12], bh[12];
  for (int i = 0; i < 12; i++) al[i] = wl[i], ah[i] = wh[i];
  al[0] = __builtin_fma(d1[0], 0.25, al[0]), ah[0] = __builtin_fma(d1[1], 0.25, ah[0]);
  al[3] = __builtin_fma(d1[0], 0.25, al[3]), ah[3] = __builtin_fma(d1[1], 0.25, ah[3]);
  al[6] = __builtin_fma(d1[0], 0.5, al[6]), ah[6] = __builtin_fma(d1[1], 0.5, ah[6]);
  for (int k = 0; k < 12; k++) renorm_planes_d(al[k], ah[k]);
  out[24] = tri ? dom_next_z_b(al) : dom_next_z(al);
  out[25] = tri ? dom_next_z_b(ah) : dom_next_z(ah);
  if (tri) dom_mul2_b(al, d2[0], bl), dom_mul2_b(ah, d2[1], bh);
  else dom_mul2_d(al, d2[0], bl), dom_mul2_d(ah, d2[1], bh);
  for (int i = 0; i < 12; i++) out[i] = bl[i], out[12 + i] = bh[i];
}
}
