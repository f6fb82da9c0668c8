// TEST-ONLY: the device twin of tests/hostsim/hostsim.hip and tests/renorm_hostsim/renorm_hostsim.hip for gl.h, poseidon.h, ntt16.h
// and ext3.h: every `hs_<name>` has a `ds_<name>` here that applies the same element-wise body (../hostsim/sim_gl.h) to arrays on
// the device, under a per-element mask (devsim.h). Built with the product's own flags, so the primitives are the `GL_DEVICE_ASM`
// forms the library gets. Arguments: the ones of the `hs_*` entry as arrays of n elements, then mask, then n; the return value is
// the hipError_t. Never loaded by the product path.
#include "devsim.h"
#include "../hostsim/sim_gl.h"

namespace devsim {
int unit_init() {
  static int err = -1;
  if (err != -1) return err;
  if ((err = hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_RC), POSEIDON_RC, sizeof POSEIDON_RC))) return err;
  if ((err = hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_RCD), POSEIDON_RCD, sizeof POSEIDON_RCD))) return err;
  if ((err = hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_DDK), poseidon::DDK_HOST, sizeof poseidon::DDK_HOST))) return err;
  return err = hipMemcpyToSymbol(HIP_SYMBOL(poseidon::d_DDLAST), poseidon::DDLAST_HOST, sizeof poseidon::DDLAST_HOST);
}
}  // namespace devsim
using devsim::Job;
typedef const uint8_t *mask_t;

static int gl2(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *da = j.in(a, n), *db = j.in(b, n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = sim::gl_op2(op, da[i], db[i]); });
}
// one kernel per form (FORM is a constant inside it: the other forms fold away), as every kernel of the product holds one
template <int FORM>
static int permute_one(uint64_t *states, size_t n, mask_t mask) {
  Job j(mask, n);
  uint64_t *s = j.inout(states, 12 * n);
  return j.run(DS_EACH { sim::permute(s + 12 * i, FORM); });
}
static int permute_form(uint64_t *states, size_t n, int form, mask_t mask) {
  switch (form) {
    case 0: return permute_one<0>(states, n, mask);
    case 1: return permute_one<1>(states, n, mask);
    case 2: return permute_one<2>(states, n, mask);
    case 3: return permute_one<3>(states, n, mask);
    case 4: return permute_one<4>(states, n, mask);
    default: return permute_one<5>(states, n, mask);
  }
}

extern "C" {
// ---- gl.h ----
int ds_mul(const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) { return gl2(0, a, b, out, mask, n); }
int ds_mul_lazy(const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) { return gl2(1, a, b, out, mask, n); }
int ds_add(const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) { return gl2(2, a, b, out, mask, n); }
int ds_sub(const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) { return gl2(3, a, b, out, mask, n); }
int ds_gl_op2(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) { return gl2(op, a, b, out, mask, n); }
int ds_gl_op1(int op, const uint64_t *a, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *da = j.in(a, n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = sim::gl_op1(op, da[i]); });
}
int ds_mul_add_lazy(const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *da = j.in(a, n), *db = j.in(b, n), *dc = j.in(c, n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = gl::mul_add_lazy(da[i], db[i], dc[i]); });
}
int ds_fold_top(const uint64_t *lo, const uint32_t *top, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *dl = j.in(lo, n);
  const uint32_t *dt = j.in(top, n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = gl::fold_top(dl[i], dt[i]); });
}
// form 1: the carries of the active lanes of a wave are gathered into the lane mask that `mul_wide_cy` would have left
int ds_reduce128_lazy(int form, const uint64_t *lo, const uint64_t *hi, const uint32_t *cy, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *dl = j.in(lo, n), *dh = j.in(hi, n);
  const uint32_t *dc = j.in(cy, n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH {
    const uint64_t lanes = form ? __ballot(dc[i] != 0) : 0;
    o[i] = sim::reduce128_lazy(form, dl[i], dh[i], dc[i], lanes);
  });
}
int ds_mul_paths(const uint64_t *a, const uint64_t *b, int *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *da = j.in(a, n), *db = j.in(b, n);
  int *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = sim::mul_paths(da[i], db[i]); });
}
int ds_ext_mul(const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *da = j.in(a, 2 * n), *db = j.in(b, 2 * n);
  uint64_t *o = j.inout(out, 2 * n);
  return j.run(DS_EACH { sim::ext_mul(da + 2 * i, db + 2 * i, o + 2 * i); });
}
// out: n x 3
int ds_gl_chain(int which, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *da = j.in(a, n), *db = j.in(b, n), *dc = j.in(c, n);
  uint64_t *o = j.inout(out, 3 * n);
  if (which == 0) return j.run(DS_EACH { sim::gl_chain(0, da[i], db[i], dc[i], o + 3 * i); });
  return j.run(DS_EACH { sim::gl_chain(1, da[i], db[i], dc[i], o + 3 * i); });
}

// ---- ntt16.h ----
int ds_mul_pow2(const uint64_t *x, const int *k, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *dx = j.in(x, n);
  const int *dk = j.in(k, n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = sim::mul_pow2(dx[i], dk[i]); });
}
// x: n x 16 in place
int ds_round16(uint64_t *x, int inverse, mask_t mask, size_t n) {
  Job j(mask, n);
  uint64_t *d = j.inout(x, 16 * n);
  if (inverse) return j.run(DS_EACH { sim::round16(d + 16 * i, 1); });
  return j.run(DS_EACH { sim::round16(d + 16 * i, 0); });
}

// ---- poseidon.h ----
int ds_poseidon_permute(uint64_t *states, size_t n, mask_t mask) { return permute_form(states, n, 0, mask); }
int ds_poseidon_permute_textbook(uint64_t *states, size_t n, mask_t mask) { return permute_form(states, n, 4, mask); }
int ds_poseidon_permute_lazy(uint64_t *states, size_t n, mask_t mask) { return permute_form(states, n, 5, mask); }
// form: 0 permute, 1 permute_absorb, 2 permute_squeeze, 3 permute_node, 4 permute_textbook; -1 (not a hipError_t) for any other
int ds_rn_permute(uint64_t *states, size_t n, int form, mask_t mask) {
  if (form < 0 || form > 4) return -1;
  return permute_form(states, n, form, mask);
}
// the whole permutation on every element (any u64 words in)
int ds_permute(uint64_t *states, size_t n, int form) {
  const std::vector<uint8_t> all(n ? n : 1, 1);
  return ds_rn_permute(states, n, form, all.data());
}
static int renorm(int which, const double *in, double *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const double *di = j.in(in, 2 * n);
  double *o = j.inout(out, 2 * n);
  return j.run(DS_EACH { sim::renorm(which, di + 2 * i, o + 2 * i); });
}
int ds_renorm_d(const double *in, double *out, mask_t mask, size_t n) { return renorm(1, in, out, mask, n); }
int ds_rn_renorm(int which, const double *in, double *out, mask_t mask, size_t n) { return renorm(which, in, out, mask, n); }
// s: n x 13, y: n x 12
int ds_dom_d(int op, const double *s, double *y, mask_t mask, size_t n) {
  Job j(mask, n);
  const double *ds = j.in(s, 13 * n);
  double *o = j.inout(y, 12 * n);
  return j.run(DS_EACH { sim::dom_d(op, ds + 13 * i, o + 12 * i); });
}
int ds_recombine_d(const double *l, const double *h, const uint64_t *c, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const double *dl = j.in(l, n), *dh = j.in(h, n);
  const uint64_t *dc = j.in(c, n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = sim::recombine_const(dl[i], dh[i], dc[i]); });
}
// table, idx per element as in hs_rn_recombine; the table entries are looked up here and travel as bit patterns. -1 for an index
// outside its table
int ds_rn_recombine(const double *l, const double *h, const int *table, const int *idx, uint64_t *out, mask_t mask, size_t n) {
  std::vector<uint64_t> m(2 * n + 2);
  for (size_t i = 0; i < n; i++) {
    const int t = table[i], k = idx[i];
    if (t < 0 || t > 3 || k < 0 || k >= ((t & 1) ? poseidon::W : poseidon::PARTIAL)) return -1;
    const uint64_t *tab = t == 0 ? POSEIDON_DOMD_K : t == 1 ? POSEIDON_DOMD_LAST : t == 2 ? POSEIDON_DOMD32_K : POSEIDON_DOMD32_LAST;
    m[2 * i] = tab[2 * k], m[2 * i + 1] = tab[2 * k + 1];
  }
  Job j(mask, n);
  const double *dl = j.in(l, n), *dh = j.in(h, n);
  const uint64_t *dm = j.in(m.data(), 2 * n);
  uint64_t *o = j.inout(out, n);
  return j.run(DS_EACH { o[i] = sim::recombine_bits(dl[i], dh[i], dm[2 * i], dm[2 * i + 1]); });
}
// s: n x 12 in place
int ds_mds_layer(uint64_t *s, int which, mask_t mask, size_t n) {
  Job j(mask, n);
  uint64_t *d = j.inout(s, 12 * n);
  if (which) return j.run(DS_EACH { sim::mds_layer(d + 12 * i, 1); });
  return j.run(DS_EACH { sim::mds_layer(d + 12 * i, 0); });
}
int ds_mds_limb(const uint32_t *s, uint32_t *y, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint32_t *ds = j.in(s, 12 * n);
  uint32_t *o = j.inout(y, 12 * n);
  return j.run(DS_EACH { sim::mds_limb(ds + 12 * i, o + 12 * i); });
}

// ---- ext3.h ----
// m: n x 2, a, b: n x 3, out: n x 4
int ds_cubic(int op, const uint64_t *m, const uint64_t *a, const uint64_t *b, uint64_t *out, mask_t mask, size_t n) {
  Job j(mask, n);
  const uint64_t *dm = j.in(m, 2 * n), *da = j.in(a, 3 * n), *db = j.in(b, 3 * n);
  uint64_t *o = j.inout(out, 4 * n);
  return j.run(DS_EACH { sim::cubic(op, dm + 2 * i, da + 3 * i, db + 3 * i, o + 4 * i); });
}
}
