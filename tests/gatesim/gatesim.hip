// TEST-ONLY: the gate constraint polynomials of the product (city-rollup_amd/csrc/gates.h) built for the CPU in both of their
// instantiations, F = canonical u64 (what the quotient kernels instantiate) and F = gl::Ext (what the host side of cp_verify
// instantiates), so that tests/test_gate_semantics.py can hold every wire of every gate against the per-row definition in
// tests/gate_semantics.py without a GPU. Never loaded by the product path.
// A gate crosses as its seven ints {type, selector_index, group_start, group_end, param, param2, param3}. Rows are
// [n_rows][num_wires] values, constants [n_rows][num_consts], out [n_rows][count]; for the extension build a value is the word
// pair (c0, c1). Every function returns the number of constraints the gate EMITTED (-1 if it emitted an index twice or out of
// range), which the test holds against gs_num_constraints.
#include "../../city-rollup_amd/csrc/gates.h"

namespace {
gates::Gate gate_of(const int *g) { return {g[0], g[1], g[2], g[3], g[4], g[5], g[6]}; }
constexpr int MAX_CONSTRAINTS = 512;

template <class F>
int eval_rows(const int *gi, const F *consts, int num_consts, const F *wires, int num_wires, const F *pi, size_t n_rows, F *out) {
  const gates::Gate g = gate_of(gi);
  const int count = gates::num_constraints(g);
  if (count < 0 || count > MAX_CONSTRAINTS) return -1;
  int emitted = 0;
  for (size_t r = 0; r < n_rows; r++) {
    const F *w = wires + r * (size_t)num_wires, *c = consts + r * (size_t)num_consts;
    F *o = out + r * (size_t)count;
    bool seen[MAX_CONSTRAINTS] = {};
    bool bad = false;
    int n = 0;
    gates::eval<F>(
        g, [&](int j) { return w[j]; }, [&](int j) { return c[j]; }, [&](int j) { return pi[j]; },
        [&](int k, F v) {
          if (k < 0 || k >= count || seen[k]) { bad = true; return; }
          seen[k] = true;
          o[k] = v;
          n++;
        });
    if (bad) return -1;
    if (r == 0) emitted = n;
    else if (n != emitted) return -1;
  }
  return n_rows ? emitted : count;
}
}  // namespace

extern "C" {
int gs_num_constraints(const int *g) { return gates::num_constraints(gate_of(g)); }
int gs_num_wires(const int *g) { return gates::num_wires(gate_of(g)); }
int gs_num_constants(const int *g) { return gates::num_constants(gate_of(g)); }
int gs_eval_base(const int *g, const uint64_t *consts, int num_consts, const uint64_t *wires, int num_wires, const uint64_t *pi,
                 size_t n_rows, uint64_t *out) {
  return eval_rows<uint64_t>(g, consts, num_consts, wires, num_wires, pi, n_rows, out);
}
int gs_eval_ext(const int *g, const uint64_t *consts, int num_consts, const uint64_t *wires, int num_wires, const uint64_t *pi,
                size_t n_rows, uint64_t *out) {
  static_assert(sizeof(gl::Ext) == 16, "an extension value crosses as two words");
  return eval_rows<gl::Ext>(g, (const gl::Ext *)consts, num_consts, (const gl::Ext *)wires, num_wires, (const gl::Ext *)pi, n_rows,
                            (gl::Ext *)out);
}
}
