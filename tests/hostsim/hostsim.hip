// TEST-ONLY: host-side instantiation of the __host__ __device__ arithmetic in city-rollup_amd/csrc
// so that the exact device formulas (lazy reductions, limb MDS, shift twiddles) can be unit-tested and
// run under sanitizers on the CPU. Never loaded by the product path. What each entry computes on one element is in
// sim_gl.h / sim_bls.h, shared with the device twin of this library (tests/devsim): every arithmetic `hs_<name>` here has a
// `ds_<name>` there (tests/test_devsim_ledger.py).
#include "sim_gl.h"

extern "C" {
void hs_poseidon_permute(uint64_t *states, size_t n) {
  for (size_t i = 0; i < n; i++) sim::permute(states + 12 * i, 0);
}
void hs_poseidon_permute_textbook(uint64_t *states, size_t n) {
  for (size_t i = 0; i < n; i++) sim::permute(states + 12 * i, 4);
}
// double-precision layers (poseidon.h): carry normalisation of a two-limb value; one plane through T / K / T^-1'
void hs_renorm_d(const double *in, double *out) { sim::renorm(1, in, out); }
// 0: dom_enter_d, 1: dom_mul_d<false>, 2: dom_mul_d<true>, 3: dom_leave_d; 4 .. 7: see sim::dom_d (op 6 reads a thirteenth input)
void hs_dom_d(int op, const double *s, double *y) { sim::dom_d(op, s, y); }
uint64_t hs_recombine_d(double l, double h, uint64_t c) {  // c: the constant already minus B (1 + 2^32), as the tables hold it
  return sim::recombine_const(l, h, c);
}
void hs_mds_layer(uint64_t *s, int which) { sim::mds_layer(s, which); }  // 0: integer planes, 1: double-precision planes; no constant
uint64_t hs_mul(uint64_t a, uint64_t b) { return sim::gl_op2(0, a, b); }
uint64_t hs_mul_lazy(uint64_t a, uint64_t b) { return sim::gl_op2(1, a, b); }
uint64_t hs_add(uint64_t a, uint64_t b) { return sim::gl_op2(2, a, b); }
uint64_t hs_sub(uint64_t a, uint64_t b) { return sim::gl_op2(3, a, b); }
uint64_t hs_gl_op1(int op, uint64_t a) { return sim::gl_op1(op, a); }
uint64_t hs_gl_op2(int op, uint64_t a, uint64_t b) { return sim::gl_op2(op, a, b); }
uint64_t hs_mul_add_lazy(uint64_t a, uint64_t b, uint64_t c) { return gl::mul_add_lazy(a, b, c); }
uint64_t hs_fold_top(uint64_t lo, uint32_t top) { return gl::fold_top(lo, top); }
// form 0: (lo, hi); form 1: (lo, hi', cy), given as the true high half hi = hi' + cy 2^32 and cy
uint64_t hs_reduce128_lazy(int form, uint64_t lo, uint64_t hi, uint32_t cy) { return sim::reduce128_lazy(form, lo, hi, cy, 0); }
void hs_ext_mul(const uint64_t *a, const uint64_t *b, uint64_t *out) { sim::ext_mul(a, b, out); }
void hs_gl_chain(int which, uint64_t a, uint64_t b, uint64_t c, uint64_t *out) { sim::gl_chain(which, a, b, c, out); }
// which rare paths a * b takes in reduce128_lazy / fold_top (tests/rare_paths.py restates this with Python integers):
// bit 0 = the borrow of `lo - w3`, bit 1 = the wrap of `+ w2 (2^32 - 1)`, bit 2 = the lazy result is >= p (canon matters)
int hs_mul_paths(uint64_t a, uint64_t b) { return sim::mul_paths(a, b); }
// `permute_until` composed from the same layers, WITHOUT the final canon: the lazy state the device canonicalises on its way out
void hs_poseidon_permute_lazy(uint64_t *states, size_t n) {
  for (size_t i = 0; i < n; i++) sim::permute(states + 12 * i, 5);
}
void hs_mds_limb(const uint32_t *s, uint32_t *y) { sim::mds_limb(s, y); }
uint64_t hs_mul_pow2(uint64_t x, int k) { return sim::mul_pow2(x, k); }  // 0 <= k < 192 (2^96 == -1)
void hs_round16(uint64_t *x, int inverse) { sim::round16(x, inverse); }
// ext3.h on the host: op 0 = mul, 1 = inverse through adjugate_row / norm, 2 = mulx, 3 = adjugate_row and norm (out: 4 words)
void hs_cubic(int op, const uint64_t *m, const uint64_t *a, const uint64_t *b, uint64_t *out) {
  uint64_t r[4] = {0, 0, 0, 0};
  sim::cubic(op, m, a, b, r);
  for (int i = 0; i < (op == 3 ? 4 : 3); i++) out[i] = r[i];
}
}

// ---- BLS12-381 (csrc/bls12_381.h, bls12_381_fr.h) and the one-limb product of r1cs.h ----
#include "sim_bls.h"
extern "C" {
void hs_bls_fp_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) { sim::bls_fp_op(op, a, b, out); }
void hs_bls_fp2_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) { sim::bls_fp2_op(op, a, b, out); }
int hs_bls_g1_chain(const uint32_t *xy, size_t n, uint32_t *out_xy) { return sim::bucket_chain<bls::Fp>(xy, n, out_xy); }
int hs_bls_g2_chain(const uint32_t *xy, size_t n, uint32_t *out_xy) { return sim::bucket_chain<bls::Fp2>(xy, n, out_xy); }
void hs_bls_lz_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) { sim::bls_lz_op(op, a, b, out); }
int hs_bls_lz_maybe_zero(const uint32_t *a) { return sim::bls_lz_maybe_zero(a); }
int hs_bls_g1_loose_step(const uint32_t *acc, const uint32_t *q_xy, uint32_t *out) { return sim::loose_step<bls::Fp>(acc, q_xy, out); }
int hs_bls_g2_loose_step(const uint32_t *acc, const uint32_t *q_xy, uint32_t *out) { return sim::loose_step<bls::Fp2>(acc, q_xy, out); }
int hs_bls_g1_loose_out(const uint32_t *acc, uint32_t *out_xy) { return sim::loose_out<bls::Fp>(acc, out_xy); }
int hs_bls_g2_loose_out(const uint32_t *acc, uint32_t *out_xy) { return sim::loose_out<bls::Fp2>(acc, out_xy); }
void hs_bls_fp_raw(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) { sim::bls_fp_raw(op, a, b, out); }
int hs_bls_lz_k(int weak, int K, const uint32_t *a, const uint32_t *b, uint32_t *out) { return sim::bls_lz_k(weak, K, a, b, out); }
int hs_bls_g1_op(int op, const uint32_t *p_xy, int p_inf, const uint32_t *q_xy, int q_inf, uint32_t k, uint32_t *out_xy) {
  return sim::group_op<bls::Fp>(op, p_xy, p_inf, q_xy, q_inf, k, out_xy);
}
int hs_bls_g2_op(int op, const uint32_t *p_xy, int p_inf, const uint32_t *q_xy, int q_inf, uint32_t k, uint32_t *out_xy) {
  return sim::group_op<bls::Fp2>(op, p_xy, p_inf, q_xy, q_inf, k, out_xy);
}
void hs_bls_fr_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) { sim::bls_fr_op(op, a, b, out); }
void hs_bls_fr_raw(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) { sim::bls_fr_raw(op, a, b, out); }
void hs_r1cs_mul_small(const uint32_t *w, uint32_t c, uint32_t *out) { sim::r1cs_mul_small(w, c, out); }
}

// ---- host_util.h: worker threads that cannot take the process down ----
#include "../../city-rollup_amd/csrc/host_util.h"
extern "C" {
// runs parallel_for over n indices on max_threads threads with the `fail_after`-th thread creation failing
// (-1: none); out[p] += p + 1 for every index done; returns the number of indices whose body ran
long hs_parallel_for(size_t n, size_t max_threads, long fail_after, uint64_t *out) {
  hostu::fault_counter(0).store(fail_after);
  std::atomic<long> ran{0};
  hostu::parallel_for(n, max_threads, [&](size_t p) { out[p] += p + 1; ran++; });
  hostu::fault_counter(0).store(-1);
  return ran.load();
}
// body that throws std::bad_alloc at index `bad`: returns 1 when the exception reached the caller after all helpers
// were joined, 0 when nothing was thrown
int hs_parallel_for_throw(size_t n, size_t max_threads, size_t bad) {
  try {
    hostu::parallel_for(n, max_threads, [&](size_t p) { if (p == bad) throw std::bad_alloc(); });
  } catch (const std::bad_alloc &) {
    return 1;
  }
  return 0;
}

// ---- dev_pool.h (the batch-handle buffer pool) over a counting allocator with a capacity: a script of operations in, the
// allocator's and the pool's counters out. op: 0 alloc(device, bytes) -> handle index, 1 release(handle, reusable),
// 2 trim(device), 3 malloc(device, bytes) -> handle index (the path every other allocation of the library takes)
}  // extern "C"
#include "../../city-rollup_amd/csrc/dev_pool.h"
#include <set>
namespace poolsim {
struct Fake {
  static constexpr int OOM = 2;
  static inline size_t capacity = 0, in_use = 0, n_malloc = 0, n_free = 0, n_oom = 0;
  static inline std::map<void *, size_t> live;
  static inline uintptr_t next = 0x1000;
  static int malloc(void **p, size_t bytes) {
    if (in_use + bytes > capacity) { n_oom++; return OOM; }
    *p = (void *)next;
    next += 0x1000;
    live[*p] = bytes;
    in_use += bytes;
    n_malloc++;
    return 0;
  }
  static void free(void *p) {
    auto it = live.find(p);
    if (it == live.end()) { n_free = (size_t)-1; return; }  // double free / foreign pointer: poison the counter
    in_use -= it->second;
    live.erase(it);
    n_free++;
  }
};
}  // namespace poolsim
extern "C" {
// ops: n x {op, device, bytes_or_handle, reusable}; results: n x int64 (handle index, -OOM, or bytes trimmed);
// counters_out: {in_use, n_malloc, n_free, n_oom, live buffers, pooled bytes dev0, pooled bytes dev1, hits0, misses0, trims0}
int hs_pool_script(size_t n_devices, size_t pool_cap, size_t capacity, const int64_t *ops, size_t n, int64_t *results, uint64_t *counters_out) {
  using poolsim::Fake;
  Fake::capacity = capacity; Fake::in_use = 0; Fake::n_malloc = Fake::n_free = Fake::n_oom = 0; Fake::live.clear();
  DevPoolT<Fake> pool(n_devices, pool_cap);
  struct H { void *p; size_t bytes; int device; };
  std::vector<H> handles;
  std::set<void *> out;  // buffers currently handed out: a pool must never hand one out twice
  for (size_t i = 0; i < n; i++) {
    const int64_t op = ops[4 * i], dev = ops[4 * i + 1], arg = ops[4 * i + 2], reusable = ops[4 * i + 3];
    if (op == 0 || op == 3) {
      void *p = nullptr;
      const int e = op == 0 ? pool.alloc((int)dev, &p, (size_t)arg) : pool.malloc((int)dev, &p, (size_t)arg);
      if (e) { results[i] = -e; continue; }
      if (!out.insert(p).second) return -1;
      handles.push_back({p, (size_t)arg, (int)dev});
      results[i] = (int64_t)handles.size() - 1;
    } else if (op == 1) {
      H &h = handles[(size_t)arg];
      out.erase(h.p);
      pool.release(h.device, h.p, h.bytes, reusable != 0);
      results[i] = 0;
    } else {
      results[i] = (int64_t)pool.trim((int)dev);
    }
  }
  counters_out[0] = Fake::in_use; counters_out[1] = Fake::n_malloc; counters_out[2] = Fake::n_free; counters_out[3] = Fake::n_oom;
  counters_out[4] = Fake::live.size();
  counters_out[5] = pool.stats(0).bytes; counters_out[6] = pool.stats(1).bytes;
  counters_out[7] = pool.stats(0).hits; counters_out[8] = pool.stats(0).misses; counters_out[9] = pool.stats(0).trims;
  return 0;
}
}

// ---- dev_mem.h: the owners over the same counting allocator. ops: n x {op, a, b, c}:
//  0 new(slot a, pooled b, with the idle callback c)   1 alloc(slot a, bytes b) -> 0 / -OOM   2 grow(slot a, bytes b) -> 0 / -OOM
//  3 reset(slot a)   4 move(slot a -> slot b)   5 the idle callback answers a from now on   6 mark_idle(slot a)   7 mark_exported(slot a)
//  8 release(slot a): the caller takes the pointer (and frees it through the runtime)   9 bag(pooled a, b allocations of c bytes, callback
//  always) -> how many succeeded before the first refusal; the bag dies with the op   10 size(slot a) -> bytes, -1 if pointer and size disagree
// Every owner dies before the counters are read: the pool script's ten, then how often the idle callback was asked.
#include "../../city-rollup_amd/csrc/dev_mem.h"
extern "C" {
int hs_mem_script(size_t pool_cap, size_t capacity, const int64_t *ops, size_t n, int64_t *results, uint64_t *counters_out) {
  using poolsim::Fake;
  using Pool = DevPoolT<Fake>;
  Fake::capacity = capacity; Fake::in_use = 0; Fake::n_malloc = Fake::n_free = Fake::n_oom = 0; Fake::live.clear();
  Pool pool(1, pool_cap);
  bool answer = true;
  uint64_t asked = 0;
  const auto idle = [&] { asked++; return answer; };
  {
    std::vector<DevBufT<Pool>> slots(8);
    for (size_t i = 0; i < n; i++) {
      const int64_t op = ops[4 * i], a = ops[4 * i + 1], b = ops[4 * i + 2], c = ops[4 * i + 3];
      results[i] = 0;
      if (op != 5 && op != 9 && (a < 0 || a >= 8)) return -1;
      if (op == 0) slots[a] = c ? DevBufT<Pool>(pool, 0, b ? DevOwn::POOLED : DevOwn::RUNTIME, idle) : DevBufT<Pool>(pool, 0, b ? DevOwn::POOLED : DevOwn::RUNTIME);
      else if (op == 1) results[i] = -slots[a].alloc((size_t)b);
      else if (op == 2) results[i] = -slots[a].grow((size_t)b);
      else if (op == 3) slots[a].reset();
      else if (op == 4) { if (b < 0 || b >= 8) return -1; slots[b] = std::move(slots[a]); }
      else if (op == 5) answer = a != 0;
      else if (op == 6) slots[a].mark_idle();
      else if (op == 7) slots[a].mark_exported();
      else if (op == 8) { void *p = slots[a].release(); if (p) Pool::free(p); }
      else if (op == 9) {
        DevBagT<Pool> bag(pool, 0, a ? DevOwn::POOLED : DevOwn::RUNTIME, idle);
        for (int64_t k = 0; k < b; k++) {
          char *q;
          if (bag.alloc(&q, (size_t)c)) { if (q) return -2; break; }
          results[i]++;
        }
        if ((int64_t)bag.size() != results[i]) return -2;
      } else if (op == 10) results[i] = ((bool)slots[a] == (slots[a].bytes() != 0)) ? (int64_t)slots[a].bytes() : -1;
    }
  }
  counters_out[0] = Fake::in_use; counters_out[1] = Fake::n_malloc; counters_out[2] = Fake::n_free; counters_out[3] = Fake::n_oom;
  counters_out[4] = Fake::live.size();
  counters_out[5] = pool.stats(0).bytes; counters_out[6] = pool.stats(1).bytes;
  counters_out[7] = pool.stats(0).hits; counters_out[8] = pool.stats(0).misses; counters_out[9] = pool.stats(0).trims;
  counters_out[10] = asked;
  pool.trim(0);  // what the pool still parks goes back too: after this nothing may be live
  return Fake::live.empty() && Fake::n_free != (size_t)-1 ? 0 : -3;
}
}

// ---- air.h: the host half (analyse + compile) and the instruction semantics the device interpreter shares (run_segment),
// executed on one row / point with plain arrays behind the memory interface ----
#include <cstdio>
#include <cstring>
#include "../../city-rollup_amd/csrc/air.h"
#include "../../city-rollup_amd/csrc/ext3.h"
namespace airsim {
struct HostMem {
  static constexpr int K = 1;
  std::vector<uint64_t> slots;
  const uint64_t *u, *loc, *nxt;
  uint64_t *out;
  const uint64_t *prog, *al;
  uint64_t code(uint32_t pc) const { return prog[pc]; }
  uint64_t alpha(int c) const { return al[c]; }
  air::Vec<1> slot_read(uint32_t i) const { return {{slots[i]}}; }
  void slot_write(uint32_t i, const air::Vec<1> &v) { slots[i] = v.v[0]; }
  uint64_t uni(uint32_t i) const { return u[i]; }
  air::Vec<1> local(uint32_t i) const { return {{loc[i]}}; }
  air::Vec<1> next(uint32_t i) const { return {{nxt[i]}}; }
  void store(uint32_t col, const air::Vec<1> &v) { out[col] = v.v[0]; }
};
}  // namespace airsim
extern "C" {
// dims: n_columns, n_public, n_global, n_challenge, n_out_columns. Returns 0, or -1 with the analyser's message in err (256 bytes).
// acc_out[c] = sum over segments of (the segment's Horner sum) * alpha_c^(sinks after it) - what k_run + k_finish add up before the
// division by Z_H; stores_out: the stored columns of a map program; info_out: segments, slots, instructions, live ops, max degree
int hs_air_point(int kind, const uint32_t *ops, size_t n_ops, const uint64_t *consts, size_t n_consts, const uint32_t *dims, uint32_t want_segments, int prefetch,
                 const uint64_t *local, const uint64_t *next, const uint64_t *publics, const uint64_t *globals, const uint64_t *challenges,
                 const uint64_t *alphas, int n_alphas, const uint64_t *sel, uint64_t *acc_out, uint64_t *stores_out, uint32_t *info_out, char *err) {
  air::Program P;
  P.kind = kind;
  P.ops.resize(n_ops);
  if (n_ops) memcpy(P.ops.data(), ops, n_ops * 16);
  P.consts.assign(consts, consts + n_consts);
  P.n_columns = dims[0]; P.n_public = dims[1]; P.n_global = dims[2]; P.n_challenge = dims[3]; P.n_out_columns = dims[4];
  const std::string why = air::analyse(P);
  if (!why.empty()) { snprintf(err, 256, "%s", why.c_str()); return -1; }
  const air::Compiled C = air::compile(P, want_segments, prefetch != 0);
  std::vector<uint64_t> uni(P.consts);
  uni.insert(uni.end(), publics, publics + P.n_public);
  uni.insert(uni.end(), globals, globals + P.n_global);
  uni.insert(uni.end(), challenges, challenges + P.n_challenge);
  uni.push_back(0);
  airsim::HostMem m{std::vector<uint64_t>(C.n_slots ? C.n_slots : 1, 0xDEADBEEFull), uni.data(), local, next, stores_out, C.code.data(), alphas};
  const air::Selectors<1> S{{{sel[0]}}, {{sel[1]}}, {{sel[2]}}};
  for (int c = 0; c < n_alphas; c++) acc_out[c] = 0;
  for (uint32_t s = 0; s < C.n_segments(); s++) {
    air::Vec<1> acc[air::MAX_ALPHAS];
    std::fill(m.slots.begin(), m.slots.end(), 0xDEADBEEFull);  // a segment must not read what another one left
    air::run_segment(C.seg_off[s], C.seg_off[s + 1], m, kind == 0 ? n_alphas : 0, S, acc);
    for (int c = 0; c < n_alphas; c++) acc_out[c] = gl::add(acc_out[c], gl::mul(acc[c].v[0], gl::pow(alphas[c], C.sinks_after[s])));
  }
  info_out[0] = C.n_segments(); info_out[1] = C.n_slots; info_out[2] = (uint32_t)C.code.size(); info_out[3] = (uint32_t)P.n_live; info_out[4] = P.max_degree;
  return 0;
}
// air::map_self_read of a map program (dims as above) whose input columns start at byte address `in` and output columns at `out`, n rows:
// 1 and the first pair (cols_out[0] = the loaded input column, cols_out[1] = the stored output column), 0 = none, -1 = malformed program
int hs_air_map_self_read(const uint32_t *ops, size_t n_ops, const uint32_t *dims, uint64_t in, uint64_t out, uint64_t n, uint32_t *cols_out, char *err) {
  air::Program P;
  P.kind = 1;
  P.ops.resize(n_ops);
  if (n_ops) memcpy(P.ops.data(), ops, n_ops * 16);
  P.n_columns = dims[0]; P.n_public = dims[1]; P.n_global = dims[2]; P.n_challenge = dims[3]; P.n_out_columns = dims[4];
  const std::string why = air::analyse(P);
  if (!why.empty()) { snprintf(err, 256, "%s", why.c_str()); return -1; }
  return air::map_self_read(P, in, out, n, &cols_out[0], &cols_out[1]) ? 1 : 0;
}
}
