// Witness checks on the ROWS themselves (host side: check.inc; DESIGN.md sections 1.1 and 1.4): does a plonky2 wire matrix satisfy
// its circuit, does a STARK trace satisfy its AIR - and if not, how many constraints break and which is the first. The provers do
// not ask (a violated witness still has well-defined proof bytes); the verifier only says "vanishing identity" / "quotient
// identity". The semantics are the quotient's own, restricted to the n rows of the trace domain:
//   * plonky2 gates (k_gate<TYPE>, one instantiation per gate type as in quotient.h): lanes run over rows; a row whose selector
//     filter is zero costs the selector load; on a bound row every constraint gates.h emits is tested against zero;
//   * copy constraints (k_cells): the sigma value of a routed cell is decoded to the cell it names - S^n = k_is[c']^n finds the
//     coset among the table in LDS, the exponent follows bit by bit from squarings of S / k_is[c'] - and the two wires compared;
//     the same walk over the columns counts wire values >= p;
//   * AIR sinks (k_air_check): the interpreter of air.h at map-mode positions (natural rows, the next row of n - 1 is 0); a sink
//     is tested against the kind of its row instead of being alpha-folded.
// Reduction: per wave (shuffles), then one 64-bit atomic minimum on a packed key and one atomic add per wave and counter. The
// value of the first violation is evaluated again by one lane after the reduction (k_firsts / k_air_check<1, true>), so a call
// reads its counters back once.
#pragma once
#include "air.h"
#include "gates.h"
#include "gl.h"
#include "poseidon.h"

namespace check {

constexpr int MAX_GATES = 32;  // quot::MAX_GATES
constexpr unsigned THREADS = 256;
constexpr uint64_t UNUSED_SELECTOR = 0xFFFFFFFFull;  // u32::MAX
constexpr unsigned long long NONE = ~0ull;

// counters of one proof. Keys: gate = row << 20 | gate index << 12 | constraint (at most 32 gates of at most 512 constraints);
// cells = row << 16 | column. Every key orders by row first. The count of gate violations is the sum of the per-gate counts.
enum { C_GATE_KEY = 0, C_N_COPY, C_COPY_KEY, C_N_SIGMA, C_SIGMA_KEY, C_N_NONCANON, C_NONCANON_KEY, C_GATE_VALUE, C_COPY_TO_ROW, C_COPY_TO_COL,
       C_COPY_VALUE, C_COPY_TO_VALUE, C_PER_GATE, C_STRIDE = C_PER_GATE + MAX_GATES };
constexpr int GATE_ROW_SHIFT = 20, GATE_INDEX_SHIFT = 12, CELL_ROW_SHIFT = 16;

// count and lowest key of a wave into their counters (every lane of the wave calls this)
__device__ __forceinline__ void wave_report(unsigned long long cnt, unsigned long long key, unsigned long long *count_slot, unsigned long long *key_slot) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off);
    const unsigned long long other = __shfl_down(key, off);
    key = other < key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(count_slot, cnt);
    atomicMin(key_slot, key);
  }
}

// ---- plonky2 gates --------------------------------------------------------------------------------------------------------
struct GateArgs {
  const uint64_t *const *cs;     // per proof: cs_values, (num_constants + num_routed_wires) x n in natural row order
  const uint64_t *wires;         // [proof][W][n]
  size_t wires_stride;
  const uint64_t *pi_hash;       // [proof][4]
  unsigned long long *counters;  // [proof][C_STRIDE]
  size_t n;
  int num_selectors, n_gates;
  gates::Gate gates[MAX_GATES];
};

// the filter of gate gi on a row whose selector value is sv: quot::gate_sum's expression
__device__ __forceinline__ uint64_t gate_filter(const GateArgs &a, int gi, uint64_t sv) {
  const gates::Gate &g = a.gates[gi];
  uint64_t f = 1;
  for (int r = g.group_start; r < g.group_end; r++)
    if (r != gi) f = gl::mul(f, gl::sub((uint64_t)r, sv));
  if (a.num_selectors > 1) f = gl::mul(f, gl::sub(UNUSED_SELECTOR, sv));
  return gl::canon(f);
}

// Unfiltered constraints of one gate on one row, canonical: emit(k, v). PoseidonGate and PoseidonMdsGate take the lazy
// permutation primitives the quotient uses (poseidon.h; anchors canonicalised), every other gate the generic code of gates.h.
template <int TYPE, class WR, class CR, class PR, class EF>
__device__ __forceinline__ void gate_constraints(const gates::Gate &g, WR W, CR C, PR PI, EF emit) {
  if constexpr (TYPE == gates::POSEIDON) {
    int c = 0;
    const uint64_t swap = W(24);
    emit(c++, gl::mul(swap, gl::sub(swap, 1)));
    uint64_t st[poseidon::W];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint64_t l = W(k), r = W(k + 4), d = W(25 + k);
      emit(c++, gl::sub(gl::mul(swap, gl::sub(r, l)), d));
      st[k] = gl::add(l, d);
      st[k + 4] = gl::sub(r, d);
    }
#pragma unroll
    for (int k = 8; k < 12; k++) st[k] = W(k);
#pragma unroll
    for (int k = 0; k < 12; k++) st[k] = poseidon::add_const_lazy(st[k], poseidon::rc(k));
    int rnd = 0;
#pragma unroll 1
    for (int r = 0; r < 4; r++, rnd++) {
      if (r != 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) {
          const uint64_t in = W(29 + 12 * (r - 1) + k);
          emit(c++, gl::sub(gl::canon(st[k]), in));
          st[k] = in;
        }
      }
#pragma unroll
      for (int k = 0; k < 12; k++) st[k] = poseidon::sbox_lazy(st[k]);
      if (r < 3) poseidon::mds_layer_d(st, (rnd + 1) * 12);
    }
    poseidon::partial_rounds(
        st,
        [&](int r, uint64_t x) {
          const uint64_t in = W(65 + r);
          emit(c + r, gl::sub(gl::canon(x), in));
          return in;
        },
        poseidon::NeverStop());
    c += 22;
    rnd += 22;
#pragma unroll 1
    for (int r = 0; r < 4; r++, rnd++) {
#pragma unroll
      for (int k = 0; k < 12; k++) {
        const uint64_t in = W(87 + 12 * r + k);
        emit(c++, gl::sub(gl::canon(st[k]), in));
        st[k] = in;
      }
#pragma unroll
      for (int k = 0; k < 12; k++) st[k] = poseidon::sbox_lazy(st[k]);
      poseidon::mds_layer_d(st, rnd + 1 < poseidon::ROUNDS ? (rnd + 1) * 12 : -1);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) emit(c++, gl::sub(gl::canon(st[k]), W(12 + k)));
  } else if constexpr (TYPE == gates::POSEIDON_MDS) {
    uint64_t sa[12], sb[12];
#pragma unroll
    for (int k = 0; k < 12; k++) {
      sa[k] = W(2 * k);
      sb[k] = W(2 * k + 1);
    }
    poseidon::mds_layer_d(sa, -1);
    poseidon::mds_layer_d(sb, -1);
#pragma unroll
    for (int r = 0; r < 12; r++) {
      emit(2 * r, gl::sub(W(24 + 2 * r), gl::canon(sa[r])));
      emit(2 * r + 1, gl::sub(W(24 + 2 * r + 1), gl::canon(sb[r])));
    }
  } else {
    gates::eval_t<TYPE, uint64_t>(g, W, C, PI, [&](int k, uint64_t v) { emit(k, gl::canon(v)); });
  }
}

// every gate type with constraints (Noop has none)
#define CITY_CHECK_GATE_TYPES(X)                                                                                                          \
  X(CONSTANT) X(PUBLIC_INPUT) X(ARITHMETIC) X(POSEIDON) X(COMPARISON) X(U32_ARITHMETIC) X(U32_RANGE_CHECK) X(U32_ADD_MANY) X(U32_SUBTRACTION) \
  X(U32_INTERLEAVE) X(UNINTERLEAVE_TO_U32) X(UNINTERLEAVE_TO_B32) X(ARITHMETIC_EXT) X(MUL_EXT) X(BASE_SUM) X(RANDOM_ACCESS) X(REDUCING)     \
  X(REDUCING_EXT) X(POSEIDON_MDS) X(COSET_INTERPOLATION) X(EXPONENTIATION)

// gate gi (of type TYPE) on row i of `proof`: emit(k, v) for every constraint, if the gate binds the row. Wires and constants are
// read mod p (k_cells counts the wire values >= p).
template <int TYPE, class EF>
__device__ __forceinline__ void gate_on_row(const GateArgs &a, int gi, size_t i, size_t proof, EF emit) {
  const size_t n = a.n;
  const uint64_t *cs = a.cs[proof] + i;
  const gates::Gate g = a.gates[gi];
  if (gate_filter(a, gi, gl::canon(cs[(size_t)g.selector_index * n])) == 0) return;
  const uint64_t *w = a.wires + proof * a.wires_stride + i;
  const uint64_t *consts = cs + (size_t)a.num_selectors * n;
  const uint64_t *pih = a.pi_hash + 4 * proof;
  gate_constraints<TYPE>(
      g, [&](int j) { return gl::canon(w[(size_t)j * n]); }, [&](int j) { return gl::canon(consts[(size_t)j * n]); }, [&](int j) { return pih[j]; }, emit);
}

// grid = (rows / 256, proofs)
template <int TYPE>
__global__ __launch_bounds__(THREADS) void k_gate(GateArgs a, int gi) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x, proof = blockIdx.y;
  unsigned long long cnt = 0, key = NONE;
  if (i < a.n) {
    int first = 1 << GATE_INDEX_SHIFT;
    gate_on_row<TYPE>(a, gi, i, proof, [&](int k, uint64_t v) {
      if (v != 0) {
        cnt++;
        first = k < first ? k : first;
      }
    });
    if (cnt) key = ((unsigned long long)i << GATE_ROW_SHIFT) | ((unsigned long long)gi << GATE_INDEX_SHIFT) | (unsigned long long)first;
  }
  unsigned long long *ctr = a.counters + proof * C_STRIDE;
  wave_report(cnt, key, &ctr[C_PER_GATE + gi], &ctr[C_GATE_KEY]);
}

// ---- copy constraints and wire values >= p --------------------------------------------------------------------------------
struct CellArgs {
  const uint64_t *const *cs;
  const uint64_t *wires;
  size_t wires_stride;
  const uint64_t *k_is;          // [R]
  const uint64_t *omega_tab;     // power table of omega_n (3 x 2048)
  unsigned long long *counters;
  size_t n;
  int degree_bits, ncst, R, W;
  uint64_t omega_inv_pow2[32];   // omega_n^(-2^b), b < degree_bits
};

__device__ __forceinline__ uint64_t pow_tab(const uint64_t *T, uint64_t e) {
  const uint32_t e0 = (uint32_t)e & 2047, e1 = (uint32_t)(e >> 11) & 2047, e2 = (uint32_t)(e >> 22);
  uint64_t r = T[e0];
  if (e1) r = gl::mul(r, T[2048 + e1]);
  if (e2) r = gl::mul(r, T[4096 + e2]);
  return r;
}
__device__ __forceinline__ uint64_t pow_2k(uint64_t x, int k) {
  for (int s = 0; s < k; s++) x = gl::sqr(x);
  return x;
}
// S (canonical) = k_is[c'] omega^r' -> true and (c', r'), or false when there is no such cell. kn(c) = k_is[c]^n.
template <class KN>
__device__ __forceinline__ bool decode_sigma(const CellArgs &a, uint64_t S, KN kn, int *col, size_t *row) {
  const uint64_t y = pow_2k(S, a.degree_bits);
  int c = 0;
  while (c < a.R && kn(c) != y) c++;
  if (c == a.R || y == 0) return false;
  uint64_t t = gl::mul(S, gl::inv(gl::canon(a.k_is[c])));  // in <omega_n>: t^n = 1
  size_t e = 0;
  for (int b = 0; b < a.degree_bits; b++)
    if (pow_2k(t, a.degree_bits - 1 - b) != 1) {  // -1: bit b of the exponent is set
      e |= (size_t)1 << b;
      t = gl::mul(t, a.omega_inv_pow2[b]);
    }
  *col = c;
  *row = e;
  return true;
}

// grid = (rows / 256, proofs), R * 8 bytes of LDS: a lane walks the columns of its row
__global__ __launch_bounds__(THREADS) void k_cells(CellArgs a) {
  extern __shared__ uint64_t kn[];  // k_is[c]^n
  for (int c = threadIdx.x; c < a.R; c += THREADS) kn[c] = pow_2k(gl::canon(a.k_is[c]), a.degree_bits);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x, proof = blockIdx.y, n = a.n;
  unsigned long long n_copy = 0, n_sigma = 0, n_non = 0, k_copy = NONE, k_sigma = NONE, k_non = NONE;
  if (i < n) {
    const uint64_t *w = a.wires + proof * a.wires_stride, *sig = a.cs[proof] + (size_t)a.ncst * n + i;
    const uint64_t wi = pow_tab(a.omega_tab, i);
    for (int c = 0; c < a.W; c++) {
      const uint64_t raw = w[(size_t)c * n + i];
      const unsigned long long key = ((unsigned long long)i << CELL_ROW_SHIFT) | (unsigned long long)c;
      if (raw >= gl::P) {
        n_non++;
        if (k_non == NONE) k_non = key;
      }
      if (c >= a.R) continue;
      const uint64_t S = gl::canon(sig[(size_t)c * n]);
      if (S == gl::mul(gl::canon(a.k_is[c]), wi)) continue;  // the cell names itself
      int c2;
      size_t r2;
      if (!decode_sigma(a, S, [&](int j) { return kn[j]; }, &c2, &r2)) {
        n_sigma++;
        if (k_sigma == NONE) k_sigma = key;
      } else if (gl::canon(w[(size_t)c2 * n + r2]) != gl::canon(raw)) {
        n_copy++;
        if (k_copy == NONE) k_copy = key;
      }
    }
  }
  unsigned long long *ctr = a.counters + proof * C_STRIDE;
  wave_report(n_copy, k_copy, &ctr[C_N_COPY], &ctr[C_COPY_KEY]);
  wave_report(n_sigma, k_sigma, &ctr[C_N_SIGMA], &ctr[C_SIGMA_KEY]);
  wave_report(n_non, k_non, &ctr[C_N_NONCANON], &ctr[C_NONCANON_KEY]);
}

// After the reduction: the value of the first violated constraint and the two ends of the first broken copy, by one lane each.
// grid = proofs, one wave.
__global__ __launch_bounds__(64) void k_firsts(GateArgs g, CellArgs a) {
  const size_t proof = blockIdx.x;
  unsigned long long *ctr = g.counters + proof * C_STRIDE;
  if (threadIdx.x == 0 && ctr[C_GATE_KEY] != NONE) {
    const unsigned long long key = ctr[C_GATE_KEY];
    const size_t row = (size_t)(key >> GATE_ROW_SHIFT);
    const int gi = (int)(key >> GATE_INDEX_SHIFT) & ((1 << (GATE_ROW_SHIFT - GATE_INDEX_SHIFT)) - 1), want = (int)key & ((1 << GATE_INDEX_SHIFT) - 1);
    uint64_t value = 0;
    auto emit = [&](int k, uint64_t v) {
      if (k == want) value = v;
    };
    switch (g.gates[gi].type) {
#define CITY_CHECK_CASE(T) case gates::T: gate_on_row<gates::T>(g, gi, row, proof, emit); break;
      CITY_CHECK_GATE_TYPES(CITY_CHECK_CASE)
#undef CITY_CHECK_CASE
      default: break;
    }
    ctr[C_GATE_VALUE] = value;
  }
  if (threadIdx.x == 1 && ctr[C_COPY_KEY] != NONE) {
    const unsigned long long key = ctr[C_COPY_KEY];
    const size_t row = (size_t)(key >> CELL_ROW_SHIFT), n = a.n;
    const int c = (int)(key & ((1u << CELL_ROW_SHIFT) - 1));
    const uint64_t *w = a.wires + proof * a.wires_stride;
    const uint64_t S = gl::canon(a.cs[proof][((size_t)a.ncst + c) * n + row]);
    int c2 = 0;
    size_t r2 = 0;
    (void)decode_sigma(a, S, [&](int j) { return pow_2k(gl::canon(a.k_is[j]), a.degree_bits); }, &c2, &r2);  // it decoded in k_cells
    ctr[C_COPY_TO_ROW] = r2;
    ctr[C_COPY_TO_COL] = (unsigned long long)c2;
    ctr[C_COPY_VALUE] = gl::canon(w[(size_t)c * n + row]);
    ctr[C_COPY_TO_VALUE] = gl::canon(w[(size_t)c2 * n + r2]);
  }
}

// ---- AIR sinks on natural rows --------------------------------------------------------------------------------------------
// counters: [A_KEY] = row << 24 | sink (a program has at most 2^24 ops), [A_VALUE], then one count per sink
enum { A_KEY = 0, A_VALUE = 1, A_PER_SINK = 2 };
constexpr int AIR_ROW_SHIFT = 24;

struct AirArgs {
  air::KArgs k;                  // code, seg_off, uni, cols, spill, spill_stride, M = rows, n_lds
  const uint32_t *first_sink;    // [segments + 1]: the number (program order) of the first sink of a segment
  unsigned long long *counters;
  uint32_t n_segments;
};

// does a sink of selector `sel` (0 every row, 1 transition, 2 first row, 3 last row) bind row `pos` of M
__device__ __forceinline__ bool sink_binds(uint32_t sel, size_t pos, size_t M) {
  return sel == 0 || (sel == 1 && pos + 1 != M) || (sel == 2 && pos == 0) || (sel == 3 && pos + 1 == M);
}

// FIRST = false: grid = (row blocks, segments), a lane works on KP rows 64 apart as air::k_run does in map mode; every sink is
// tested on the rows it binds. FIRST = true (one wave, KP = 1, after the reduction): the segment of the first violated sink runs
// again on its row and leaves the sink's value.
template <int KP, bool FIRST>
__global__ __launch_bounds__(air::WAVE) void k_air_check(AirArgs a) {
  extern __shared__ uint64_t lds[];
  using V = air::Vec<KP>;
  const int lane = threadIdx.x;
  const size_t M = a.k.M;
  uint32_t seg = blockIdx.y;
  size_t first_row = 0;
  uint32_t first_sink = 0;
  if (FIRST) {
    const unsigned long long key = a.counters[A_KEY];
    if (key == NONE) return;
    first_row = (size_t)(key >> AIR_ROW_SHIFT);
    first_sink = (uint32_t)key & ((1u << AIR_ROW_SHIFT) - 1);
    seg = 0;
    while (seg + 1 < a.n_segments && air::constant_as(a.first_sink)[seg + 1] <= first_sink) seg++;
  }
  air::DevMem<KP> m{lds, a.k, {}, {}, {}, {}, lane, a.k.uni, a.k.alphas, a.k.cols, a.k.out_cols};
  air::for_k<KP>([&](auto k) {
    const size_t p0 = FIRST ? first_row : ((size_t)blockIdx.x * KP + k) * air::WAVE + lane;
    m.active[k] = p0 < M;
    const size_t pos = m.active[k] ? p0 : M - 1;  // idle lanes shadow the last row (loads stay in bounds)
    m.pos[k] = pos;
    m.npos[k] = pos + 1 == M ? 0 : pos + 1;
    m.gid[k] = FIRST ? (size_t)lane : (((size_t)seg * gridDim.x + blockIdx.x) * KP + k) * air::WAVE + lane;
  });
  unsigned long long key[KP];
  air::for_k<KP>([&](auto k) { key[k] = NONE; });
  uint32_t sink = air::constant_as(a.first_sink)[seg];
  V acc = air::vsplat<KP>(0);
  const uint32_t last = air::constant_as(a.k.seg_off)[seg + 1];
  for (uint32_t pc = air::constant_as(a.k.seg_off)[seg]; pc < last; pc++) {
    const uint64_t w = m.code(pc);
    const uint32_t op = (uint32_t)w & 15, ka = (uint32_t)(w >> 4) & 7, kb = (uint32_t)(w >> 7) & 7, dst = (uint32_t)(w >> 10) & 0x3FFF,
                   ia = (uint32_t)(w >> 24) & 0xFFFFF, ib = (uint32_t)(w >> 44);
    auto fetch = [&](uint32_t kd, uint32_t i) -> V {
      switch (kd) {
        case air::K_ACC: return acc;
        case air::K_SLOT: return m.slot_read(i);
        case air::K_UNI: return air::vsplat<KP>(m.uni(i));
        case air::K_LOCAL: return m.local(i);
        default: return m.next(i);
      }
    };
    if (op == air::I_LOAD) {
      m.slot_write(dst, ka == air::K_NEXT ? m.next(ia) : m.local(ia));
      continue;
    }
    if (op == air::I_STORE) continue;  // a constraint program has none
    const V x = fetch(ka, ia);
    if (op == air::I_SINK) {
      if (FIRST) {
        if (sink == first_sink && lane == 0) a.counters[A_VALUE] = gl::canon(x.v[0]);
      } else {
        unsigned long long bad = 0;
        air::for_k<KP>([&](auto k) {
          const bool b = m.active[k] && sink_binds(dst, m.pos[k], M) && gl::canon(x.v[k]) != 0;
          if (b && key[k] == NONE) key[k] = ((unsigned long long)m.pos[k] << AIR_ROW_SHIFT) | sink;
          bad += (unsigned long long)__popcll(__ballot(b));
        });
        if (bad && lane == 0) atomicAdd(&a.counters[A_PER_SINK + sink], bad);
      }
      sink++;
      continue;
    }
    V r;
    if (op == air::I_INV) r = air::vinv<KP>(x);
    else {
      const V y = fetch(kb, ib);
      r = op == air::I_ADD ? air::vadd<KP>(x, y) : op == air::I_SUB ? air::vsub<KP>(x, y) : air::vmul<KP>(x, y);
    }
    if (dst != air::DST_NONE) m.slot_write(dst, r);
    acc = r;
  }
  if (!FIRST) {
    unsigned long long lowest = NONE;
    air::for_k<KP>([&](auto k) { lowest = key[k] < lowest ? key[k] : lowest; });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long other = __shfl_down(lowest, off);
      lowest = other < lowest ? other : lowest;
    }
    if (lane == 0 && lowest != NONE) atomicMin(&a.counters[A_KEY], lowest);
  }
}

}  // namespace check
