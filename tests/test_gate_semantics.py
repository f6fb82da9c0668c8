"""The 22 plonky2 gate types, every wire, against what a gate MEANS (tests/gate_semantics.py), on the CPU.

Three statements of the gates are evaluated row by row: the oracle's (or_gate_row_constraints) and csrc/gates.h in both of its
instantiations, uint64_t and gl::Ext (tests/gatesim, a host build with the product's flags). For every gate, over the 200 random
rows of synth_gates' generators, every edge row, every malicious row and every corruption of gate_semantics:
  - the constraint vector is all zero exactly when the definition names no violation, in all three;
  - the three vectors are equal word for word, and have num_constraints values;
  - no wire at or above the gate's wire count changes any value;
  - on 20 rows of genuine extension values (c1 != 0) the gl::Ext instantiation equals the oracle.
Every list length is a literal below, so a case cannot drop out silently, and the number of corruptions the definition ACCEPTS is
a literal with its reason, so nothing passes by accepting everything."""
import ctypes
import json
import os

import numpy as np
import pytest

import gate_semantics as S
import oracle_lib as O
import synth_gates as SG
from synth_circuit import poseidon_gate_row

P = S.P
W = S.NUM_WIRES
HERE = os.path.dirname(os.path.abspath(__file__))

# ---- the literals ----
# wires of each gate (sum = 1963: every one of them is corrupted at least once), constraints of each gate
NUM_WIRES = {S.NOOP: 0, S.CONSTANT: 2, S.PUBLIC_INPUT: 4, S.ARITHMETIC: 80, S.POSEIDON: 135, S.COMPARISON: 87, S.U32_ARITHMETIC: 114,
             S.U32_RANGE_CHECK: 119, S.U32_ADD_MANY: 120, S.U32_SUBTRACTION: 126, S.U32_INTERLEAVE: 102, S.UNINTERLEAVE_TO_U32: 134,
             S.UNINTERLEAVE_TO_B32: 134, S.ARITHMETIC_EXT: 80, S.MUL_EXT: 78, S.BASE_SUM: 64, S.RANDOM_ACCESS: 90, S.REDUCING: 133,
             S.REDUCING_EXT: 132, S.POSEIDON_MDS: 48, S.COSET_INTERPOLATION: 47, S.EXPONENTIATION: 134}
NUM_CONSTRAINTS = {S.NOOP: 0, S.CONSTANT: 2, S.PUBLIC_INPUT: 4, S.ARITHMETIC: 20, S.POSEIDON: 123, S.COMPARISON: 88,
                   S.U32_ARITHMETIC: 108, S.U32_RANGE_CHECK: 119, S.U32_ADD_MANY: 105, S.U32_SUBTRACTION: 114, S.U32_INTERLEAVE: 102,
                   S.UNINTERLEAVE_TO_U32: 134, S.UNINTERLEAVE_TO_B32: 134, S.ARITHMETIC_EXT: 20, S.MUL_EXT: 26, S.BASE_SUM: 64,
                   S.RANDOM_ACCESS: 26, S.REDUCING: 86, S.REDUCING_EXT: 64, S.POSEIDON_MDS: 24, S.COSET_INTERPOLATION: 12,
                   S.EXPONENTIATION: 67}
# ranged wires (limbs, bits, chunks): each gets two more corruptions
NUM_RANGED = {S.POSEIDON: 1,            # swap
              S.COMPARISON: 35,         # 2 x 16 chunks, 3 diff bits
              S.U32_ARITHMETIC: 96,     # 3 ops x 32 limbs
              S.U32_RANGE_CHECK: 112,   # 7 inputs x 16 limbs
              S.U32_ADD_MANY: 90,       # 5 ops x 18 limbs
              S.U32_SUBTRACTION: 102,   # 6 ops x (16 limbs + output_borrow)
              S.U32_INTERLEAVE: 96, S.UNINTERLEAVE_TO_U32: 128, S.UNINTERLEAVE_TO_B32: 128,   # bits
              S.BASE_SUM: 63, S.RANDOM_ACCESS: 16, S.EXPONENTIATION: 66}
# corruptions per gate = wires + 2 * ranged + 1 beyond the gate (Poseidon fills all 135 wires: none beyond)
NUM_CORRUPTIONS = {S.NOOP: 1, S.CONSTANT: 3, S.PUBLIC_INPUT: 5, S.ARITHMETIC: 81, S.POSEIDON: 137, S.COMPARISON: 158,
                   S.U32_ARITHMETIC: 307, S.U32_RANGE_CHECK: 344, S.U32_ADD_MANY: 301, S.U32_SUBTRACTION: 331, S.U32_INTERLEAVE: 295,
                   S.UNINTERLEAVE_TO_U32: 391, S.UNINTERLEAVE_TO_B32: 391, S.ARITHMETIC_EXT: 81, S.MUL_EXT: 79, S.BASE_SUM: 191,
                   S.RANDOM_ACCESS: 123, S.REDUCING: 134, S.REDUCING_EXT: 133, S.POSEIDON_MDS: 49, S.COSET_INTERPOLATION: 48,
                   S.EXPONENTIATION: 267}
# corruptions of the typical row that the definition accepts. Every gate but Poseidon: the wire AT its wire count belongs to no
# condition of the gate (1). Beyond that:
#   RandomAccess: 4 copies x 15 items the index does not select are free (60);
#   Comparison: the typical operands differ in chunks 6 and 7 only, and the equality_dummy of an EQUAL chunk is free: it is the
#     witness of the difference's inverse, and there is no difference (14).
NUM_ACCEPTED = {t: 1 for t in NUM_WIRES}
NUM_ACCEPTED.update({S.POSEIDON: 0, S.RANDOM_ACCESS: 61, S.COMPARISON: 15})
NUM_EDGES = {S.NOOP: 1, S.CONSTANT: 2, S.PUBLIC_INPUT: 2, S.ARITHMETIC: 4, S.POSEIDON: 5, S.COMPARISON: 10, S.U32_ARITHMETIC: 8,
             S.U32_RANGE_CHECK: 7, S.U32_ADD_MANY: 5, S.U32_SUBTRACTION: 9, S.U32_INTERLEAVE: 5, S.UNINTERLEAVE_TO_U32: 9,
             S.UNINTERLEAVE_TO_B32: 9, S.ARITHMETIC_EXT: 4, S.MUL_EXT: 4, S.BASE_SUM: 4, S.RANDOM_ACCESS: 4, S.REDUCING: 6,
             S.REDUCING_EXT: 6, S.POSEIDON_MDS: 4, S.COSET_INTERPOLATION: 7, S.EXPONENTIATION: 9}
NUM_MALICIOUS = {S.NOOP: 0, S.CONSTANT: 1, S.PUBLIC_INPUT: 1, S.ARITHMETIC: 1, S.POSEIDON: 3, S.COMPARISON: 4, S.U32_ARITHMETIC: 6,
                 S.U32_RANGE_CHECK: 2, S.U32_ADD_MANY: 2, S.U32_SUBTRACTION: 2, S.U32_INTERLEAVE: 1, S.UNINTERLEAVE_TO_U32: 1,
                 S.UNINTERLEAVE_TO_B32: 1, S.ARITHMETIC_EXT: 1, S.MUL_EXT: 1, S.BASE_SUM: 2, S.RANDOM_ACCESS: 2, S.REDUCING: 1,
                 S.REDUCING_EXT: 1, S.POSEIDON_MDS: 1, S.COSET_INTERPOLATION: 1, S.EXPONENTIATION: 1}
NUM_RANDOM = 200

GATE_IDS = [S.NAME[g[0]] for g in S.ALL_GATES]


# ---- the evaluators ----
class GateSim:
    def __init__(self):
        import simlibs
        self.L = ctypes.CDLL(simlibs.build("gatesim"))
        for name in ("gs_num_constraints", "gs_num_wires", "gs_num_constants", "gs_eval_base", "gs_eval_ext"):
            getattr(self.L, name).restype = ctypes.c_int

    @staticmethod
    def _gate(gate):
        return (ctypes.c_int * 7)(gate[0], 0, 0, 1, gate[1], gate[2], gate[3])

    def counts(self, gate):
        g = self._gate(gate)
        return self.L.gs_num_constraints(g), self.L.gs_num_wires(g), self.L.gs_num_constants(g)

    def eval(self, gate, consts, wires, pi, ext):
        """base: consts [n][k], wires [n][W], pi [4] -> [n][count]; ext: the same with a last axis of 2"""
        consts, wires, pi = O.arr(consts), O.arr(wires), O.arr(pi)
        n = wires.shape[0]
        out = np.zeros((n, 512) + ((2,) if ext else ()), np.uint64)
        f = self.L.gs_eval_ext if ext else self.L.gs_eval_base
        cnt = f(self._gate(gate), O.ptr(consts), ctypes.c_int(consts.shape[1]), O.ptr(wires), ctypes.c_int(wires.shape[1]), O.ptr(pi),
                ctypes.c_size_t(n), O.ptr(out))
        assert 0 <= cnt <= 512, cnt
        per = cnt * (2 if ext else 1)
        return out.reshape(-1)[:n * per].reshape((n, cnt) + ((2,) if ext else ())).copy()


@pytest.fixture(scope="module")
def sim():
    return GateSim()


def embed(a):
    return np.stack([O.arr(a), np.zeros_like(O.arr(a))], axis=-1)


def three_vectors(sim, gate, consts, wires, pi):
    """the constraint values of n base-field rows from the oracle, gates.h<uint64_t> and gates.h<gl::Ext>: [3][n][count]"""
    consts, wires, pi = O.arr(consts), O.arr(wires), O.arr(pi)
    orc = O.gate_row_constraints(gate, embed(consts), embed(wires), embed(pi))
    ext = sim.eval(gate, embed(consts), embed(wires), embed(pi), True)
    base = sim.eval(gate, consts, wires, pi, False)
    assert not orc[..., 1].any() and not ext[..., 1].any(), "base-field rows give base-field constraint values"
    return np.stack([orc[..., 0], base, ext[..., 0]])


# ---- the rows ----
def random_rows(gate):
    """200 satisfying rows from synth_gates' own generators (uniform operands), with their constants and hash"""
    rng = np.random.default_rng(4000 + gate[0])
    pi = [int(v) for v in rng.integers(0, P, 4, dtype=np.uint64)]
    rows, consts = [], []
    for _ in range(NUM_RANDOM):
        k0, k1 = (int(v) for v in rng.integers(0, P, 2, dtype=np.uint64))
        full = [int(v) for v in rng.integers(0, P, W, dtype=np.uint64)]
        if gate[0] == S.POSEIDON:
            row = poseidon_gate_row(full[:12], int(rng.integers(0, 2)))
        else:
            row = SG.gate_row(rng, gate, k0, k1, pi) or []
        full[:len(row)] = [int(v) for v in row]
        rows.append(full)
        consts.append((k0, k1))
    return rows, consts, pi


def all_rows(gate):
    """[(kind, name, consts, pi_hash, full row)] in a fixed order: random, edge, malicious, typical, corruptions"""
    out = []
    rows, consts, pi = random_rows(gate)
    out += [("random", str(i), consts[i], pi, rows[i]) for i in range(len(rows))]
    for name, o in S.edge_operands(gate):
        out.append(("edge", name, S.consts_of(gate, o), S.pi_hash_of(gate, o), S.full_row(gate, S.honest_row(gate, o))))
    for name, k, ph, row in S.malicious_rows(gate):
        out.append(("malicious", name, k, ph, S.full_row(gate, row)))
    typ = S.typical_operands(gate)
    row = S.honest_row(gate, typ)
    full = S.full_row(gate, row)
    out.append(("typical", "", S.consts_of(gate, typ), S.pi_hash_of(gate, typ), full))
    for cor in S.corruptions(gate, row):
        out.append(("corruption", cor, S.consts_of(gate, typ), S.pi_hash_of(gate, typ), S.apply_corruption(gate, full, cor)))
    return out


def by_pi(rows):
    """the evaluators take one public-inputs hash per call: group the row indices by hash"""
    groups = {}
    for i, r in enumerate(rows):
        groups.setdefault(tuple(r[3]), []).append(i)
    return groups


# ---- the definition against itself and the data it rests on ----
def test_the_gate_list_is_synth_gates():
    assert S.ALL_GATES == SG.ALL_GATES and len(S.ALL_GATES) == 22
    for g in S.ALL_GATES:
        names = S.wire_names(g)  # asserts the layout is a partition
        assert len(names) == NUM_WIRES[g[0]] == SG.gate_num_wires(g), S.NAME[g[0]]
        assert len(S.ranged_wires(g)) == NUM_RANGED.get(g[0], 0), S.NAME[g[0]]
        assert len({j for j, _ in S.ranged_wires(g)}) == NUM_RANGED.get(g[0], 0)
    assert sum(NUM_WIRES.values()) == 1963
    assert sum(NUM_CORRUPTIONS.values()) == 1963 + 2 * sum(NUM_RANGED.values()) + 21 == 3850


def test_the_python_permutation_is_the_pinned_one():
    """tests/golden/poseidon_zero_hashes.json pins the permutation (and so the round constants): zero hash i+1 is
    two_to_one(zero hash i, zero hash i) = the first four lanes of the permutation of (l, r, 0, 0, 0, 0)."""
    z = json.load(open(os.path.join(HERE, "golden", "poseidon_zero_hashes.json")))["two_to_one"]
    for i in range(4):
        assert S.poseidon_permutation(z[i] + z[i] + [0] * 4)[:4] == z[i + 1]
    st = S.det(9, 12)
    assert S.poseidon_permutation(st) == [int(v) for v in O.permute(O.arr(st))]
    assert S.round_constants() == __import__("synth_circuit")._rc()


def test_honest_rows_mean_what_they_say():
    """spot checks of honest_row against the plain meaning, beyond the assertions inside it"""
    row = S.honest_row(S.GATE[S.U32_ARITHMETIC], {"ops": [(S.U32_MAX,) * 3, (0, 0, 0), (3, 5, 7)]})
    assert row[3:6] == [0, S.U32_MAX, 0] and (S.U32_MAX ** 2 + S.U32_MAX) == P - 1     # lo = 0, hi = 2^32-1, no inverse
    assert row[9:12] == [0, 0, pow(S.U32_MAX, P - 2, P)] and row[15:17] == [22, 0]
    row = S.honest_row(S.GATE[S.U32_SUBTRACTION], {"ops": [(0, S.U32_MAX, 1), (5, 5, 1), (5, 5, 0), (9, 4, 0), (0, 0, 0), (1, 0, 1)]})
    assert row[3:5] == [0, 1] and row[8:10] == [S.U32_MAX, 1] and row[13:15] == [0, 0] and row[18:20] == [5, 0]
    row = S.honest_row(S.GATE[S.U32_INTERLEAVE], {"values": [0b1011, 1 << 31, 0]})
    assert row[1] == 0b1000101 and row[3] == 1 << 62 and row[6:6 + 32] == [0] * 28 + [1, 0, 1, 1]
    for t, (ev, od) in ((S.UNINTERLEAVE_TO_U32, (0b10, 0b11)), (S.UNINTERLEAVE_TO_B32, (0b100, 0b101))):
        row = S.honest_row(S.GATE[t], {"values": [0b1101, P - 1]})    # bits 3..0 = 1 1 0 1: wire 60 = 1, 61 = 1, 62 = 0, 63 = 1
        assert row[0:3] == [0b1101, ev, od], (t, row[0:3])
    row = S.honest_row(S.GATE[S.COMPARISON], {"first": 7, "second": 7 + (1 << 30)})
    assert row[2] == 1 and row[3] == 1 and row[4 + 80:] == [1, 0, 1]
    row = S.honest_row(S.GATE[S.RANDOM_ACCESS], {"copies": [(i, list(range(100 * i, 100 * i + 16))) for i in (0, 15, 5, 10)]})
    assert [row[18 * i + 1] for i in range(4)] == [0, 1515, 505, 1010] and row[74:] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 0, 0, 1, 0, 1]


def test_list_lengths_are_the_literals():
    for g in S.ALL_GATES:
        t = g[0]
        row = S.honest_row(g, S.typical_operands(g))
        cors = S.corruptions(g, row)
        assert len(cors) == NUM_CORRUPTIONS[t] == NUM_WIRES[t] + 2 * NUM_RANGED.get(t, 0) + (NUM_WIRES[t] < W), S.NAME[t]
        assert {c[0] for c in cors if c[2] == "+1"} == set(range(NUM_WIRES[t])), "every wire gets its +1"
        assert len(S.edge_operands(g)) == NUM_EDGES[t], S.NAME[t]
        assert len(S.malicious_rows(g)) == NUM_MALICIOUS[t], S.NAME[t]


def free_wires_of_the_typical_row(gate):
    """the named free classes, as wire indices, from the typical operands alone"""
    t, a, b, c = gate
    L = S.layout(gate)
    free = set()
    if NUM_WIRES[t] < W:
        free.add(NUM_WIRES[t])                       # beyond the gate
    if t == S.RANDOM_ACCESS:
        for cp, (idx, _) in enumerate(S.typical_operands(gate)["copies"]):
            free |= {L["list_item"][cp][i] for i in range(1 << a) if i != idx}   # items the index does not select
    if t == S.COMPARISON:
        o = S.typical_operands(gate)
        free |= {L["equality_dummy"][i] for i in range(b) if (o["first"] >> (2 * i)) & 3 == (o["second"] >> (2 * i)) & 3}
    return free


def test_accepted_corruptions_are_the_named_free_classes():
    """From the definition alone: the accepted corruptions are the +1 (or beyond-the-gate) ones of the named free wires, nothing
    else; every other wire's +1, every out-of-range value and every other in-range value is refused. Malicious rows are all refused,
    edge rows all accepted."""
    for g in S.ALL_GATES:
        typ = S.typical_operands(g)
        k, ph = S.consts_of(g, typ), S.pi_hash_of(g, typ)
        row = S.honest_row(g, typ)
        full = S.full_row(g, row)
        assert S.violations(g, k, full, ph) == []
        accepted = [c for c in S.corruptions(g, row) if not S.violations(g, k, S.apply_corruption(g, full, c), ph)]
        assert len(accepted) == NUM_ACCEPTED[g[0]], S.NAME[g[0]]
        assert {c[0] for c in accepted} == free_wires_of_the_typical_row(g) and len({c[0] for c in accepted}) == len(accepted)
        assert all(c[2] in ("+1", "beyond the gate") for c in accepted)
        for name, o in S.edge_operands(g):
            assert S.violations(g, S.consts_of(g, o), S.full_row(g, S.honest_row(g, o)), S.pi_hash_of(g, o)) == [], (S.NAME[g[0]], name)
        for name, kk, pp, r in S.malicious_rows(g):
            assert S.violations(g, kk, S.full_row(g, r), pp), (S.NAME[g[0]], name)
    assert sum(NUM_ACCEPTED.values()) == 21 + 60 + 14


def test_named_free_wires_of_edge_rows():
    """the accepted corruptions the issue names that only an edge row shows"""
    g = S.GATE[S.EXPONENTIATION]
    o = dict(S.edge_operands(g))["all bits 0"]
    full = S.full_row(g, S.honest_row(g, o))
    full[0] = (full[0] + 1) % P     # the base under all-zero bits multiplies nothing
    assert S.violations(g, S.DEFAULT_CONSTS, full, S.DEFAULT_PI_HASH) == []
    g = S.GATE[S.U32_ARITHMETIC]
    full = S.full_row(g, S.honest_row(g, {"ops": [(0, 0, 0)] * 3}))
    full[5] = 12345                 # lo = 0: the inverse witnesses nothing
    assert S.violations(g, S.DEFAULT_CONSTS, full, S.DEFAULT_PI_HASH) == []
    g = S.GATE[S.NOOP]
    assert all(S.violations(g, S.DEFAULT_CONSTS, S.det(i, W), S.DEFAULT_PI_HASH) == [] for i in range(3))


# ---- the three statements against the definition ----
@pytest.mark.parametrize("gate", S.ALL_GATES, ids=GATE_IDS)
def test_constraints_vanish_exactly_when_the_definition_holds(sim, gate):
    t = gate[0]
    assert sim.counts(gate) == (NUM_CONSTRAINTS[t], NUM_WIRES[t], {S.CONSTANT: 2, S.ARITHMETIC: 2, S.ARITHMETIC_EXT: 2, S.MUL_EXT: 1,
                                                                   S.RANDOM_ACCESS: 2}.get(t, 0))
    rows = all_rows(gate)
    assert len(rows) == NUM_RANDOM + NUM_EDGES[t] + NUM_MALICIOUS[t] + 1 + NUM_CORRUPTIONS[t]
    verdicts = [S.violations(gate, r[2], r[4], r[3]) for r in rows]
    tail = S.det(77, W)
    seen_accept = seen_refuse = 0
    for ph, idx in by_pi(rows).items():
        consts = [rows[i][2] for i in idx]
        wires = [rows[i][4] for i in idx]
        vec = three_vectors(sim, gate, consts, wires, ph)
        assert vec.shape == (3, len(idx), NUM_CONSTRAINTS[t]), "the number of constraints is num_constraints"
        assert (vec[0] == vec[1]).all() and (vec[0] == vec[2]).all(), "oracle, gates.h<u64> and gates.h<Ext> differ"
        for n, i in enumerate(idx):
            zero = not vec[0][n].any()
            assert zero == (verdicts[i] == []), (S.NAME[t], rows[i][0], rows[i][1], verdicts[i][:3], np.nonzero(vec[0][n])[0][:5])
            seen_accept += zero
            seen_refuse += not zero
        # wires at or above the gate's wire count change no value (the corruption "beyond the gate" is one of the rows, too)
        moved = [w[:NUM_WIRES[t]] + tail[NUM_WIRES[t]:] for w in wires]
        assert (three_vectors(sim, gate, consts, moved, ph) == vec).all()
    kinds = [r[0] for r in rows]
    assert seen_accept == NUM_RANDOM + NUM_EDGES[t] + 1 + NUM_ACCEPTED[t]
    assert seen_refuse == NUM_MALICIOUS[t] + NUM_CORRUPTIONS[t] - NUM_ACCEPTED[t]
    assert kinds.count("corruption") == NUM_CORRUPTIONS[t]


@pytest.mark.parametrize("gate", S.ALL_GATES, ids=GATE_IDS)
def test_extension_instantiation_equals_the_oracle_on_extension_values(sim, gate):
    """20 rows with genuine F_p^2 values in every wire, constant and hash element (c1 != 0): the verifier's side of gates.h. Ten are
    uniform; ten are an honest row plus X times a uniform row, so that the values stay near the gate's zero set."""
    t = gate[0]
    rng = np.random.default_rng(6000 + t)
    rows, consts, _ = random_rows(gate)
    wires = rng.integers(1, P, (20, W, 2), dtype=np.uint64)
    ks = rng.integers(1, P, (20, 2, 2), dtype=np.uint64)
    for i in range(10):
        wires[i, :, 0] = O.arr(rows[i])
        ks[i, :, 0] = O.arr(consts[i])
    pi = rng.integers(1, P, (4, 2), dtype=np.uint64)
    assert wires[..., 1].all() and ks[..., 1].all() and pi[..., 1].all()
    want = O.gate_row_constraints(gate, ks, wires, pi)
    got = sim.eval(gate, ks, wires, pi, True)
    assert want.shape == got.shape == (20, NUM_CONSTRAINTS[t], 2)
    assert (want == got).all()
    if NUM_CONSTRAINTS[t]:
        assert want[..., 1].any(), "the rows never left the base field"
