"""Whole-proof instances of the per-row gate definition (tests/gate_semantics.py): one witness of the ALL_GATES circuit per row
under test, shared by test_gate_semantics_proofs.py (CPU oracle) and test_gpu_gate_semantics.py (device).

The circuit is synth_gates.build_gate_set(ALL_GATES, db=6): the real selector grouping (five groups), and copy constraints that
touch only columns beyond each gate's wires, so a gate's row can be overwritten after the build. An instance overwrites the wires
of ONE row (the first row of its gate type, unless it says otherwise) and, for the edge rows that set the gate's constants, the
two constants of that row, which nothing but that row's gate reads. Its verdict is the definition's, computed on the row as it
stands in the witness."""
import numpy as np

import gate_semantics as S
import oracle_lib as O
import synth_gates as SG

P = S.P
DB, SEED = 6, 17   # a seed whose circuit has a Noop row free of copy constraints (GateCircuit asserts what it needs)


class GateCircuit:
    def __init__(self, gate_set=SG.ALL_GATES, db=DB, seed=SEED):
        self.c = c = SG.build_gate_set(gate_set, db=db, seed=seed, arity_bits=(2,))
        self.digest = [7, 1, 7, db]
        self.params = {g[0]: g for g in c["sorted_gates"]}
        self.nsel = c["num_selectors"]
        self.pi_hash = tuple(int(v) for v in O.hash_no_pad(O.arr(c["public_inputs"])))
        copied = {cell for pair in c["copies"] for cell in pair}      # (column, row)
        self.copied = copied
        self.row_of = {}
        for t in self.params:
            nw = S.num_wires(self.params[t])
            rows = [i for i, rt in enumerate(c["row_types"]) if rt == t]
            # the wire AT the gate's wire count is to be corrupted freely: it must not be one end of a copy constraint
            ok = [i for i in rows if (nw, i) not in copied]
            assert ok, ("every row of this gate has a copy constraint at its wire count: pick another seed", S.NAME[t])
            self.row_of[t] = ok[0]
        for (col, row) in copied:   # what build_gate_set promises: copies lie beyond the row's gate
            assert col >= S.num_wires(self.params[c["row_types"][row]])
        self._caps = {}

    @property
    def noop_row(self):
        """a Noop row whose cells no copy constraint touches: it can take any gate's values"""
        return next(i for i, rt in enumerate(self.c["row_types"]) if rt == S.NOOP and not any(r == i for _, r in self.copied))

    def consts_at(self, row, cs=None):
        cs = self.c["cs_values"] if cs is None else cs
        return (int(cs[self.nsel, row]), int(cs[self.nsel + 1, row]))

    def cs_with(self, row, consts):
        """cs_values with the two constants of one row replaced (None: the circuit as built)"""
        if consts is None or tuple(consts) == self.consts_at(row):
            return self.c["cs_values"]
        cs = self.c["cs_values"].copy()
        cs[self.nsel, row], cs[self.nsel + 1, row] = consts
        return cs

    def cap(self, cs):
        key = cs.tobytes()
        if key not in self._caps:
            sh = self.c["shape"]
            k, _ = cs.shape
            cap = np.zeros((1 << sh.cap_height, 4), np.uint64)
            O.lib().or_commit_batch(O.ptr(cs), k, sh.degree_bits, sh.rate_bits, sh.cap_height, None, None, None, O.ptr(cap))
            self._caps[key] = cap
        return self._caps[key]

    def witness(self, inst):
        w = self.c["wires"].copy()
        for row, values in inst["writes"]:
            w[:len(values), row] = np.array(values, dtype=np.uint64)
        for col, row in inst.get("bumps", ()):
            w[col, row] = (int(w[col, row]) + 1) % P
        return w

    def verdict(self, inst):
        """the definition's violations of every row the instance touches, under the gate the SELECTOR of that row names"""
        w = self.witness(inst)
        bad = []
        for row in {r for r, _ in inst["writes"]} | {r for _, r in inst.get("bumps", ())}:
            gate = self.params[self.c["row_types"][row]]
            consts = inst["consts"] if inst["consts"] is not None and row == inst["const_row"] else self.consts_at(row)
            bad += S.violations(gate, consts, [int(v) for v in w[:, row]], self.pi_hash)
        return bad


def _inst(gc, gate, kind, name, values, consts=None, row=None, bumps=()):
    row = gc.row_of[gate[0]] if row is None else row
    return dict(gate=gate[0], kind=kind, name=name, writes=[(row, [int(v) for v in values])], consts=consts, const_row=row,
                bumps=list(bumps))


def semantic_instances(gc, gate, corruptions="all"):
    """The instances of one gate, in a fixed order: the honest typical row; every edge row; every malicious row; corruptions of the
    typical row ("all", "first", or "accepted": the first one the definition accepts, if any). Edge operands that set the
    public-inputs hash itself are left to the row evaluators: a proof's hash is the hash of its public inputs."""
    t = gate[0]
    row = gc.row_of[t]
    k, ph = gc.consts_at(row), gc.pi_hash
    typ = dict(S.typical_operands(gate), consts=k, pi_hash=ph)
    honest = S.honest_row(gate, typ) if t != S.NOOP else []
    out = [_inst(gc, gate, "honest", "typical", honest)]
    for name, o in S.edge_operands(gate):
        if "pi_hash" in o:
            continue
        o = dict(o, pi_hash=ph)
        consts = tuple(o["consts"]) if "consts" in o else None
        o.setdefault("consts", k)
        out.append(_inst(gc, gate, "edge", name, S.honest_row(gate, o), consts=consts))
    for name, _, _, r in S.malicious_rows(gate, k, ph):
        out.append(_inst(gc, gate, "malicious", name, r))
    cors = S.corruptions(gate, honest)
    if corruptions != "all":
        full = [int(v) for v in gc.witness(out[0])[:, row]]
        if corruptions == "accepted":
            cors = [c for c in cors if not S.violations(gate, k, S.apply_corruption(gate, full, c), ph)][:1]
        else:
            cors = cors[:1]
    for col, v, kind in cors:
        if v is None:
            out.append(_inst(gc, gate, "corruption", f"wire {col}: {kind}", honest, bumps=[(col, row)]))
        else:
            r = list(honest)
            r[col] = v
            out.append(_inst(gc, gate, "corruption", f"wire {col}: {kind}", r))
    return out


def cross_gate_instances(gc, gate):
    """An honest row of `gate` on a row whose selector names ANOTHER gate (the next gate type, in ALL_GATES order, that the
    definition says these values violate), and the same values on a Noop row, where no filter is open."""
    t = gate[0]
    if t == S.NOOP:
        return []
    row = gc.row_of[t]
    honest = S.honest_row(gate, dict(S.typical_operands(gate), consts=gc.consts_at(row), pi_hash=gc.pi_hash))
    order = [g for g in S.ALL_GATES if g[0] not in (S.NOOP, t)]
    start = next(i for i, g in enumerate(S.ALL_GATES) if g[0] == t)
    order = order[start % len(order):] + order[:start % len(order)]
    out = []
    for other in order:
        inst = _inst(gc, gate, "other gate's row", f"on the {S.NAME[other[0]]} row", honest, row=gc.row_of[other[0]])
        if any((col, gc.row_of[other[0]]) in gc.copied for col in range(len(honest))):
            continue   # it would be refused by the permutation argument as well: not what this instance is about
        if gc.verdict(inst):
            out.append(inst)
            break
    assert out, S.NAME[t]
    out.append(_inst(gc, gate, "noop row", "on a Noop row", honest, row=gc.noop_row))
    return out
