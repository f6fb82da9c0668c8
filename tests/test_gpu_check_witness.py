"""GPU: cp_circuit_check_witness_dev / cp_circuit_check_witness against the per-row gate definition (tests/gate_semantics.py) and
the oracle's row evaluator (O.gate_row_constraints), on the circuits of tests/gate_instances.py.

Every instance of every gate of the ALL_GATES circuit at 2^6 rows (the honest row, every edge row, every malicious row, every
corruption, the honest row under another gate's selector and on a Noop row) goes up once per gate and is checked in calls of at
most 256: zero gate violations exactly where the definition finds none; elsewhere the row, the gate the row's selector names,
the lowest violated constraint with its value, the count, and the per-gate counts. Then the order of the "first" across rows and
gates, independent reports within a batch, the city-common circuit at 2^7 rows, copy constraints against a Python decoding of
sigma, a sigma value that names no cell, a wire equal to p, the host-array entry point, every refusal, and injected allocation
failures (refused allocations that return a status: nothing here faults the device). Every comparison is an equality."""
import ctypes

import numpy as np
import pytest

import gate_instances as GI
import gate_semantics as S
import oracle_lib as O
import synth_gates as SG
from test_gpu_prove_full import cp_shape_of

pytestmark = pytest.mark.gpu

P = S.P
GATE_IDS = [S.NAME[g[0]] for g in S.ALL_GATES]
MAX_CALL = 256
DEVMEM = 3   # CP_FAULT_DEVMEM
NONE_FIELDS = dict(gate_row=-1, gate_index=-1, gate_type=-1, constraint=-1, constraint_value=0, copy_row=-1, copy_column=-1, copy_to_row=-1,
                   copy_to_column=-1, copy_value=0, copy_to_value=0, sigma_row=-1, sigma_column=-1, noncanonical_row=-1, noncanonical_column=-1)


@pytest.fixture(scope="module")
def gc():
    return GI.GateCircuit()


@pytest.fixture(scope="module")
def gc7():
    return GI.GateCircuit(SG.CITY_COMMON, db=7, seed=GI.SEED)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


class Circuits:
    """one cp.Circuit per set of constants (an edge row that sets its gate's constants is checked against a circuit of its own)"""

    def __init__(self, prover, gc):
        self.prover, self.gc, self.by_cs = prover, gc, {}

    def of_cs(self, cs):
        import cityprover as cp
        key = cs.tobytes()
        if key not in self.by_cs:
            c = self.gc.c
            circ = cp.Circuit(self.prover, cp_shape_of(cp, c["shape"]), self.gc.digest, cs)
            cp.set_gates(circ, c["gate_list"], c["num_selectors"])
            self.by_cs[key] = circ
        return self.by_cs[key]

    def of(self, inst):
        return self.of_cs(self.gc.cs_with(inst["const_row"], inst["consts"]))

    def close(self):
        for circ in self.by_cs.values():
            circ.close()


@pytest.fixture(scope="module")
def circuits(prover, gc):
    cs = Circuits(prover, gc)
    yield cs
    cs.close()


@pytest.fixture(scope="module")
def circuits7(prover, gc7):
    cs = Circuits(prover, gc7)
    yield cs
    cs.close()


def embed(a):
    a = O.arr(a)
    return np.stack([a, np.zeros_like(a)], axis=-1)


def gate_index_at(gc, row, cs=None):
    """the index of the gate that the selector of `row` names"""
    cs = gc.c["cs_values"] if cs is None else cs
    return next(g for g, gl in enumerate(gc.c["gate_list"]) if int(cs[gl[1], row]) == g)


def rows_of(inst):
    return sorted({r for r, _ in inst["writes"]} | {r for _, r in inst.get("bumps", ())})


def expected_gates(gc, inst, witness):
    """-> (count, first (row, gate index, gate type, constraint, value) or None, per-gate counts) from the oracle's row evaluator"""
    per_gate, first, total = [0] * len(gc.c["gate_list"]), None, 0
    for row in rows_of(inst):
        gate = gc.params[gc.c["row_types"][row]]
        consts = inst["consts"] if inst["consts"] is not None and row == inst["const_row"] else gc.consts_at(row)
        vec = O.gate_row_constraints(gate, embed([consts]), embed([witness[:, row]]), embed(gc.pi_hash))[0]
        assert not vec[:, 1].any()
        bad = [k for k in range(len(vec)) if int(vec[k, 0])]
        gi = gate_index_at(gc, row)
        assert gc.c["gate_list"][gi][0] == gate[0]
        per_gate[gi] += len(bad)
        total += len(bad)
        if bad and first is None:     # rows ascend: the first row with a violation is the lowest
            first = (row, gi, gate[0], bad[0], int(vec[bad[0], 0]))
    return total, first, per_gate


def assert_gate_report(rep, want, what):
    total, first, per_gate = want
    assert rep["n_gate_violations"] == total, what
    assert rep["per_gate"] == per_gate, what
    got = (rep["gate_row"], rep["gate_index"], rep["gate_type"], rep["constraint"], rep["constraint_value"])
    assert got == (first if first is not None else (-1, -1, -1, -1, 0)), what
    assert rep["n_copy_violations"] == rep["n_sigma_undecodable"] == rep["n_noncanonical"] == 0, what
    for f in ("copy_row", "copy_column", "copy_to_row", "copy_to_column", "copy_value", "copy_to_value", "sigma_row", "sigma_column",
              "noncanonical_row", "noncanonical_column"):
        assert rep[f] == NONE_FIELDS[f], (what, f)


def check_all(prover, circuits, gc, insts, witnesses, call=MAX_CALL):
    """the witnesses go up once; reports come back from check_witness_batch_dev in calls of `call` instances"""
    import cityprover as cp
    per = witnesses[0].size
    dw = prover.to_device(np.stack(witnesses))
    try:
        circs = [circuits.of(i) for i in insts]
        reports = []
        for lo in range(0, len(insts), call):
            hi = min(lo + call, len(insts))
            reports += cp.check_witness_batch_dev(prover, circs[lo:hi], [gc.c["public_inputs"]] * (hi - lo), dw.at(lo * per))
    finally:
        dw.free()
    return reports


def check_instances(prover, circuits, gc, insts, label):
    witnesses = [gc.witness(i) for i in insts]
    reports = check_all(prover, circuits, gc, insts, witnesses)
    assert len(reports) == len(insts)
    for inst, w, rep in zip(insts, witnesses, reports):
        what = (label, inst["kind"], inst["name"])
        want = expected_gates(gc, inst, w)
        assert (want[0] == 0) == (gc.verdict(inst) == []), what       # the oracle's rows and the definition agree on the verdict
        assert (rep["n_gate_violations"] == 0) == (gc.verdict(inst) == []), what
        if want[0]:
            assert want[1][0] == inst["writes"][0][0], what             # the instance's row
        assert_gate_report(rep, want, what)
    return reports


@pytest.mark.parametrize("gate", S.ALL_GATES, ids=GATE_IDS)
def test_every_instance_of_every_gate(prover, circuits, gc, gate):
    insts = GI.semantic_instances(gc, gate) + GI.cross_gate_instances(gc, gate)
    reports = check_instances(prover, circuits, gc, insts, S.NAME[gate[0]])
    print(f"{S.NAME[gate[0]]}: {len(insts)} instances, {sum(r['n_gate_violations'] == 0 for r in reports)} without a violation")


def violating_instances(gc):
    """per gate type, the first instance on the circuit's own constants that the definition refuses"""
    out = {}
    for g in S.ALL_GATES:
        for i in GI.semantic_instances(gc, g, corruptions="first"):
            if i["consts"] is None and gc.verdict(i):
                out[g[0]] = i
                break
    return out


def merged(*insts):
    return dict(gate=insts[0]["gate"], kind="merged", name=" + ".join(i["name"] for i in insts), writes=[w for i in insts for w in i["writes"]],
                consts=None, const_row=insts[0]["const_row"], bumps=[b for i in insts for b in i["bumps"]])


def test_the_earlier_row_wins_over_the_lower_gate_index(prover, circuits, gc):
    bad = violating_instances(gc)
    pair = next((a, b) for a in bad.values() for b in bad.values()
                if rows_of(a)[0] > rows_of(b)[0] and gate_index_at(gc, rows_of(a)[0]) < gate_index_at(gc, rows_of(b)[0]))
    a, b = pair          # a: the later row under the lower gate index
    both = merged(a, b)
    w = gc.witness(both)
    rep = check_all(prover, circuits, gc, [both], [w])[0]
    want = expected_gates(gc, both, w)
    wa, wb = expected_gates(gc, a, gc.witness(a)), expected_gates(gc, b, gc.witness(b))
    assert want[0] == wa[0] + wb[0] and want[1] == wb[1] and wa[0] and wb[0]
    assert_gate_report(rep, want, both["name"])


def test_reports_of_a_batch_are_independent(prover, circuits, gc):
    bad = list(violating_instances(gc).values())
    honest = GI.semantic_instances(gc, S.ALL_GATES[3], corruptions="first")[0]
    assert honest["kind"] == "honest"
    insts = [bad[0], honest, bad[len(bad) // 2], bad[-1]]
    witnesses = [gc.witness(i) for i in insts]
    together = check_all(prover, circuits, gc, insts, witnesses)
    alone = [check_all(prover, circuits, gc, [i], [w])[0] for i, w in zip(insts, witnesses)]
    assert together == alone
    assert [r["n_gate_violations"] == 0 for r in together] == [False, True, False, False]
    assert len({(r["gate_row"], r["gate_index"]) for r in together}) == 4
    for i, w, r in zip(insts, witnesses, together):
        assert_gate_report(r, expected_gates(gc, i, w), i["name"])


def test_city_common_circuit_edge_rows(prover, circuits7, gc7):
    insts = []
    for g in S.ALL_GATES:
        if g[0] in gc7.params:
            insts += [i for i in GI.semantic_instances(gc7, g, corruptions="first") if i["kind"] == "edge"]
    assert len(insts) > 20
    reports = check_instances(prover, circuits7, gc7, insts, "city-common")
    assert all(r["n_gate_violations"] == 0 for r in reports)      # edge rows are honest rows


# ---- copy constraints --------------------------------------------------------------------------------------------------------
def sigma_targets(gc, cs=None):
    """(target column, target row) of every routed cell, decoded through a dictionary of k_is[c] * omega^i; -1 where there is none"""
    c = gc.c
    cs = c["cs_values"] if cs is None else cs
    sh = c["shape"]
    n, R, ncst = 1 << sh.degree_bits, sh.num_routed_wires, c["num_constants"]
    omega = pow(7, (P - 1) >> sh.degree_bits, P)
    cell = {}
    for col in range(R):
        x = c["k_is"][col] % P
        for i in range(n):
            cell[x] = (col, i)
            x = x * omega % P
    tc, tr = np.full((R, n), -1, np.int64), np.full((R, n), -1, np.int64)
    for col in range(R):
        for i in range(n):
            tc[col, i], tr[col, i] = cell.get(int(cs[ncst + col, i]), (-1, -1))
    return tc, tr


def expected_copies(w, tc, tr):
    """-> (count, first (row, column, to_row, to_column, value, to_value) or None) in the order row, then column"""
    R, n = tc.shape
    bad = [(i, col) for i in range(n) for col in range(R) if tc[col, i] >= 0 and int(w[tc[col, i], tr[col, i]]) % P != int(w[col, i]) % P]
    if not bad:
        return 0, None
    i, col = bad[0]
    return len(bad), (i, col, int(tr[col, i]), int(tc[col, i]), int(w[col, i]) % P, int(w[tc[col, i], tr[col, i]]) % P)


def copy_fields(rep):
    return (rep["copy_row"], rep["copy_column"], rep["copy_to_row"], rep["copy_to_column"], rep["copy_value"], rep["copy_to_value"])


def test_copy_constraints_one_end_bumped(prover, circuits, gc):
    import cityprover as cp
    c = gc.c
    tc, tr = sigma_targets(gc)
    assert (tc >= 0).all()
    assert expected_copies(c["wires"], tc, tr) == (0, None)
    assert len(c["copies"]) >= 4
    witnesses, wants = [c["wires"]], [(0, None)]
    for k, ((ja, ra), (jb, rb)) in enumerate(c["copies"]):
        col, row = (ja, ra) if k % 2 == 0 else (jb, rb)          # one end, alternating
        w = c["wires"].copy()
        w[col, row] = (int(w[col, row]) + 1) % P
        witnesses.append(w)
        wants.append(expected_copies(w, tc, tr))
        assert wants[-1][0] == 2 and wants[-1][1][:2] == min((ra, ja), (rb, jb))     # both ends disagree with each other
    circ = circuits.of_cs(c["cs_values"])
    dw = prover.to_device(np.stack(witnesses))
    try:
        reports = cp.check_witness_batch_dev(prover, [circ] * len(witnesses), [c["public_inputs"]] * len(witnesses), dw.ptr)
    finally:
        dw.free()
    for rep, (count, first) in zip(reports, wants):
        assert rep["n_copy_violations"] == count
        assert copy_fields(rep) == (first if first else (-1, -1, -1, -1, 0, 0))
        # the copies lie beyond the gates of their rows: nothing else is broken
        assert rep["n_gate_violations"] == rep["n_sigma_undecodable"] == rep["n_noncanonical"] == 0 and rep["gate_row"] == -1


def test_a_sigma_value_that_names_no_cell(prover, circuits, gc):
    import cityprover as cp
    c = gc.c
    ncst = c["num_constants"]
    tc, tr = sigma_targets(gc)
    col, row = next((col, i) for i in range(3, tc.shape[1]) for col in range(tc.shape[0]) if (tc[col, i], tr[col, i]) == (col, i))
    cs = c["cs_values"].copy()
    cs[ncst + col, row] = 0          # the loader does not look at sigma
    tc2, tr2 = sigma_targets(gc, cs)
    assert (tc2 < 0).sum() == 1 and tc2[col, row] == -1
    circ = circuits.of_cs(cs)
    w = c["wires"].copy()
    w[col, row] = (int(w[col, row]) + 1) % P     # whatever the cell holds, it is compared with nothing
    for wires in (c["wires"], w):
        rep = cp.check_witness(circ, wires, c["public_inputs"])
        assert rep["n_sigma_undecodable"] == 1 and (rep["sigma_row"], rep["sigma_column"]) == (row, col)
        assert rep["n_copy_violations"] == 0 and copy_fields(rep) == (-1, -1, -1, -1, 0, 0)
        assert rep["n_noncanonical"] == 0


def test_a_wire_equal_to_p_is_counted_and_read_as_zero(prover, circuits, gc):
    import cityprover as cp
    c = gc.c
    w0 = c["wires"]
    row, col = next((i, col) for i, rt in enumerate(c["row_types"]) if rt != S.NOOP for col in range(S.num_wires(gc.params[rt]))
                    if int(w0[col, i]) == 0 and (col, i) not in gc.copied)
    w = w0.copy()
    w[col, row] = P
    circ = circuits.of_cs(c["cs_values"])
    rep = cp.check_witness(circ, w, c["public_inputs"])
    assert rep["n_noncanonical"] == 1 and (rep["noncanonical_row"], rep["noncanonical_column"]) == (row, col)
    assert rep["n_gate_violations"] == 0 and rep["gate_row"] == -1 and rep["n_copy_violations"] == 0      # the verdict of the value 0
    # and a violated row stays violated whichever representative of its values it holds
    inst, zr, zc = next((x, i, col) for x in violating_instances(gc).values() for i in rows_of(x) for col in range(w0.shape[0])
                        if int(gc.witness(x)[col, i]) == 0)
    bad = gc.witness(inst)
    want = expected_gates(gc, inst, bad)
    bad[zc, zr] = P
    rep = cp.check_witness(circuits.of(inst), bad, c["public_inputs"])
    assert rep["n_noncanonical"] == 1 and (rep["noncanonical_row"], rep["noncanonical_column"]) == (zr, zc)
    assert (rep["n_gate_violations"], rep["per_gate"]) == (want[0], want[2])
    assert (rep["gate_row"], rep["gate_index"], rep["gate_type"], rep["constraint"], rep["constraint_value"]) == want[1]


def test_host_and_device_entry_points_agree(prover, circuits, gc):
    import cityprover as cp
    inst = list(violating_instances(gc).values())[1]
    circ = circuits.of(inst)
    for w in (gc.c["wires"], gc.witness(inst)):
        dw = prover.to_device(w[None])
        try:
            dev = cp.check_witness_batch_dev(prover, [circ], [gc.c["public_inputs"]], dw.ptr)[0]
        finally:
            dw.free()
        assert cp.check_witness(circ, w, gc.c["public_inputs"]) == dev
    assert dev["n_gate_violations"] > 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def honest_report_is_clean(prover, circ, gc):
    import cityprover as cp
    rep = cp.check_witness(circ, gc.c["wires"], gc.c["public_inputs"])
    assert {k: rep[k] for k in NONE_FIELDS} == NONE_FIELDS
    assert rep["n_gate_violations"] == rep["n_copy_violations"] == rep["n_sigma_undecodable"] == rep["n_noncanonical"] == 0
    assert rep["per_gate"] == [0] * len(gc.c["gate_list"])


def test_refusals_leave_the_context_usable(prover, circuits, circuits7, gc, gc7):
    import cityprover as cp
    c = gc.c
    circ = circuits.of_cs(c["cs_values"])
    circ7 = circuits7.of_cs(gc7.c["cs_values"])
    bare = cp.Circuit(prover, cp_shape_of(cp, c["shape"]), gc.digest, c["cs_values"])      # no gate set
    pis = c["public_inputs"]
    dw = prover.to_device(np.stack([c["wires"], c["wires"]]))
    lib = prover.lib
    try:
        def refused(message, circs, pi_list, wires_ptr=dw.ptr):
            with pytest.raises(cp.CityProverError, match=message) as e:
                cp.check_witness_batch_dev(prover, circs, pi_list, wires_ptr)
            assert str(e.value).startswith("[-1] ")          # CP_ERR_INVALID_ARG
            honest_report_is_clean(prover, circ, gc)

        refused("n_proofs is 0", [], [])
        refused("NULL argument", [circ], [pis], None)
        refused(r"circuit 1 has no gate set", [circ, bare], [pis, pis])
        refused(r"circuit 1 has a different shape", [circ, circ7], [pis, pis])
        refused(r"proof 1: %d public inputs given, the circuit has %d" % (len(pis) - 1, len(pis)), [circ, circ], [pis, pis[:-1]])
        bad_pi = np.array(pis, dtype=np.uint64)
        bad_pi[1] = P
        refused(r"proof 0: public input 1 is not canonical", [circ, circ], [bad_pi, pis])
        # NULL report array, NULL circuit: the bare ABI
        one = (ctypes.c_size_t * 1)(len(pis))
        cs = (ctypes.c_void_p * 1)(circ.handle)
        pi_arr = O.arr(pis)
        pp = (ctypes.POINTER(ctypes.c_uint64) * 1)(pi_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
        assert lib.cp_circuit_check_witness_dev(prover.ctx, 1, cs, pp, one, dw.ptr, None, None) == -1
        assert b"NULL argument" in lib.cp_last_error(prover.ctx)
        cs[0] = None
        rep = cp.WitnessReport()
        assert lib.cp_circuit_check_witness_dev(prover.ctx, 1, cs, pp, one, dw.ptr, ctypes.byref(rep), None) == -1
        assert b"circuit 0 is NULL" in lib.cp_last_error(prover.ctx)
        assert lib.cp_circuit_check_witness(circ.handle, None, pp[0], len(pis), ctypes.byref(rep), None) == -1
        assert b"NULL argument" in lib.cp_last_error(prover.ctx)
        honest_report_is_clean(prover, circ, gc)
        # without per_gate_out the report is the same
        cs[0] = circ.handle
        assert lib.cp_circuit_check_witness_dev(prover.ctx, 1, cs, pp, one, dw.ptr, ctypes.byref(rep), None) == 0
        assert rep.n_gate_violations == 0 and rep.gate_row == -1
    finally:
        dw.free()
        bare.close()


def test_injected_allocation_failures(gc):
    """cp_fault_inject(CP_FAULT_DEVMEM, j) for every j until the check gets through: out of memory, and the same context then
    gives the report of a context nothing was refused on"""
    import cityprover as cp
    lib = cp.load_library()
    c = gc.c
    inst = next(iter(violating_instances(gc).values()))
    w = gc.witness(inst)
    want = None
    refused = 0
    try:
        for j in range(16):
            p = cp.Prover(0)
            circ = None
            try:
                circ = cp.Circuit(p, cp_shape_of(cp, c["shape"]), gc.digest, c["cs_values"])
                cp.set_gates(circ, c["gate_list"], c["num_selectors"])
                if want is None:
                    q = cp.Circuit(p, cp_shape_of(cp, c["shape"]), gc.digest, c["cs_values"])
                    cp.set_gates(q, c["gate_list"], c["num_selectors"])
                    want = cp.check_witness(q, w, c["public_inputs"])
                    q.close()
                    assert want["n_gate_violations"] > 0
                    continue          # a fresh context for the walk itself
                cp.batch_pool_trim(p)      # a refused allocation is tried again after the pool gave its buffers back: it holds none
                assert lib.cp_fault_inject(DEVMEM, j - 1) == 0
                try:
                    got = cp.check_witness(circ, w, c["public_inputs"])
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert str(e).startswith("[-4] ") and "out of memory" in str(e), (j, str(e))      # CP_ERR_OOM
                    refused += 1
                    assert cp.check_witness(circ, w, c["public_inputs"]) == want, "allocation %d refused: the context did not recover" % (j - 1)
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                assert got == want
                break
            finally:
                lib.cp_fault_inject(DEVMEM, -1)
                if circ is not None:
                    circ.close()
                p.close()
        else:
            pytest.fail("the walk did not end")
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    assert refused >= 1      # the staging buffer and the arena of a fresh context (the power table of omega came with the circuit)
