"""GPU: every instance of the per-row gate definition (tests/gate_semantics.py) through the C ABI, on the ALL_GATES circuit at 2^6
rows (tests/gate_instances.py). The quotient kernels are the device's instantiation of csrc/gates.h, and PoseidonGate and
PoseidonMdsGate have device code of their own in csrc/quotient.h that nothing on the host runs: here every wire of every gate goes
through them.

Per gate type, one batch: the honest witness, every edge row, every malicious row and every corruption of the definition (each wire
+1; ranged wires also the first out-of-range value and another in-range value; one wire beyond the gate). It goes up once and is
proved by cp.prove_batch_dev in calls of at most 256.
  VERDICTS, all instances: cp.verify accepts exactly those the definition finds no violation in and refuses the others with
    "vanishing identity"; the oracle's verifier accepts the accepted ones too.
  BYTES, the honest row, the edge rows, the malicious rows and the first corruption of each gate (under 20 per gate): equal to
    O.prove_full's. A violated witness still has well-defined bytes. The other corruptions are held by verdict only.
The forms of the quotient (one grid, a launch per gate, the arithmetic group, the tile kernel): the edge and malicious instances of
all gates, and on the city-common circuit at 2^7 rows (which takes the tile kernel) the edge rows of its own gates, prove to the
same bytes and verdicts on a context of its own under every row of test_gpu_gate_set.QUOT_ROWS, in calls of 1 and of 3."""
import collections
import hashlib

import numpy as np
import pytest

import gate_instances as GI
import gate_semantics as S
import oracle_lib as O
import synth_gates as SG
from test_gate_semantics import NUM_ACCEPTED, NUM_CORRUPTIONS, NUM_EDGES, NUM_MALICIOUS
from test_gpu_gate_set import QUOT_BATCHES, QUOT_RATE_BITS, QUOT_ROWS, QUOT_WIRES, quotient_plan
from test_gpu_prove_full import cp_shape_of

pytestmark = pytest.mark.gpu

GATE_IDS = [S.NAME[g[0]] for g in S.ALL_GATES]
MAX_CALL = 256
# edge operands that set the public-inputs hash itself cannot be a proof's (PublicInput has one)
NUM_PROOF_EDGES = dict(NUM_EDGES)
NUM_PROOF_EDGES[S.PUBLIC_INPUT] -= 1


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
    """one cp.Circuit per set of constants (an edge row that sets its gate's constants proves against a circuit of its own)"""

    def __init__(self, prover, gc):
        self.prover, self.gc, self.by_cs = prover, gc, {}

    def of(self, inst):
        import cityprover as cp
        cs = self.gc.cs_with(inst["const_row"], inst["consts"])
        key = cs.tobytes()
        if key not in self.by_cs:
            c = self.gc.c
            circ = cp.Circuit(self.prover, cp_shape_of(cp, c["shape"]), self.gc.digest, cs)
            cp.set_gates(circ, c["gate_list"], c["num_selectors"])
            self.by_cs[key] = circ
        return self.by_cs[key]

    def close(self):
        for circ in self.by_cs.values():
            circ.close()


@pytest.fixture(scope="module")
def circuits(prover, gc):
    cs = Circuits(prover, gc)
    yield cs
    cs.close()


_ORACLE = {}    # the oracle's proof of an instance, computed once for the whole module


def oracle_proof(gc, inst, witness):
    cs = gc.cs_with(inst["const_row"], inst["consts"])
    key = hashlib.sha256(cs.tobytes() + witness.tobytes()).digest()
    if key not in _ORACLE:
        c = gc.c
        O.lib().or_set_threads(8)
        try:
            _ORACLE[key] = O.prove_full(c["shape"], c["gates"], gc.digest, c["public_inputs"], cs, witness)[0]
        finally:
            O.lib().or_set_threads(1)
    return _ORACLE[key]


def prove_all(prover, circuits, gc, insts, witnesses, call):
    """the witnesses go up once; proofs come back from prove_batch_dev in calls of `call` instances"""
    import cityprover as cp
    per = witnesses[0].size
    dw = prover.to_device(np.stack(witnesses))
    try:
        circs = [circuits.of(i) for i in insts]
        proofs = []
        for lo in range(0, len(insts), call):
            hi = min(lo + call, len(insts))
            proofs += cp.prove_batch_dev(prover, circs[lo:hi], [gc.c["public_inputs"]] * (hi - lo), dw.at(lo * per))
    finally:
        dw.free()
    return circs, proofs


def device_verdict(circ, proof):
    import cityprover as cp
    try:
        cp.verify(circ, proof)
        return True
    except cp.CityProverError as e:
        assert "vanishing identity" in str(e), str(e)
        return False


@pytest.mark.parametrize("gate", S.ALL_GATES, ids=GATE_IDS)
def test_every_instance_through_the_abi(prover, circuits, gc, gate):
    t = gate[0]
    insts = GI.semantic_instances(gc, gate)
    kinds = [i["kind"] for i in insts]
    assert kinds == ["honest"] + ["edge"] * NUM_PROOF_EDGES[t] + ["malicious"] * NUM_MALICIOUS[t] + ["corruption"] * NUM_CORRUPTIONS[t]
    witnesses = [gc.witness(i) for i in insts]
    want_ok = [gc.verdict(i) == [] for i in insts]
    # from the definition: honest and edge rows hold, malicious rows do not, and of the corruptions the literal number is free
    assert all(want_ok[:1 + NUM_PROOF_EDGES[t]]) and not any(want_ok[1 + NUM_PROOF_EDGES[t]:][:NUM_MALICIOUS[t]])
    assert sum(want_ok[-NUM_CORRUPTIONS[t]:]) == NUM_ACCEPTED[t]
    circs, proofs = prove_all(prover, circuits, gc, insts, witnesses, MAX_CALL)
    assert len(proofs) == len(insts)
    print(f"{S.NAME[t]}: {len(insts)} instances, the definition accepts {sum(want_ok)}")
    got_ok = [device_verdict(c, p) for c, p in zip(circs, proofs)]
    wrong = [(i["kind"], i["name"]) for i, g, w in zip(insts, got_ok, want_ok) if g != w]
    assert not wrong, (S.NAME[t], wrong[:10])
    for inst, circ, proof, ok in zip(insts, circs, proofs, want_ok):
        if ok:
            assert O.verify_full(gc.c["shape"], gc.c["gates"], gc.digest, circ.cs_cap(), proof) == 0, (inst["kind"], inst["name"])
    n_bytes = 1 + NUM_PROOF_EDGES[t] + NUM_MALICIOUS[t] + 1
    assert n_bytes < 20
    for inst, w, proof in list(zip(insts, witnesses, proofs))[:n_bytes]:
        assert proof == oracle_proof(gc, inst, w), (S.NAME[t], inst["kind"], inst["name"])


def form_instances(gc, kinds):
    out = []
    for g in S.ALL_GATES:
        if g[0] in gc.params:
            out += [i for i in GI.semantic_instances(gc, g, corruptions="first") if i["kind"] in kinds]
    return out


@pytest.mark.parametrize("options", QUOT_ROWS, ids=[",".join(f"{k}={v}" for k, v in o.items()) for o in QUOT_ROWS])
def test_every_form_of_the_quotient_agrees_with_the_definition(options, gc, gc7):
    import cityprover as cp
    p = cp.Prover(0)
    try:
        for name, v in options.items():
            p.set_option(name, v)
        for g, kinds, count in ((gc, ("edge", "malicious"), sum(NUM_PROOF_EDGES.values()) + sum(NUM_MALICIOUS.values())),
                                (gc7, ("edge",), sum(NUM_PROOF_EDGES[t] for t in gc7.params))):
            insts = form_instances(g, kinds)
            assert len(insts) == count
            witnesses = [g.witness(i) for i in insts]
            want = [oracle_proof(g, i, w) for i, w in zip(insts, witnesses)]
            want_ok = [g.verdict(i) == [] for i in insts]
            assert want_ok == [i["kind"] == "edge" for i in insts]
            circuits = Circuits(p, g)
            types = [x[0] for x in g.c["gate_list"]]
            verdict_of = {}
            try:
                for B in QUOT_BATCHES:
                    p.profile_begin()
                    try:
                        circs, proofs = prove_all(p, circuits, g, insts, witnesses, B)
                    finally:
                        prof = p.profile_end()
                    differ = [(i["gate"], i["name"]) for i, a, b in zip(insts, proofs, want) if a != b]
                    assert not differ, (options, B, differ[:5])
                    for c, pr in zip(circs, proofs):   # the bytes are the same for both batch sizes: one verification each
                        if pr not in verdict_of:
                            verdict_of[pr] = device_verdict(c, pr)
                    assert [verdict_of[pr] for pr in proofs] == want_ok
                    # the launches say which form of the quotient ran (test_gpu_gate_set's plan; its rows reach all four forms)
                    sizes = collections.Counter(min(B, len(insts) - lo) for lo in range(0, len(insts), B))
                    plan = collections.Counter()
                    for size, n in sizes.items():
                        one = quotient_plan(types, size, options, QUOT_WIRES, (1 << g.c["shape"].degree_bits) << QUOT_RATE_BITS)
                        for k, v in one.items():
                            plan[k] += v * n
                    launches = collections.Counter({k: v["launches"] for k, v in prof.items() if k.startswith("quotient_") and k != "quotient_fill_l0"})
                    assert launches == plan, (options, B, dict(launches), dict(plan))
            finally:
                circuits.close()
    finally:
        p.close()
