"""Whole proofs on the CPU oracle against the per-row gate definition (tests/gate_semantics.py), a few per gate, on the ALL_GATES
circuit at 2^6 rows with its real selector grouping: every honest edge row, every malicious row and one accepted corruption of each
gate, placed on that gate's row, must prove and then verify exactly when the definition names no violation; an honest row of gate A
on a row whose selector says gate B is refused, and the same values on a Noop row are accepted (a filter binds a gate to its own
rows and leaves the others alone)."""
import pytest

import gate_instances as GI
import gate_semantics as S
import oracle_lib as O

GATE_IDS = [S.NAME[g[0]] for g in S.ALL_GATES]
# instances per gate: 1 honest + edges (less the two that set the public-inputs hash itself, which a proof cannot choose)
# + malicious + 1 accepted corruption (every gate but Poseidon has one) + 2 cross-gate (none for Noop)
NUM_INSTANCES = {S.NOOP: 1 + 1 + 0 + 1 + 0, S.CONSTANT: 1 + 2 + 1 + 1 + 2, S.PUBLIC_INPUT: 1 + 1 + 1 + 1 + 2, S.ARITHMETIC: 1 + 4 + 1 + 1 + 2,
                 S.POSEIDON: 1 + 5 + 3 + 0 + 2, S.COMPARISON: 1 + 10 + 4 + 1 + 2, S.U32_ARITHMETIC: 1 + 8 + 6 + 1 + 2,
                 S.U32_RANGE_CHECK: 1 + 7 + 2 + 1 + 2, S.U32_ADD_MANY: 1 + 5 + 2 + 1 + 2, S.U32_SUBTRACTION: 1 + 9 + 2 + 1 + 2,
                 S.U32_INTERLEAVE: 1 + 5 + 1 + 1 + 2, S.UNINTERLEAVE_TO_U32: 1 + 9 + 1 + 1 + 2, S.UNINTERLEAVE_TO_B32: 1 + 9 + 1 + 1 + 2,
                 S.ARITHMETIC_EXT: 1 + 4 + 1 + 1 + 2, S.MUL_EXT: 1 + 4 + 1 + 1 + 2, S.BASE_SUM: 1 + 4 + 2 + 1 + 2,
                 S.RANDOM_ACCESS: 1 + 4 + 2 + 1 + 2, S.REDUCING: 1 + 6 + 1 + 1 + 2, S.REDUCING_EXT: 1 + 6 + 1 + 1 + 2,
                 S.POSEIDON_MDS: 1 + 4 + 1 + 1 + 2, S.COSET_INTERPOLATION: 1 + 7 + 1 + 1 + 2, S.EXPONENTIATION: 1 + 9 + 1 + 1 + 2}


@pytest.fixture(scope="module")
def gc():
    return GI.GateCircuit()


def test_the_circuit_has_the_real_selector_grouping(gc):
    assert gc.c["groups"] == [(0, 7), (7, 13), (13, 18), (18, 21), (21, 22)] and gc.c["copies"]
    assert sorted(gc.row_of) == list(range(22))


@pytest.mark.parametrize("gate", S.ALL_GATES, ids=GATE_IDS)
def test_prove_then_verify_agrees_with_the_definition(gc, gate):
    insts = GI.semantic_instances(gc, gate, corruptions="accepted") + GI.cross_gate_instances(gc, gate)
    assert len(insts) == NUM_INSTANCES[gate[0]]
    kinds = [i["kind"] for i in insts]
    c = gc.c
    O.lib().or_set_threads(8)
    try:
        for inst in insts:
            want_ok = gc.verdict(inst) == []
            # what each kind is for: honest rows hold, malicious rows and another gate's row do not, the rest is free
            assert want_ok == (inst["kind"] not in ("malicious", "other gate's row")), (inst["kind"], inst["name"], gc.verdict(inst)[:3])
            cs = gc.cs_with(inst["const_row"], inst["consts"])
            proof, _ = O.prove_full(c["shape"], c["gates"], gc.digest, c["public_inputs"], cs, gc.witness(inst))
            rc = O.verify_full(c["shape"], c["gates"], gc.digest, gc.cap(cs), proof)
            assert (rc == 0) if want_ok else (rc <= -1000), (S.NAME[gate[0]], inst["kind"], inst["name"], rc)
    finally:
        O.lib().or_set_threads(1)
    assert kinds.count("corruption") == (gate[0] != S.POSEIDON)
