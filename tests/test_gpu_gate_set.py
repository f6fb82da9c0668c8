"""GPU A8 gate-set parity: circuits containing every gate of the city-common set (pad_circuit.rs:31-55) and every
in-tree u32 gate, with plonky2's selector grouping. cp_prove_batch bytes == oracle bytes; cp_verify (vanishing identity
over F_p^2 through the same gates.h code, host side) and the oracle verifier accept; corrupted wires are rejected."""
import collections

import pytest

import oracle_lib as O
import synth_gates as SG
from test_gpu_prove_full import cp_shape_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


@pytest.mark.parametrize("name,gate_set,db,arity", [("city_common", SG.CITY_COMMON, 6, (2,)), ("all", SG.ALL_GATES, 6, (2,)),
                                                    ("all_2^8", SG.ALL_GATES, 8, (2, 2))])
def test_gate_set_proofs_byte_identical(prover, name, gate_set, db, arity):
    import cityprover as cp
    c = SG.build_gate_set(gate_set, db=db, seed=11 + db, arity_bits=arity)
    sh = cp_shape_of(cp, c["shape"])
    digest = [6, 6, 6, db]
    circ = cp.Circuit(prover, sh, digest, c["cs_values"])
    cp.set_gates(circ, c["gate_list"], c["num_selectors"])
    dw = prover.to_device(c["wires"][None])
    got = cp.prove_batch_dev(prover, [circ], [c["public_inputs"]], dw.ptr)[0]
    O.lib().or_set_threads(8)
    try:
        want, _ = O.prove_full(c["shape"], c["gates"], digest, c["public_inputs"], c["cs_values"], c["wires"])
    finally:
        O.lib().or_set_threads(1)
    assert got == want
    cp.verify(circ, got)
    assert O.verify_full(c["shape"], c["gates"], digest, circ.cs_cap(), got) == 0
    params = {g[0]: g for g in c["sorted_gates"]}
    for t in sorted(set(c["row_types"])):
        nw = SG.gate_num_wires(params[t])
        if nw == 0:
            continue
        row = c["row_types"].index(t)
        w = c["wires"].copy()
        w[nw - 1, row] = (int(w[nw - 1, row]) + 1) % O.P
        dw2 = prover.to_device(w[None])
        bad = cp.prove_batch_dev(prover, [circ], [c["public_inputs"]], dw2.ptr)[0]
        dw2.free()
        with pytest.raises(cp.CityProverError, match="vanishing identity"):
            cp.verify(circ, bad)
    dw.free(); circ.close()


# ---- the launch plan of the quotient (csrc/quotient.inc), restated: label -> launches of one prove_batch call ----
GATE_LABEL = {SG.CONSTANT: "constant", SG.PUBLIC_INPUT: "public_input", SG.ARITHMETIC: "arithmetic", SG.POSEIDON: "poseidon",
              SG.COMPARISON: "comparison", SG.U32_ARITHMETIC: "u32_arithmetic", SG.U32_RANGE_CHECK: "u32_range_check",
              SG.U32_ADD_MANY: "u32_add_many", SG.U32_SUBTRACTION: "u32_subtraction", SG.U32_INTERLEAVE: "u32_interleave",
              SG.UNINTERLEAVE_TO_U32: "uninterleave_to_u32", SG.UNINTERLEAVE_TO_B32: "uninterleave_to_b32",
              SG.ARITHMETIC_EXT: "arithmetic_ext", SG.MUL_EXT: "mul_ext", SG.BASE_SUM: "base_sum", SG.RANDOM_ACCESS: "random_access",
              SG.REDUCING: "reducing", SG.REDUCING_EXT: "reducing_ext", SG.POSEIDON_MDS: "poseidon_mds",
              SG.COSET_INTERPOLATION: "coset_interpolation", SG.EXPONENTIATION: "exponentiation"}
ARITH_FAMILY = (SG.CONSTANT, SG.PUBLIC_INPUT, SG.ARITHMETIC, SG.ARITHMETIC_EXT, SG.MUL_EXT)
PIECE_WEIGHT = {SG.POSEIDON: 9.7, SG.REDUCING: 4.5, SG.COMPARISON: 4.2, SG.REDUCING_EXT: 3.5, SG.COSET_INTERPOLATION: 3.2, SG.BASE_SUM: 2.9,
                SG.RANDOM_ACCESS: 1.8, SG.POSEIDON_MDS: 1.1, SG.ARITHMETIC: 1.5, SG.ARITHMETIC_EXT: 1.5, SG.MUL_EXT: 1.5, SG.CONSTANT: 0.2,
                SG.PUBLIC_INPUT: 0.2}
TILE, MAXC, LDS_MAX = 64, 4, 160 * 1024


def arith_group(types):
    """indices of the gates that run as one piece: the first of each family type, if there are at least two"""
    first = {}
    for gi, t in enumerate(types):
        if t in ARITH_FAMILY:
            first.setdefault(t, gi)
    return set(first.values()) if len(first) >= 2 else set()


def tile_fits(types, num_wires):
    """the tile planner: longest piece first onto the lightest of four bins; at most four pieces per bin, LDS within a workgroup's"""
    group = arith_group(types)
    weights = [7.1] + ([4.5] if group else []) + [PIECE_WEIGHT.get(t, 3.0) for gi, t in enumerate(types) if gi not in group and t != SG.NOOP]
    load, size = [0.0] * 4, [0] * 4
    for w in sorted(weights, reverse=True):
        b = load.index(min(load))
        load[b] += w
        size[b] += 1
    depth = max(size)
    return depth <= 4 and max(num_wires, 4 * depth * MAXC) * TILE * 8 <= LDS_MAX


def quotient_plan(types, B, options, num_wires, N):
    plan = collections.Counter({"quotient_alpha_powers": 1})
    if B <= options.get("QUOT_ALL_MAX", 4):
        plan.update(["quotient_all", "quotient_finish"])
    elif options.get("QUOT_TILE", 0) and N % TILE == 0 and tile_fits(types, num_wires):
        plan.update(["quotient_tile"])
    else:
        group = arith_group(types) if options.get("QUOT_GROUP", 1) else set()
        plan.update(["quotient_perm", "quotient_finish"] + (["quotient_arith_group"] if group else []))
        plan.update("quotient_" + GATE_LABEL[t] for gi, t in enumerate(types) if gi not in group and t != SG.NOOP)
    return plan


def form_of(plan):
    if plan["quotient_all"] or plan["quotient_tile"]:
        return "all" if plan["quotient_all"] else "tile"
    return "arith_group" if plan["quotient_arith_group"] else "per_gate"


QUOT_ROWS = [dict(QUOT_ALL_MAX=0), dict(QUOT_ALL_MAX=0, QUOT_GROUP=0), dict(QUOT_ALL_MAX=0, QUOT_TILE=1),
             dict(QUOT_ALL_MAX=0, QUOT_FLIP=0, QUOT_TILE=1, QUOT_GROUP=0), dict(QUOT_ALL_MAX=100)]
QUOT_SETS = ((SG.ALL_GATES, 6), (SG.CITY_COMMON, 7))
QUOT_BATCHES = (1, 3)
QUOT_WIRES, QUOT_RATE_BITS = 135, 3   # build_gate_set's defaults


def test_the_quotient_rows_reach_every_form():
    """Every row below asserts the launches this plan predicts, so the plan reaching all four forms means the GPU ran all four. With
    all 22 gate types the tile planner needs five pieces per bin and the call falls back to a launch per gate; the city-common set
    needs three and takes the tile kernel."""
    seen = {form_of(quotient_plan([g[0] for g in gs], B, o, QUOT_WIRES, (1 << db) << QUOT_RATE_BITS))
            for o in QUOT_ROWS for gs, db in QUOT_SETS for B in QUOT_BATCHES}
    assert seen == {"all", "tile", "arith_group", "per_gate"}
    assert not tile_fits([g[0] for g in SG.ALL_GATES], QUOT_WIRES) and tile_fits([g[0] for g in SG.CITY_COMMON], QUOT_WIRES)


@pytest.mark.parametrize("options", QUOT_ROWS)
def test_every_form_of_the_quotient_gives_the_same_bytes(options):
    """The quotient has four forms, chosen by batch size and switches: every piece a slice of one grid (small batches), a launch per
    gate, the arithmetic family grouped into one launch (round 4, default for batches that fill the chip), and a workgroup per
    64-point tile with the wires staged in LDS once (round 4, off by default). cp_ctx_set_option forces each on a context of its
    own; a circuit with all 22 gate types and one with the city-common set must prove to the oracle's bytes under every one, with
    the quotient launches that quotient_plan predicts (the L_0 table is filled by the first proof of a shape on a context)."""
    import cityprover as cp
    p = cp.Prover(0)
    try:
        for name, v in options.items():
            p.set_option(name, v)
        for gate_set, db in QUOT_SETS:
            c = SG.build_gate_set(gate_set, db=db, seed=31 + db, arity_bits=(2,))
            assert c["wires"].shape[0] == QUOT_WIRES and c["shape"].rate_bits == QUOT_RATE_BITS
            types = [g[0] for g in c["gate_list"]]
            sh = cp_shape_of(cp, c["shape"])
            digest = [5, 5, 5, db]
            circ = cp.Circuit(p, sh, digest, c["cs_values"])
            cp.set_gates(circ, c["gate_list"], c["num_selectors"])
            O.lib().or_set_threads(8)
            try:
                want, _ = O.prove_full(c["shape"], c["gates"], digest, c["public_inputs"], c["cs_values"], c["wires"])
            finally:
                O.lib().or_set_threads(1)
            for i, B in enumerate(QUOT_BATCHES):
                p.profile_begin()
                try:
                    got = cp.prove_batch(p, [circ] * B, [c["public_inputs"]] * B, [c["wires"]] * B)
                finally:
                    prof = p.profile_end()
                assert all(g == want for g in got), (options, B)
                launches = collections.Counter({k: v["launches"] for k, v in prof.items() if k.startswith("quotient_")})
                plan = quotient_plan(types, B, options, QUOT_WIRES, (1 << db) << QUOT_RATE_BITS)
                if i == 0:
                    plan["quotient_fill_l0"] = 1
                print(options, len(types), B, dict(launches))
                assert launches == plan, (options, len(types), B, dict(launches))
            circ.close()
    finally:
        p.close()


def test_set_gates_parameter_validation(prover):
    import cityprover as cp
    c = SG.build_gate_set(SG.CITY_COMMON, db=6, seed=1, arity_bits=(2,))
    sh = cp_shape_of(cp, c["shape"])
    circ = cp.Circuit(prover, sh, [1, 1, 1, 1], c["cs_values"])
    for bad in [(cp.GATE_RANDOM_ACCESS, 0, 0, 1, 5, 1, 0),        # bits > 4
                (cp.GATE_RANDOM_ACCESS, 0, 0, 1, 4, 8, 0),        # 8 copies need 176 wires
                (cp.GATE_COSET_INTERPOLATION, 0, 0, 1, 4, 1, 0),  # degree < 2
                (cp.GATE_COSET_INTERPOLATION, 0, 0, 1, 6, 6, 0),  # 64-point coset
                (cp.GATE_BASE_SUM, 0, 0, 1, 63, 1, 0),            # base 1
                (cp.GATE_REDUCING, 0, 0, 1, 44, 0, 0),            # 136 wires
                (cp.GATE_U32_ADD_MANY, 0, 0, 1, 5, 0, 0),         # no addends
                (cp.GATE_UNINTERLEAVE_TO_U32, 0, 0, 1, 3, 0, 0),  # 201 wires
                (cp.GATE_EXPONENTIATION, 0, 0, 1, 67, 0, 0),      # 136 wires
                (22, 0, 0, 1, 0, 0, 0)]:                          # unknown type
        with pytest.raises(cp.CityProverError):
            cp.set_gates(circ, [bad], 1)
    circ.close()


@pytest.mark.parametrize("db,arity", [(13, (4, 4)), (14, (4, 4, 1))])
def test_larger_circuits(prover, db, arity):
    """Degrees above the 4096-point single-pass NTT tile (op circuits before minification are 2^13..2^15 rows): the
    multi-pass iNTT / LDE paths, deeper trees and a third FRI layer must give the oracle's bytes too."""
    import cityprover as cp
    c = SG.build_gate_set(SG.CITY_COMMON, db=db, seed=40 + db, arity_bits=arity, cap_height=4, num_query_rounds=8,
                          pow_bits=8, noop_fraction=0.3)
    sh = cp_shape_of(cp, c["shape"])
    digest = [9, 9, db, 1]
    circ = cp.Circuit(prover, sh, digest, c["cs_values"])
    cp.set_gates(circ, c["gate_list"], c["num_selectors"])
    got = cp.prove(circ, c["wires"], c["public_inputs"])
    O.lib().or_set_threads(16)
    try:
        want, _ = O.prove_full(c["shape"], c["gates"], digest, c["public_inputs"], c["cs_values"], c["wires"])
    finally:
        O.lib().or_set_threads(1)
    assert got == want
    cp.verify(circ, got)
    circ.close()
