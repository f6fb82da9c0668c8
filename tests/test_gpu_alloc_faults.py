"""A refused device allocation anywhere inside an entry point is an out-of-memory STATUS that leaks nothing and leaves the context
usable ("who owns device memory"; csrc/dev_mem.h). For each entry point: the expected result once on a clean context
(against the oracle where the other tests compare it), then a walk over its allocations - for j = 0, 1, ...: a fresh context (cold
caches), an empty pool (nothing a trim-and-retry could absorb the fault with), cp_fault_inject(CP_FAULT_DEVMEM, j), the call. A call
that raises must report out of memory, and the same call on the same context, fault disarmed, must give exactly the expected
result. The first call that succeeds has not reached the fault and ends the walk. These are refused allocations that return a
status (as in test_gpu_fri_generic.py's pool test): nothing here faults the device."""
import re

import numpy as np
import pytest

import air_programs as A
import oracle_lib as O
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
DEVMEM = 3   # CP_FAULT_DEVMEM
MAX_WALK = 64


@pytest.fixture(scope="module")
def setup_prover():
    """holds what the calls under test only read (device inputs, proving keys): made before any fault is armed"""
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def walk(call, want):
    """call(prover) -> something comparable with ==; returns how many allocations of the call were refused"""
    import cityprover
    lib = cityprover.load_library()
    refused = 0
    try:
        for j in range(MAX_WALK):
            p = cityprover.Prover(0)
            try:
                cityprover.batch_pool_trim(p)
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    got = call(p)
                except cityprover.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    msg = str(e)
                    assert re.search("(?i)memory", msg), (j, msg)
                    if msg.startswith("["):   # entry points that return a status (the ones that return a handle have only the message)
                        assert msg.startswith("[-4]"), (j, msg)   # CP_ERR_OOM
                    refused += 1
                    assert call(p) == want, "allocation %d refused: the context did not recover" % j
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                assert got == want
                break
            finally:
                lib.cp_fault_inject(DEVMEM, -1)
                p.close()
        else:
            pytest.fail("the walk did not end before j = %d" % MAX_WALK)
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    assert refused >= 1
    return refused


def clean(call):
    import cityprover
    p = cityprover.Prover(0)
    try:
        return call(p)
    finally:
        p.close()


def limbs(v, n):
    return [(int(v) >> (64 * i)) & (2**64 - 1) for i in range(n)]


def test_ntt_from_host(setup_prover):
    x = O.splitmix64_felts(11, 2 << 5).reshape(2, 32)
    call = lambda p: p.ntt(x).tobytes()
    want = clean(call)
    assert want == np.array([O.ntt(x[0]), O.ntt(x[1])], dtype=np.uint64).tobytes()
    assert walk(call, want) >= 2   # the upload and a power table at the least (the scratch may already be large enough)


def test_merkle_cap(setup_prover):
    rows = O.splitmix64_felts(12, 8 * 5).reshape(8, 5)
    call = lambda p: p.merkle_cap(rows, 1).tobytes()
    want = clean(call)
    assert want == np.asarray(O.merkle_tree(rows, 1), dtype=np.uint64).tobytes()
    assert walk(call, want) >= 2


@pytest.mark.parametrize("salted", [False, True])
def test_poly_batch(setup_prover, salted):
    import cityprover
    k, db, rb, ch = 3, 5, 1, 1
    polys = O.splitmix64_felts(13, k << db).reshape(k, 1 << db)
    salts = O.splitmix64_felts(14, 4 << (db + rb)).reshape(4, 1 << (db + rb)) if salted else None

    def call(p):
        g = cityprover.PolyBatch(p, polys, rb, ch, False, salts)
        try:
            return g.cap().tobytes()
        finally:
            g.close()
    want = clean(call)
    o = O.Batch(polys, rb, ch, False, salts)
    try:
        assert want == np.asarray(o.cap(), dtype=np.uint64).tobytes()
    finally:
        o.close()
    assert walk(call, want) >= (5 if salted else 4)


def test_circuit_load_and_one_proof(setup_prover):
    import cityprover
    from synth_circuit import build as build_circuit
    c = build_circuit(db=5, num_routed=16, num_wires=20, chunk=8, rate_bits=3, seed=1)   # the smallest shape the other tests build
    s = c["shape"]
    sh = cityprover.standard_recursion_shape(
        degree_bits=s.degree_bits, num_constants=s.num_constants, num_routed_wires=s.num_routed_wires, num_wires=s.num_wires,
        num_challenges=s.num_challenges, num_partial_products=s.num_partial_products, quotient_degree_factor=s.quotient_degree_factor,
        rate_bits=s.rate_bits, cap_height=s.cap_height, pow_bits=s.pow_bits, num_query_rounds=s.num_query_rounds,
        arity_bits=tuple(s.arity_bits[i] for i in range(s.n_arity)), num_public_inputs=len(c["public_inputs"]))

    def call(p):
        circ = cityprover.Circuit(p, sh, [1, 2, 3, 4], c["cs_values"])
        try:
            cityprover.set_gates(circ, c["gate_list"], 1)
            return cityprover.prove(circ, c["wires"], c["public_inputs"])   # wires from the host: the staging buffer, the arena, the pinned area
        finally:
            circ.close()
    want = clean(call)
    assert want == O.prove_full(c["shape"], c["gates"], [1, 2, 3, 4], c["public_inputs"], c["cs_values"], c["wires"])[0]
    assert walk(call, want) >= 6   # the circuit's six arrays at the least


def test_stark_prove(setup_prover):
    import cityprover
    db, rb, ch, pow_bits, nq, arity = 4, 1, 2, 5, 12, (2,)
    cons, ma, mb = A.lookup_programs()
    trace = A.lookup_trace(1 << db)

    def call(p):
        gp = [x.gpu(p) for x in (cons, ma, mb)]
        try:
            gd, keep = cityprover.stark_desc(db, 1, 2, cityprover.fri_params(db, rb, ch, pow_bits, nq, arity), A.LOOKUP_K0, gp[0], A.LOOKUP_K1, 3,
                                             steps=A.lookup_steps(gp[1], gp[2]))
            gc = cityprover.ChallengerState()
            gc.observe([1, 2, 3, 4, 5])
            return cityprover.stark_prove(p, gd, trace, gc), gc.as_tuple()
        finally:
            for g in gp:
                g.close()
    want = clean(call)
    op = [x.oracle() for x in (cons, ma, mb)]
    od, okeep = O.stark_desc(db, 1, 2, O.fri_params(db, rb, ch, pow_bits, nq, arity), A.LOOKUP_K0, op[0], A.LOOKUP_K1, 3, steps=A.lookup_steps(op[1], op[2]))
    oc = O.challenger_new()
    O.challenger_observe(oc, [1, 2, 3, 4, 5])
    assert want == (O.stark_prove(od, trace, oc), O.challenger_tuple(oc))
    assert walk(call, want) >= 8   # the value columns, a compiled program, the selector table, three commitments of four buffers


def test_msm_g1_from_host(setup_prover):
    import cityprover
    _, r, G = O.bls_constants()
    rng = np.random.default_rng(33)
    pts = [O.bls_g1_mul(G, int.from_bytes(rng.bytes(32), "little") % r) for _ in range(8)]
    xy = np.array([limbs(P[0], 6) + limbs(P[1], 6) for P in pts], dtype=np.uint64)[rng.integers(0, 8, 33)]
    sc = np.array([limbs(int.from_bytes(rng.bytes(32), "little"), 4) for _ in range(33)], dtype=np.uint64)
    call = lambda p: cityprover.msm_g1(p, sc, xy)
    want = clean(call)
    assert want == O.bls_g1_msm(sc, xy)
    assert walk(call, want) >= 4   # three input copies and the workspace


def test_fr_ntt(setup_prover):
    import cityprover
    _, r, _ = O.bls_constants()
    rng = np.random.default_rng(5)
    a = np.array([limbs(int.from_bytes(rng.bytes(40), "little") % r, 4) for _ in range(32)], dtype=np.uint64)
    call = lambda p: (cityprover.fr_ntt(p, a).tobytes(), cityprover.fr_ntt(p, a, inverse=True, shift=7).tobytes())
    want = clean(call)
    assert want == (np.asarray(O.fr_ntt(a), dtype=np.uint64).tobytes(), np.asarray(O.fr_ntt(a, inverse=True, shift=7), dtype=np.uint64).tobytes())
    assert walk(call, want) >= 4   # the copy, the work array, a twiddle table, the coset powers


def test_r1cs_create_and_check(setup_prover):
    import cityprover
    s = RC.random_system(1, seed=1001)
    dw = setup_prover.to_device(RC.limbs4(s["w"]))

    def call(p):
        h = cityprover.R1cs(p, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"])
        try:
            return h.check(dw.ptr)
        finally:
            h.free()
    try:
        want = clean(call)
        bad = RC.violated_rows(s)
        assert want == (len(bad), bad[0] if bad else None)
        assert walk(call, want) >= 8   # eight arrays of the handle, then the counters
    finally:
        dw.free()


def test_groth16_prove(setup_prover):
    import cityprover as cp
    log_n, n_pub, n_in = 3, 2, 3
    _, r, G1 = O.bls_constants()
    G2 = O.bls_g2_generator()
    case = RC.groth16_case(log_n, n_pub, n_in)
    w, m = case["system"]["w"], case["system"]["n_wires"]
    g1_rows = lambda pts: np.array([limbs(P[0], 6) + limbs(P[1], 6) for P in pts], dtype=np.uint64)
    g2_words = lambda P: limbs(P[0][0], 6) + limbs(P[0][1], 6) + limbs(P[1][0], 6) + limbs(P[1][1], 6)
    pts1 = lambda logs: ([O.bls_g1_mul(G1, x) if x else G1 for x in logs], np.array([0 if x else 1 for x in logs], np.uint8))
    pa, a_inf = pts1(case["u"])
    pb1, b_inf = pts1(case["v"])
    pb2 = [O.bls_g2_mul(G2, x) if x else G2 for x in case["v"]]
    sp = setup_prover
    sets = [cp.G1Points(sp, g1_rows(pa)), cp.G1Points(sp, g1_rows(pb1)), cp.G2Points(sp, np.array([g2_words(P) for P in pb2], dtype=np.uint64)),
            cp.G1Points(sp, g1_rows(pts1(case["k_log"])[0])), cp.G1Points(sp, g1_rows(pts1(case["z_log"])[0]))]
    flags = lambda f: sp.to_device(np.frombuffer(np.concatenate([f, np.zeros(-len(f) % 8, np.uint8)]).tobytes(), np.uint64))
    to_dev = lambda vals: sp.to_device(np.array([limbs(x, 4) for x in vals], dtype=np.uint64))
    bufs = [flags(a_inf), flags(b_inf), to_dev(w)] + [to_dev(v) for v in case["evals"]]
    try:
        pk = cp.Groth16Pk()
        pk.n_wires, pk.n_private, pk.log_domain = m, m - n_pub, log_n
        pk.a_g1, pk.b_g1, pk.b_g2, pk.k_g1, pk.z_g1 = (x.buf.ptr for x in sets)
        pk.a_inf, pk.b_inf = bufs[0].ptr, bufs[1].ptr
        for name in ("alpha", "beta", "delta"):
            P = O.bls_g1_mul(G1, case[name])
            getattr(pk, name + "_g1")[:] = limbs(P[0], 6) + limbs(P[1], 6)
        for name in ("beta", "delta"):
            getattr(pk, name + "_g2")[:] = g2_words(O.bls_g2_mul(G2, case[name]))
        evals = [np.array([limbs(x, 4) for x in v], dtype=np.uint64) for v in case["evals"]]

        def call(p):
            for buf, v in zip(bufs[3:], evals):   # the quotient works in place on the three evaluation arrays: fresh ones for every call
                buf.upload(v)
            return cp.groth16_prove(p, pk, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, case["r"], case["s"])
        want = clean(call)
        assert want == (O.bls_g1_mul(G1, case["a_log"]), O.bls_g2_mul(G2, case["b_log"]), O.bls_g1_mul(G1, case["c_log"]))
        assert walk(call, want) >= 3   # the F_r work array, a twiddle table, the MSM workspace
    finally:
        for b in bufs:
            b.free()
        for x in sets:
            x.free()
