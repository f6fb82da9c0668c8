"""cp_groth16_setup_bls12381 against the trapdoor: every point of the key is compared with [its logarithm] G, the logarithms
computed term by term in Python integers (tests/groth16_setup_cases.py) and the points by the oracle's scalar multiplication;
the key is then used by the two existing provers, whose proofs are compared with the trapdoor logarithms of (A, B, C) - which
satisfy the verification equation in the exponent with the IC logarithms and gamma. Everything is compared for equality.
The injected allocation failures are refused allocations that return a status (the pattern of tests/test_gpu_alloc_faults.py):
nothing here faults the device."""
import numpy as np
import pytest

import groth16_setup_cases as GC
import oracle_lib as O
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
R = GC.R
DEVMEM = 3   # CP_FAULT_DEVMEM
MAX_WALK = 96


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def gens():
    return O.bls_constants()[2], O.bls_g2_generator()


def setup(prover, case, n_pub=None, td=None, system=None):
    import cityprover as cp
    s = system or case["system"]
    return cp.Groth16Key.setup(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], case["n_pub"] if n_pub is None else n_pub,
                               **(td or case["td"]))


def g1(log):
    return O.bls_g1_mul(gens()[0], log)


def g2(log):
    return O.bls_g2_mul(gens()[1], log)


def check_set(points, flags, logs, mul, gen, index=None):
    """points[i] = [logs[i]] gen; where the logarithm is zero the flag is set (if the set has flags) and the entry is the generator"""
    index = range(len(logs)) if index is None else index
    got = points.to_host(list(index))
    for i, P in zip(index, got):
        if logs[i] == 0:
            assert flags is not None and flags[i] == 1, i
            assert P == gen, i
        else:
            assert flags is None or flags[i] == 0, i
            assert P == mul(gen, logs[i]), i


def check_single_points(key, case):
    td, exp = case["td"], case["exp"]
    pk, vk = key.pk(), key.vk()
    val = lambda a: sum(int(v) << (64 * j) for j, v in enumerate(a))
    p1 = lambda a: (val(a[0:6]), val(a[6:12]))
    p2 = lambda a: ((val(a[0:6]), val(a[6:12])), (val(a[12:18]), val(a[18:24])))
    assert p1(pk.alpha_g1) == g1(td["alpha"]) == vk["alpha_g1"]
    assert p1(pk.beta_g1) == g1(td["beta"])
    assert p1(pk.delta_g1) == g1(td["delta"])
    assert p2(pk.beta_g2) == g2(td["beta"]) == vk["beta_g2"]
    assert p2(pk.delta_g2) == g2(td["delta"]) == vk["delta_g2"]
    assert vk["gamma_g2"] == g2(td["gamma"])
    s = case["system"]
    assert (pk.n_wires, pk.n_private, pk.log_domain, vk["n_public"]) == (s["n_wires"], s["n_wires"] - case["n_pub"], exp["log_domain"], case["n_pub"])
    assert vk["ic"] == [g1(x) if x else None for x in exp["ic"]]


def check_whole_key(key, case):
    exp = case["exp"]
    G1, G2 = gens()
    sets = key.point_sets()
    assert sets["a_inf"].tolist() == [int(x == 0) for x in exp["u"]]
    assert sets["b_inf"].tolist() == [int(x == 0) for x in exp["v"]]
    check_set(sets["a_g1"], sets["a_inf"], exp["u"], O.bls_g1_mul, G1)
    check_set(sets["b_g1"], sets["b_inf"], exp["v"], O.bls_g1_mul, G1)
    check_set(sets["b_g2"], sets["b_inf"], exp["v"], O.bls_g2_mul, G2)
    check_set(sets["k_g1"], None, exp["k"], O.bls_g1_mul, G1)
    check_set(sets["z_g1"], None, exp["z"], O.bls_g1_mul, G1)
    assert sets["z_g1"].n == (1 << exp["log_domain"]) - 1
    check_single_points(key, case)


_cases = {}


def case_of(name):
    if name not in _cases:
        if name == "shapes":
            # 300 constraints (a domain of 2^9: padded rows, 511 Z points); wire 0 in all 300 rows of A: a column above the long-row
            # threshold of the transposed product; columns of exactly the threshold and one more; wires in A only / B only; a
            # public wire that occurs nowhere
            c = GC.small_case(300, 3, 5, 300, wire0_in_every_a_row=True, a_columns=(GC.LONG, GC.LONG + 1), a_only=True, b_only=True, unused_public=True)
        elif name == "sat12":
            c = GC.satisfied_case(1 << 12, 4012, 4)
        else:
            n, n_pub, n_in = {"2^3": (8, 3, 3), "2^5": (32, 3, 6), "2^8": (256, 2, 5)}[name]
            c = GC.small_case(n, n_pub, n_in, 100 + n)
        _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("name", ["2^3", "2^5", "2^8"])
def test_every_point_of_the_key(prover, name):
    case = case_of(name)
    key = setup(prover, case)
    try:
        check_whole_key(key, case)
    finally:
        key.free()


def test_every_point_of_the_key_on_the_shapes_that_take_other_paths(prover):
    case = case_of("shapes")
    s, exp, sp = case["system"], case["exp"], case["special"]
    # the case has what it says, before the device is asked
    assert s["n"] == 300 and exp["log_domain"] == 9 and len(exp["z"]) == 511
    a_col = np.bincount(s["mats"][0][1], minlength=s["n_wires"])
    assert a_col[0] == 300 > GC.LONG
    assert [int(a_col[w]) for w, _ in sp["a_columns"]] == [GC.LONG, GC.LONG + 1]
    assert exp["u"][sp["a_only"]] != 0 and exp["v"][sp["a_only"]] == 0
    assert exp["u"][sp["b_only"]] == 0 and exp["v"][sp["b_only"]] != 0
    assert exp["ic"][sp["unused_public"]] == 0 and all(exp["k"])
    key = setup(prover, case)
    try:
        check_whole_key(key, case)
        sets = key.point_sets()
        assert sets["b_inf"][sp["a_only"]] == 1 and sets["a_inf"][sp["b_only"]] == 1
        assert key.vk()["ic"][sp["unused_public"]] is None
    finally:
        key.free()


def prove_both_ways(prover, key, case, r, s):
    """(proof through cp_groth16_prove_r1cs_bls12381, proof through cp_groth16_prove_bls12381 with host-computed evaluations)"""
    import cityprover as cp
    sysm = case["system"]
    N = 1 << case["exp"]["log_domain"]
    h = cp.R1cs(prover, sysm["n"], sysm["n_wires"], RC.limbs4(sysm["coeffs"]), sysm["mats"])
    dw = prover.to_device(RC.limbs4(sysm["w"]))
    ev = [prover.to_device(RC.limbs4(col + [0] * (N - len(col)))) for col in RC.eval_all(sysm)]
    try:
        pk = key.pk()
        return (cp.groth16_prove_r1cs(prover, pk, h, dw.ptr, r, s), cp.groth16_prove(prover, pk, dw.ptr, ev[0].ptr, ev[1].ptr, ev[2].ptr, r, s))
    finally:
        for b in [dw] + ev:
            b.free()
        h.free()


def test_the_key_proves_with_the_existing_provers(prover):
    case = case_of("2^8")
    r, s = GC.random_scalars(2, 88)
    r, s = r % R, s % R
    a_log, b_log, c_log = GC.proof_logs(case["system"], case["n_pub"], case["td"], case["exp"], r, s)   # asserts the verification equation
    key = setup(prover, case)
    try:
        from_witness, from_evals = prove_both_ways(prover, key, case, r, s)
    finally:
        key.free()
    assert from_witness == (g1(a_log), g2(b_log), g1(c_log))
    assert from_evals == from_witness


def test_a_key_with_real_infinity_patterns_at_2_12(prover):
    """r1cs_cases.satisfied_system at 2^12 constraints: long rows and columns, and a B query in which many wires do not occur"""
    case = case_of("sat12")
    exp, m = case["exp"], case["system"]["n_wires"]
    flagged_b = [i for i, x in enumerate(exp["v"]) if x == 0]
    assert len(flagged_b) > 0, "the generator must leave wires out of B: the test would pass on a key without infinities"
    assert all(exp["k"])
    G1, G2 = gens()
    key = setup(prover, case)
    try:
        sets = key.point_sets()
        assert sets["a_inf"].tolist() == [int(x == 0) for x in exp["u"]]          # all wires
        assert sets["b_inf"].tolist() == [int(x == 0) for x in exp["v"]]
        rng = np.random.default_rng(12)

        def sample(logs):
            pick = set(rng.choice(len(logs), size=min(256, len(logs)), replace=False).tolist()) | {0, len(logs) - 1}
            return sorted(pick | {i for i, x in enumerate(logs) if x == 0})
        check_set(sets["a_g1"], sets["a_inf"], exp["u"], O.bls_g1_mul, G1, sample(exp["u"]))
        check_set(sets["b_g1"], sets["b_inf"], exp["v"], O.bls_g1_mul, G1, sample(exp["v"]))
        check_set(sets["b_g2"], sets["b_inf"], exp["v"], O.bls_g2_mul, G2, sample(exp["v"]))
        check_set(sets["k_g1"], None, exp["k"], O.bls_g1_mul, G1, sample(exp["k"]))
        check_set(sets["z_g1"], None, exp["z"], O.bls_g1_mul, G1, sample(exp["z"]))
        check_single_points(key, case)
        import cityprover as cp
        r, s = (x % R for x in GC.random_scalars(2, 89))
        a_log, b_log, c_log = GC.proof_logs(case["system"], case["n_pub"], case["td"], exp, r, s)
        sysm = case["system"]
        h = cp.R1cs(prover, sysm["n"], m, RC.limbs4(sysm["coeffs"]), sysm["mats"])
        dw = prover.to_device(RC.limbs4(sysm["w"]))
        try:
            assert cp.groth16_prove_r1cs(prover, key.pk(), h, dw.ptr, r, s) == (g1(a_log), g2(b_log), g1(c_log))
        finally:
            dw.free()
            h.free()
    finally:
        key.free()


def test_refusals_leave_the_context_usable(prover):
    import cityprover as cp
    case = case_of("2^3")
    s, td = case["system"], case["td"]
    m = s["n_wires"]
    omega = pow(7, (R - 1) >> case["exp"]["log_domain"], R)
    unused = dict(s, n_wires=m + 1, w=s["w"] + [5])                         # a private wire that no constraint names
    bad_col = [tuple(a.copy() for a in mat) for mat in s["mats"]]
    bad_col[1][1][0] = m                                                   # B names a wire that does not exist
    refused = [(dict(td, tau=0), {}, "tau is zero"), (dict(td, delta=0), {}, "delta is zero"), (dict(td, alpha=R), {}, r"alpha is not canonical"),
               (dict(td, gamma=2**256 - 1), {}, "gamma is not canonical"), (dict(td, tau=omega), {}, r"tau\^\(2\^3\) = 1"),
               (td, {"n_pub": 0}, "n_public 0 out of range"), (td, {"n_pub": m + 1}, "n_public %d out of range" % (m + 1)),
               (td, {"system": unused}, "private wire %d " % m), (td, {"system": dict(s, mats=bad_col)}, "R1CS matrix B row 0: wire %d >= n_wires %d" % (m, m))]
    for td_, kw, msg in refused:
        with pytest.raises(cp.CityProverError, match=msg):
            setup(prover, case, td=td_, **kw)
        key = setup(prover, case)                                          # the same context, straight afterwards
        try:
            check_single_points(key, case)
        finally:
            key.free()
    key = setup(prover, case)
    try:
        check_whole_key(key, case)
    finally:
        key.free()


def key_bytes(key):
    """everything the key holds, as bytes: two keys of the same setup are equal exactly when these are"""
    pk, sets = key.pk(), key.point_sets()
    vk = key.vk()
    raw = [sets[k].buf.download().tobytes() for k in ("a_g1", "b_g1", "b_g2", "k_g1", "z_g1")] + [sets["a_inf"].tobytes(), sets["b_inf"].tobytes()]
    singles = [bytes(bytearray(getattr(pk, f))) for f in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")]
    return raw, singles, repr(vk)


def test_injected_allocation_failures(prover):
    """cp_fault_inject(CP_FAULT_DEVMEM, j) for every j until the setup gets through: out of memory, no handle, nothing held, and
    the same context then makes exactly the key that was checked point by point"""
    import cityprover as cp
    lib = cp.load_library()
    case = case_of("2^3")
    key = setup(prover, case)
    try:
        check_whole_key(key, case)
        want = key_bytes(key)
    finally:
        key.free()
    refused = 0
    try:
        for j in range(MAX_WALK):
            p = cp.Prover(0)
            try:
                cp.batch_pool_trim(p)
                held = cp.batch_pool_stats(0)["bytes"]
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    key = setup(p, case)
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert "out of memory" in str(e), (j, str(e))          # alloc_status: the text of CP_ERR_OOM
                    assert cp.batch_pool_stats(0)["bytes"] == held, j
                    refused += 1
                    key = setup(p, case)
                    try:
                        assert key_bytes(key) == want, "allocation %d refused: the context did not recover" % j
                    finally:
                        key.free()
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                try:
                    assert key_bytes(key) == want
                finally:
                    key.free()
                break
            finally:
                lib.cp_fault_inject(DEVMEM, -1)
                p.close()
        else:
            pytest.fail("the walk did not end before j = %d" % MAX_WALK)
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    assert refused >= 20   # the transposed system's eight arrays, the temporaries, two tables, the key's seven arrays at the least


def test_a_key_outlives_its_context():
    import cityprover as cp
    case = case_of("2^3")
    p = cp.Prover(0)
    key = setup(p, case)
    p.close()
    key.free()
    key.free()      # and a second free does nothing
