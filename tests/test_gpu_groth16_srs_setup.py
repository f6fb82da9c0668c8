"""cp_groth16_setup_srs_bls12381 against the trapdoor setup: for an SRS built from a known (tau, alpha, beta) the key must be,
byte for byte, the key cp_groth16_setup_bls12381 returns for (tau, alpha, beta, gamma = 1, delta = 1) - the setup that
tests/test_gpu_groth16_setup.py pins point by point against Python integers. The key then proves and verifies, goes through a
file, and every refusal leaves the context usable. The injected allocation failures are refused allocations that return a
status (the pattern of tests/test_gpu_alloc_faults.py): nothing here faults the device."""
import numpy as np
import pytest

import groth16_setup_cases as GC
import groth16_srs_cases as SC
import oracle_lib as O
import pairing_cases as PC
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


_arrays = {}


def arrays_of(prover, td, log_size):
    key = (td["tau"], td["alpha"], td["beta"], log_size)
    if key not in _arrays:
        _arrays[key] = SC.srs_arrays(prover, td, log_size)
    return _arrays[key]


def unit(td):
    return dict(td, gamma=1, delta=1)


def both_keys_equal(prover, case, log_size=None, ctx=None):
    """the SRS key and the trapdoor key of a case, as bytes; the SRS lives on `prover`, the setups run on `ctx`"""
    ctx = ctx or prover
    L = case["exp"]["log_domain"] if log_size is None else log_size
    srs = SC.make_srs(prover, arrays_of(prover, case["td"], L))
    try:
        key = SC.setup_srs(ctx, case, srs)
        try:
            got = SC.key_bytes(key)
        finally:
            key.free()
    finally:
        srs.free()
    ref = SC.setup_trapdoor(ctx, case, td=unit(case["td"]))
    try:
        want = SC.key_bytes(ref)
    finally:
        ref.free()
    assert got[1] == want[1]                      # the single points
    assert got[2] == want[2]                      # the verifying key, IC points and their flags included
    for name, a, b in zip(("a_g1", "b_g1", "b_g2", "k_g1", "z_g1", "a_inf", "b_inf"), got[0], want[0]):
        assert a == b, name
    return got


@pytest.mark.parametrize("name", ["2^3", "2^5", "2^8", "shapes"])
def test_the_key_is_the_trapdoor_key_byte_for_byte(prover, name):
    case = SC.case_of(name)
    if name == "shapes":
        # the case has what it says, before the device is asked: the workgroup-per-column form, both flag arrays, an infinite IC point
        s, exp, sp = case["system"], case["exp"], case["special"]
        assert s["n"] == 300 and exp["log_domain"] == 9 and len(exp["z"]) == 511
        a_col = np.bincount(s["mats"][0][1], minlength=s["n_wires"])
        assert a_col[0] == 300 > GC.LONG
        assert [int(a_col[w]) for w, _ in sp["a_columns"]] == [GC.LONG, GC.LONG + 1]
        assert exp["u"][sp["a_only"]] != 0 and exp["v"][sp["a_only"]] == 0
        assert exp["u"][sp["b_only"]] == 0 and exp["v"][sp["b_only"]] != 0
        assert exp["ic"][sp["unused_public"]] == 0 and all(exp["k"])
    got = both_keys_equal(prover, case)
    if name == "shapes":
        sp, m = case["special"], case["system"]["n_wires"]
        a_inf, b_inf = np.frombuffer(got[0][5], np.uint8), np.frombuffer(got[0][6], np.uint8)
        assert b_inf[sp["a_only"]] == 1 and a_inf[sp["b_only"]] == 1 and len(a_inf) == m


def two_constraints():
    """a b = c, c b = d by hand: a domain of two points (log_domain 1), one Z point"""
    a, b = 3, R - 5
    w = [1, a, b, a * b % R, a * b * b % R]
    system = RC.from_dict_rows([{1: 1}, {3: 2}], [{2: 1}, {2: 1, 0: 7}], [{3: 1}, {4: 2, 3: 14}], w)
    assert RC.eval_all(system)[0][1] * RC.eval_all(system)[1][1] % R == RC.eval_all(system)[2][1]
    td = GC.trapdoor(4242)
    return {"system": system, "n_pub": 2, "td": td, "exp": GC.expected_logs(system, 2, td), "special": {}}


def test_the_smallest_domain(prover):
    case = two_constraints()
    assert case["system"]["n"] == 2 and case["exp"]["log_domain"] == 1
    both_keys_equal(prover, case)


def test_an_srs_larger_than_the_domain_serves_it_by_its_prefix(prover):
    import cityprover as cp
    case = SC.case_of("2^3")
    assert both_keys_equal(prover, case, log_size=10) == both_keys_equal(prover, case, log_size=3)
    srs = SC.make_srs(prover, arrays_of(prover, case["td"], 2))
    try:
        with pytest.raises(cp.CityProverError, match=r"log_domain 3 exceeds the SRS's log_size 2"):
            SC.setup_srs(prover, case, srs)
    finally:
        srs.free()
    both_keys_equal(prover, case)


def proof_words(proof):
    a, b, c = proof
    return np.concatenate([PC.g1_words(a), PC.g2_words(b), PC.g1_words(c)])


def test_the_key_proves_and_its_proofs_verify(prover):
    import cityprover as cp
    case = SC.case_of("2^8")
    td, sysm, n_pub = unit(case["td"]), case["system"], case["n_pub"]
    exp = GC.expected_logs(sysm, n_pub, td)
    r, s = (x % R for x in GC.random_scalars(2, 88))
    a_log, b_log, c_log = GC.proof_logs(sysm, n_pub, td, exp, r, s)    # asserts the verification equation in the exponent
    G1, G2 = O.bls_constants()[2], O.bls_g2_generator()
    srs = SC.make_srs(prover, arrays_of(prover, case["td"], 8))
    key = SC.setup_srs(prover, case, srs)
    h = cp.R1cs(prover, sysm["n"], sysm["n_wires"], RC.limbs4(sysm["coeffs"]), sysm["mats"])
    dw = prover.to_device(RC.limbs4(sysm["w"]))
    ver = cp.Groth16Verifier.from_key(prover, key)
    try:
        proof = cp.groth16_prove_r1cs(prover, key.pk(), h, dw.ptr, r, s)
        assert proof == (O.bls_g1_mul(G1, a_log), O.bls_g2_mul(G2, b_log), O.bls_g1_mul(G1, c_log))
        pub = RC.limbs4(sysm["w"][1:n_pub])
        forged = (proof[0], proof[1], O.bls_g1_add(proof[2], G1))
        assert ver.verify(np.stack([proof_words(proof), proof_words(forged)]), np.stack([pub, pub])).tolist() == [0, 1]
    finally:
        ver.close()
        dw.free()
        h.free()
        key.free()
        srs.free()


def test_the_key_goes_through_a_file(prover, tmp_path):
    import cityprover as cp
    case = SC.case_of("2^5")
    srs = SC.make_srs(prover, arrays_of(prover, case["td"], 5))
    key = SC.setup_srs(prover, case, srs)
    try:
        path = str(tmp_path / "srs.key")
        key.save(path)
        loaded = cp.Groth16Key.load(prover, path, check_torsion=True)
        try:
            assert SC.key_bytes(loaded) == SC.key_bytes(key)
        finally:
            loaded.free()
    finally:
        key.free()
        srs.free()


def test_refusals_leave_the_context_usable(prover):
    import cityprover as cp
    case = SC.case_of("2^3")
    s, m = case["system"], case["system"]["n_wires"]
    good = arrays_of(prover, case["td"], 3)
    P = PC.P

    def edited(name, index, point_words):
        a = dict(good)
        a[name] = good[name].copy()
        a[name][index] = point_words
        return a
    off = good["tau_g1"][5].copy()
    y = sum(int(v) << (64 * j) for j, v in enumerate(off[6:]))
    off[6:] = PC.g1_words((0, (y + 1) % P))[6:]                                     # the same x, another canonical y: off the curve
    off2 = good["tau_g2"][2].copy()
    off2[0] ^= np.uint64(1)
    big = good["beta_tau_g1"][1].copy()
    big[:6] = PC.g1_words((P, 0))[:6]                                               # x = p: not canonical
    outside = PC.g1_words(PC.g1_outside_torsion())
    bad_srs = [(edited("tau_g1", 5, off), {}, r"SRS: tau_g1\[5\] is not on the curve"),
               (edited("tau_g2", 2, off2), {}, r"SRS: tau_g2\[2\] is not on the curve"),
               (edited("beta_tau_g1", 1, big), {}, r"SRS: beta_tau_g1\[1\]: coordinate is not canonical"),
               (edited("tau_g1", 0, good["tau_g1"][1]), {}, r"SRS: tau_g1\[0\] is not the standard generator"),
               (edited("tau_g2", 0, good["tau_g2"][1]), {}, r"SRS: tau_g2\[0\] is not the standard generator"),
               (edited("alpha_tau_g1", 3, outside), {"check_torsion": True}, r"SRS: alpha_tau_g1\[3\] is outside the r-torsion"),
               (good, {"flags": 2}, "SRS: unknown flags 0x2")]
    for arrays, kw, msg in bad_srs:
        with pytest.raises(cp.CityProverError, match=msg):
            SC.make_srs(prover, arrays, **kw)
        both_keys_equal(prover, case)                                              # the same context, straight afterwards
    SC.make_srs(prover, edited("alpha_tau_g1", 3, outside)).free()                 # on the curve: taken when the torsion is not asked for
    SC.make_srs(prover, good, check_torsion=True).free()                           # and the good SRS passes the torsion check
    unused = dict(s, n_wires=m + 1, w=s["w"] + [5])                                 # a private wire that no constraint names
    srs = SC.make_srs(prover, good)
    try:
        for kw, msg in (({"system": unused}, "setup: private wire %d occurs in no constraint: its key point would be the point at infinity" % m),
                        ({"n_pub": 0}, "n_public 0 out of range"), ({"n_pub": m + 1}, "n_public %d out of range" % (m + 1))):
            with pytest.raises(cp.CityProverError, match=msg):
                SC.setup_srs(prover, case, srs, **kw)
            with pytest.raises(cp.CityProverError, match=msg):                     # the trapdoor setup's words
                SC.setup_trapdoor(prover, case, **kw)
            both_keys_equal(prover, case)
    finally:
        srs.free()


def test_injected_allocation_failures(prover):
    """cp_fault_inject(CP_FAULT_DEVMEM, j) for every j until the SRS setup gets through: out of memory, no handle, nothing held,
    and the same context then makes exactly the key of the trapdoor setup"""
    import cityprover as cp
    lib = cp.load_library()
    case = SC.case_of("2^3")
    want = both_keys_equal(prover, case)
    srs = SC.make_srs(prover, arrays_of(prover, case["td"], 3))
    refused = 0
    try:
        for j in range(MAX_WALK):
            p = cp.Prover(0)
            try:
                cp.batch_pool_trim(p)
                held = cp.batch_pool_stats(0)["bytes"]
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    key = SC.setup_srs(p, case, srs)
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert "out of memory" in str(e), (j, str(e))          # alloc_status: the text of CP_ERR_OOM
                    assert cp.batch_pool_stats(0)["bytes"] == held, j
                    refused += 1
                    key = SC.setup_srs(p, case, srs)
                    try:
                        assert SC.key_bytes(key) == want, "allocation %d refused: the context did not recover" % j
                    finally:
                        key.free()
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                try:
                    assert SC.key_bytes(key) == want
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
        srs.free()
    # groth16_setup_srs_run on a fresh context: the transposed system's seventeen arrays (three row_ptr / terms pairs, for each
    # of the three jobs its long wires, their chunk ranges and the chunks, the chunk sums, the coefficients), the eight Lagrange
    # arrays (points and flags, four times), the key's seven arrays and the four temporaries behind them (the K / IC points and
    # flags, the Z flags, the flag slot) are 36 sites; the work array and the twiddle table of the transforms come on top. The
    # walk bound leaves room for more than twice that.
    assert refused >= 36


def test_the_key_and_the_srs_outlive_their_context():
    import cityprover as cp
    case = SC.case_of("2^3")
    p = cp.Prover(0)
    srs = SC.make_srs(p, arrays_of(p, case["td"], 3))
    key = SC.setup_srs(p, case, srs)
    p.close()
    key.free()
    key.free()      # and a second free does nothing
    srs.free()
    srs.free()
