"""Phase 1 of the Groth16 ceremony on the device: cp_groth16_srs_unit / _contribute / _points / _check.
unit(L).contribute(t, a, b).points() must be, word for word, the SRS tests/groth16_srs_cases.py builds from fixed-base multiples
(the path tests/test_gpu_fixed_base.py pins against the oracle); contributions compose; the arrays read back make the key of
the trapdoor setup; check() accepts every SRS made here and gives each spoiled one - edited on the host, so that it still passes
the per-point checks of srs_create - the verdict of the first equation it breaks. The injected allocation failures are refused
allocations that return a status (the pattern of tests/test_gpu_alloc_faults.py): nothing here faults the device."""
import ctypes

import numpy as np
import pytest

import groth16_setup_cases as GC
import groth16_srs_cases as SC
import oracle_lib as O
import pairing_cases as PC

pytestmark = pytest.mark.gpu
R = GC.R
DEVMEM = 3   # CP_FAULT_DEVMEM
MAX_WALK = 96
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")
u64p = ctypes.POINTER(ctypes.c_uint64)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def tab(seed):
    td = GC.trapdoor(seed)
    return td["tau"], td["alpha"], td["beta"]


def weights(log_size, seed):
    """5 n - 5 non-zero 128-bit values"""
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(16), "little") | 1 for _ in range(5 * (1 << log_size) - 5)]


_made = {}


def made(prover, log_size, scalars):
    """unit(L).contribute(t, a, b) read back, once per (L, t, a, b): the host arrays (never edited in place)"""
    import cityprover as cp
    key = (log_size,) + tuple(scalars)
    if key not in _made:
        unit = cp.Groth16Srs.unit(prover, log_size)
        try:
            srs = unit.contribute(*scalars)
            try:
                _made[key] = srs.points()
            finally:
                srs.free()
        finally:
            unit.free()
    return _made[key]


def same_arrays(got, want):
    assert got["log_size"] == want["log_size"]
    for name in ARRAYS:
        assert got[name].shape == want[name].shape, name
        assert got[name].tobytes() == want[name].tobytes(), name


def verdict_of(prover, arrays, seed=7, **kw):
    srs = SC.make_srs(prover, arrays, **kw)
    try:
        return srs.check(weights(arrays["log_size"], seed))
    finally:
        srs.free()


def g1_ints(words):
    return (O._int(words[:6]), O._int(words[6:]))


@pytest.mark.parametrize("log_size", [1, 3, 6])
def test_generation_is_byte_exact_and_consistent(prover, log_size):
    """L = 6: 127 points of tau_g1 across the 64- and 128-lane boundaries, 31 + 3 points in the last lane groups of k_finish;
    L = 1 is the smallest SRS: 3 / 2 / 2 / 2 points and 5 weights"""
    import cityprover as cp
    t, a, b = tab(1000 + log_size)
    got = made(prover, log_size, (t, a, b))
    n = 1 << log_size
    assert got["tau_g1"].shape == (2 * n - 1, 12) and got["tau_g2"].shape == (n, 24) and got["beta_g2"].shape == (24,)
    same_arrays(got, SC.srs_arrays(prover, {"tau": t, "alpha": a, "beta": b}, log_size))
    assert len(weights(log_size, 1)) == 5 * n - 5
    unit = cp.Groth16Srs.unit(prover, log_size)
    try:
        srs = unit.contribute(t, a, b)
        try:
            for seed in (1, 2):
                verdict, why = srs.check(weights(log_size, seed))
                assert verdict == 0, why
                assert "verdict 0" in why
            verdict, why = srs.check(np.array([[w & (2**64 - 1), w >> 64] for w in weights(log_size, 3)], np.uint64))
            assert verdict == 0, why
        finally:
            srs.free()
        verdict, why = unit.check(weights(log_size, 4))      # the unit SRS is consistent (and worthless)
        assert verdict == 0, why
    finally:
        unit.free()


def test_the_unit_srs_is_the_generators(prover):
    import cityprover as cp
    unit = cp.Groth16Srs.unit(prover, 2)
    try:
        pts = unit.points()
    finally:
        unit.free()
    G1, G2 = PC.g1_words(O.bls_constants()[2]), PC.g2_words(O.bls_g2_generator())
    assert pts["log_size"] == 2
    for name, rows, g in (("tau_g1", 7, G1), ("alpha_tau_g1", 4, G1), ("beta_tau_g1", 4, G1), ("tau_g2", 4, G2)):
        assert pts[name].shape == (rows, len(g)) and (pts[name] == g).all(), name
    assert (pts["beta_g2"] == G2).all()


def test_contributions_compose_and_leave_their_input_alone(prover):
    import cityprover as cp
    s1, s2, _ = tab(77)
    first, second = (s1, R - 1, 1), (R - 1, 1, s2)
    product = tuple(x * y % R for x, y in zip(first, second))
    assert product == (R - s1, R - 1, s2)
    unit = cp.Groth16Srs.unit(prover, 3)
    try:
        one = unit.contribute(*first)
        try:
            before = one.points()
            two = one.contribute(*second)
            try:
                got = two.points()
                verdict, why = two.check(weights(3, 5))
                assert verdict == 0, why
            finally:
                two.free()
            same_arrays(one.points(), before)                           # the input is unchanged
            same_arrays(before, made(prover, 3, first))
        finally:
            one.free()
        same_arrays(got, made(prover, 3, product))
        same_arrays(got, SC.srs_arrays(prover, dict(zip(("tau", "alpha", "beta"), product)), 3))
        # times 1 and times -1, fully reduced: (1, 1, 1) is the unit SRS again, (-1)(-1) too
        ident = unit.contribute(1, 1, 1)
        try:
            same_arrays(ident.points(), unit.points())
        finally:
            ident.free()
        neg = unit.contribute(R - 1, R - 1, R - 1)
        try:
            back = neg.contribute(R - 1, R - 1, R - 1)
            try:
                same_arrays(back.points(), unit.points())            # every entry the generator again
            finally:
                back.free()
        finally:
            neg.free()
    finally:
        unit.free()


def test_points_go_back_through_create_and_make_the_trapdoor_key(prover):
    case = SC.case_of("2^3")
    td = case["td"]
    arrays = made(prover, 3, (td["tau"], td["alpha"], td["beta"]))
    srs = SC.make_srs(prover, arrays, check_torsion=True)
    try:
        verdict, why = srs.check(weights(3, 6))
        assert verdict == 0, why
        key = SC.setup_srs(prover, case, srs)
        try:
            got = SC.key_bytes(key)
        finally:
            key.free()
    finally:
        srs.free()
    ref = SC.setup_trapdoor(prover, case, td=dict(td, gamma=1, delta=1))
    try:
        assert got == SC.key_bytes(ref)
    finally:
        ref.free()


def edited(good, name, index, point_words):
    a = dict(good)
    a[name] = good[name].copy()
    if index is None:
        a[name][:] = point_words
    else:
        a[name][index] = point_words
    return a


EQUATION = {1: "e(H(tau_g1), G2) != e(L(tau_g1), tau_g2[1])", 2: "e(tau_g1[1], L(tau_g2)) != e(G1, H(tau_g2))",
            3: "e(H(alpha_tau_g1), G2) != e(L(alpha_tau_g1), tau_g2[1])", 4: "e(H(beta_tau_g1), G2) != e(L(beta_tau_g1), tau_g2[1])",
            5: "e(beta_tau_g1[0], G2) != e(G1, beta_g2)"}


def test_every_verdict_of_the_check(prover):
    """the spoiled arrays pass srs_create's per-point checks (torsion included): only the check tells"""
    t, a, b = tab(2024)
    good = made(prover, 3, (t, a, b))
    other = made(prover, 3, tab(2025))
    n = 8
    cases = []
    for k in (1, 7, 2 * n - 2):
        doubled = PC.g1_words(O.bls_g1_mul(g1_ints(good["tau_g1"][k]), 2))
        cases.append((edited(good, "tau_g1", k, doubled), 1, "tau_g1[%d] doubled" % k))
    swapped = edited(good, "tau_g1", 4, good["tau_g1"][5])
    swapped["tau_g1"][5] = good["tau_g1"][4]
    cases.append((swapped, 1, "tau_g1[4] and [5] swapped"))
    cases.append((edited(good, "tau_g2", 1, other["tau_g2"][1]), 1, "tau_g2[1]: row 1 reads it and comes first"))
    cases.append((edited(good, "tau_g2", n - 1, other["tau_g2"][n - 1]), 2, "tau_g2[n - 1]"))
    cases.append((edited(good, "tau_g2", 2, other["tau_g2"][2]), 2, "tau_g2[2]"))
    cases.append((edited(good, "alpha_tau_g1", 3, other["alpha_tau_g1"][3]), 3, "alpha_tau_g1[3]"))
    cases.append((edited(good, "beta_tau_g1", n - 1, other["beta_tau_g1"][n - 1]), 4, "beta_tau_g1[n - 1]"))
    cases.append((edited(good, "beta_g2", None, other["beta_g2"]), 5, "beta_g2"))
    for arrays, want, what in cases:
        verdict, why = verdict_of(prover, arrays, check_torsion=True)
        assert verdict == want, (what, why)
        assert "verdict %d" % want in why and EQUATION[want] in why, (what, why)
    verdict, why = verdict_of(prover, good, check_torsion=True)
    assert verdict == 0, why


def test_a_point_outside_the_torsion_is_verdict_6(prover):
    import cityprover as cp
    t, a, b = tab(2024)
    good = made(prover, 3, (t, a, b))
    X = PC.g1_outside_torsion()
    arrays = edited(good, "tau_g1", 3, PC.g1_words(X))
    with pytest.raises(cp.CityProverError, match=r"SRS: tau_g1\[3\] is outside the r-torsion"):
        SC.make_srs(prover, arrays, check_torsion=True)
    srs = SC.make_srs(prover, arrays)                  # on the curve: taken when the torsion is not asked for
    try:
        verdict, why = srs.check(weights(3, 8))
        assert verdict == 6, why
        assert "outside the r-torsion" in why and "CP_GROTH16_SRS_CHECK_TORSION" in why
        t2, a2, b2 = tab(31)
        if O.bls_g1_mul(X, pow(t2, 3, R)) is None:     # what the order of X dictates for the scalar t2^3 mod r
            with pytest.raises(cp.CityProverError, match=r"SRS contribution: tau_g1\[3\] times its scalar is the point at infinity"):
                srs.contribute(t2, a2, b2)
        else:
            out = srs.contribute(t2, a2, b2)
            try:
                assert g1_ints(out.points()["tau_g1"][3]) == O.bls_g1_mul(X, pow(t2, 3, R))
            finally:
                out.free()
    finally:
        srs.free()


def test_refusals_leave_the_context_usable(prover):
    import cityprover as cp
    lib = cp.load_library()
    scalars = tab(2024)
    good = made(prover, 3, scalars)
    for L in (0, 29):
        with pytest.raises(cp.CityProverError, match=r"SRS: log_size %d out of range \(1 \.\. 28\)" % L):
            cp.Groth16Srs.unit(prover, L)
    unit = cp.Groth16Srs.unit(prover, 3)
    try:
        count = 5 * 8 - 5
        for i in (0, 17, count - 1):
            w = weights(3, 9)
            w[i] = 0
            with pytest.raises(cp.CityProverError, match=r"SRS check: weight %d is zero" % i):
                unit.check(w)
        with pytest.raises(cp.CityProverError, match="SRS check: weights is NULL"):
            unit.check(None)
        w = np.array([[1, 0]] * count, np.uint64)
        assert lib.cp_groth16_srs_check_bls12381(prover.ctx, unit.handle, w.ctypes.data_as(u64p), None) != 0
        assert b"NULL argument" in lib.cp_last_error(prover.ctx)
        verdict = ctypes.c_int(9)
        assert lib.cp_groth16_srs_check_bls12381(prover.ctx, None, w.ctypes.data_as(u64p), ctypes.byref(verdict)) != 0
        assert verdict.value == 9
        for bad, name, what in ((0, "t", "zero"), (R, "t", "not canonical"), (0, "a", "zero"), (R + 5, "a", "not canonical"), (0, "b", "zero"),
                                (2**256 - 1, "b", "not canonical")):
            s = {"t": 2, "a": 3, "b": 5}
            s[name] = bad
            with pytest.raises(cp.CityProverError, match=r"SRS contribution: %s is %s" % (name, what)):
                unit.contribute(s["t"], s["a"], s["b"])
        limbs = [np.array([(v >> (64 * j)) & (2**64 - 1) for j in range(4)], np.uint64) for v in (0, 3, 5)]
        out = ctypes.c_void_p(77)
        assert lib.cp_groth16_srs_contribute_bls12381(prover.ctx, unit.handle, *(x.ctypes.data_as(u64p) for x in limbs), ctypes.byref(out)) != 0
        assert out.value is None                                    # *srs_out is left NULL
        assert lib.cp_groth16_srs_contribute_bls12381(prover.ctx, unit.handle, None, limbs[1].ctypes.data_as(u64p), limbs[2].ctypes.data_as(u64p), ctypes.byref(out)) != 0
        assert b"NULL argument" in lib.cp_last_error(prover.ctx)
        assert lib.cp_groth16_srs_points_bls12381(prover.ctx, None, None, None, None, None, None, None) != 0
        srs = unit.contribute(*scalars)                             # the same context, straight afterwards
        try:
            same_arrays(srs.points(), good)
        finally:
            srs.free()
    finally:
        unit.free()


def walk(lib, cp, call, same):
    """cp_fault_inject(CP_FAULT_DEVMEM, j) for every j until call(p) gets through on a fresh context p: each refusal is out of
    memory, leaves the pool's bytes alone, and the same context then gives the same result. Returns the number of refusals."""
    refused = 0
    try:
        for j in range(MAX_WALK):
            p = cp.Prover(0)
            try:
                cp.batch_pool_trim(p)
                held = cp.batch_pool_stats(0)["bytes"]
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    got = call(p)
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert "out of memory" in str(e), (j, str(e))
                    assert cp.batch_pool_stats(0)["bytes"] == held, j
                    refused += 1
                    same(call(p), "allocation %d refused: the context did not recover" % j)
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                same(got, "no allocation refused")
                return refused
            finally:
                lib.cp_fault_inject(DEVMEM, -1)
                p.close()
        pytest.fail("the walk did not end before j = %d" % MAX_WALK)
    finally:
        lib.cp_fault_inject(DEVMEM, -1)


def test_injected_allocation_failures(prover):
    import cityprover as cp
    lib = cp.load_library()
    scalars = tab(2024)
    good = made(prover, 3, scalars)
    unit = cp.Groth16Srs.unit(prover, 3)
    srs = unit.contribute(*scalars)
    unit_pts = unit.points()
    w = weights(3, 10)

    def arrays_equal(want):
        def same(got, msg):
            for name in ARRAYS:
                assert got[name].tobytes() == want[name].tobytes(), (msg, name)
        return same

    def handle_equal(want):                   # walk() hands the new SRS over with the injection disarmed: read it back on `prover`
        def same(s, msg):
            try:
                arrays_equal(want)(s.points(prover), msg)
            finally:
                s.free()
        return same

    def verdict_zero(got, msg):
        assert got[0] == 0, (msg, got)

    try:
        # unit: the four arrays. contribute: the powers, the flags, the flag slot, the work array and the four arrays.
        # points: a staging buffer per array. check: the scalars, the workspace of the MSMs, the buffers of the pairing call.
        assert walk(lib, cp, lambda p: cp.Groth16Srs.unit(p, 3), handle_equal(unit_pts)) >= 4
        assert walk(lib, cp, lambda p: unit.contribute(*scalars, prover=p), handle_equal(good)) >= 8
        assert walk(lib, cp, lambda p: srs.points(p), arrays_equal(good)) >= 4
        assert walk(lib, cp, lambda p: srs.check(w, prover=p), verdict_zero) >= 3
    finally:
        srs.free()
        unit.free()


def test_an_srs_made_here_outlives_its_context():
    import cityprover as cp
    p = cp.Prover(0)
    unit = cp.Groth16Srs.unit(p, 1)
    srs = unit.contribute(2, 3, 5)
    p.close()
    srs.free()
    srs.free()      # and a second free does nothing
    unit.free()
