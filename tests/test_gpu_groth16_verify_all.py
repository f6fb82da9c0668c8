"""cp_groth16_verify_all_bls12381 and cp_groth16_verify_all_city_bls12381: a batch of Groth16 proofs under one final
exponentiation. The keys and proofs are made as in tests/test_gpu_groth16_verify.py: a tiny system of
tests/groth16_setup_cases.py, cp_groth16_setup_bls12381, eight distinct proofs of cp_groth16_prove_r1cs_bls12381 (eight
blindings), repeated to fill a batch; n_public 1, 2 and 3. The oracle of every verdict array is the per-proof function
cp_groth16_verify_bls12381 on the same input. The weights come from a seeded generator so that a failure can be repeated: a
caller draws them from a cryptographic one. The injected allocation failures are refused allocations that return a status (the
pattern of tests/test_gpu_alloc_faults.py): nothing here faults the device."""
import ctypes

import numpy as np
import pytest

import groth16_setup_cases as GC
import oracle_lib as O
import pairing_cases as PC
import pairing_ref as PR
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
P, R = PR.P, PR.R
DEVMEM = 3   # CP_FAULT_DEVMEM
MAX_WALK = 32
SIZES = (1, 2, 3, 5, 64, 65, 127, 129)   # one lane, odd counts at each round of the product tree (n + 3 values), both sides of a wavefront
u64p, u8p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    for m in _made.values():
        m["verifier"].close()
        m["key"].free()
    _made.clear()
    p.close()


def proof_words(A, B, Cc):
    return np.concatenate([PC.g1_words(A), PC.g2_words(B), PC.g1_words(Cc)])


def publics_words(xs):
    return np.array([[(x >> (64 * j)) & PC.MASK for j in range(4)] for x in xs], np.uint64).reshape(len(xs), 4)


_made = {}


def made(prover, n_pub):
    """case, key, verifier and eight distinct proofs of the one witness, once per module"""
    import cityprover as cp
    if n_pub not in _made:
        case = GC.small_case(8, n_pub, 3, 8100 + n_pub)
        s = case["system"]
        key = cp.Groth16Key.setup(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], n_pub, **case["td"])
        h = cp.R1cs(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"])
        dw = prover.to_device(RC.limbs4(s["w"]))
        try:
            blind = [x % R for x in GC.random_scalars(16, 8200 + n_pub)]
            proofs = [cp.groth16_prove_r1cs(prover, key.pk(), h, dw.ptr, blind[2 * i], blind[2 * i + 1]) for i in range(8)]
        finally:
            dw.free()
            h.free()
        assert len({p[0] for p in proofs}) == 8 and len({p[2] for p in proofs}) == 8
        _made[n_pub] = {"key": key, "verifier": cp.Groth16Verifier.from_key(prover, key), "proofs": proofs, "n_pub": n_pub,
                        "pub": [int(x) for x in s["w"][1:n_pub]]}
    return _made[n_pub]


def batch(m, n):
    """n proofs (the eight, repeated) and their public inputs: lists, for a test to alter"""
    return [m["proofs"][i % 8] for i in range(n)], [list(m["pub"]) for _ in range(n)]


def arrays(m, proofs, pubs):
    return np.stack([proof_words(*p) for p in proofs]), (np.stack([publics_words(x) for x in pubs]) if m["n_pub"] > 1 else None)


def weights(n, seed):
    """n distinct non-zero 128-bit values"""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        out.add(int.from_bytes(rng.bytes(16), "little") | 1)
    return sorted(out, key=lambda w: w % 1000003)


# ---- valid batches ----
@pytest.mark.parametrize("n_pub", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_valid_batches_take_the_aggregated_path(prover, n, n_pub):
    import cityprover as cp
    m = made(prover, n_pub)
    proofs, pubs = batch(m, n)
    words, pw = arrays(m, proofs, pubs)
    w = weights(n, 100 * n + n_pub)
    flags = cp.PAIRING_TRUSTED if n % 2 == 0 else 0         # both settings over the sizes
    got, path = m["verifier"].verify_all(words, w, pw, flags=flags)
    assert (got.tolist(), path) == ([0] * n, 0)
    blobs = [cp.groth16_pack_city(*p) for p in proofs]
    got, path = m["verifier"].verify_all_city(blobs, w, pw, flags=flags)
    assert (got.tolist(), path) == ([0] * n, 0)


def test_weights_at_the_edges_of_their_range(prover):
    """1, 2^64, 2^128 - 1 and a weight whose low word is zero: every word of the 128 bits enters the multiple of A"""
    m = made(prover, 3)
    proofs, pubs = batch(m, 5)
    words, pw = arrays(m, proofs, pubs)
    got, path = m["verifier"].verify_all(words, [1, 1 << 64, (1 << 128) - 1, 7 << 96, (1 << 127) + 1], pw)
    assert (got.tolist(), path) == ([0] * 5, 0)


# ---- invalid batches against the per-proof function ----
def g1_on_curve_outside_torsion():
    return PC.g1_outside_torsion()


CORRUPTIONS = {
    # name: (alter(proofs, pubs, i), the path: 1 where the bad proof survives the point checks)
    "C of another proof": (lambda pr, pu, i: pr.__setitem__(i, (pr[i][0], pr[i][1], pr[(i + 1) % 8][2])), 1),
    "A negated": (lambda pr, pu, i: pr.__setitem__(i, (PC.g1_neg(pr[i][0]), pr[i][1], pr[i][2])), 1),
    "a public input off by one": (lambda pr, pu, i: pu[i].__setitem__(1, (pu[i][1] + 1) % R), 1),
    "a coordinate >= p": (lambda pr, pu, i: pr.__setitem__(i, ((pr[i][0][0] + P, pr[i][0][1]), pr[i][1], pr[i][2])), 0),
    "a point off the curve": (lambda pr, pu, i: pr.__setitem__(i, (pr[i][0], pr[i][1], (pr[i][2][0], (pr[i][2][1] + 1) % P))), 0),
    "a G1 point outside the r-torsion": (lambda pr, pu, i: pr.__setitem__(i, (g1_on_curve_outside_torsion(), pr[i][1], pr[i][2])), 0),
    "a public input >= r": (lambda pr, pu, i: pu[i].__setitem__(0, R), 0),
}
WANT = {"C of another proof": 1, "A negated": 1, "a public input off by one": 1, "a coordinate >= p": 2, "a point off the curve": 2,
        "a G1 point outside the r-torsion": 3, "a public input >= r": 4}


@pytest.mark.parametrize("at", [0, 32, 64])
@pytest.mark.parametrize("name", list(CORRUPTIONS))
def test_one_bad_proof_in_65_gets_the_per_proof_verdicts(prover, name, at):
    m = made(prover, 3)
    proofs, pubs = batch(m, 65)
    alter, want_path = CORRUPTIONS[name]
    alter(proofs, pubs, at)
    words, pw = arrays(m, proofs, pubs)
    want = m["verifier"].verify(words, pw)
    assert want.tolist() == [WANT[name] if i == at else 0 for i in range(65)]      # the oracle says what the case says
    got, path = m["verifier"].verify_all(words, weights(65, 65 + at), pw)
    assert got.tobytes() == want.tobytes()
    assert path == want_path


def test_a_trusted_batch_skips_the_torsion_check_like_the_per_proof_function(prover):
    """with CP_PAIRING_TRUSTED a point outside the r-torsion reaches the equation, where its result is unspecified; whatever the
    per-proof function says of it, this call says the same, and the other proofs keep verdict 0"""
    import cityprover as cp
    m = made(prover, 2)
    proofs, pubs = batch(m, 5)
    proofs[2] = (PC.g1_outside_torsion(), proofs[2][1], proofs[2][2])
    words, pw = arrays(m, proofs, pubs)
    want = m["verifier"].verify(words, pw, flags=cp.PAIRING_TRUSTED)
    got, path = m["verifier"].verify_all(words, weights(5, 5), pw, flags=cp.PAIRING_TRUSTED)
    assert [want[i] for i in (0, 1, 3, 4)] == [0] * 4
    assert got.tobytes() == want.tobytes()


def test_every_proof_bad_at_the_point_checks_leaves_nothing_to_aggregate(prover):
    m = made(prover, 2)
    proofs, pubs = batch(m, 3)
    for i in range(3):
        pubs[i][0] = R + i
    words, pw = arrays(m, proofs, pubs)
    got, path = m["verifier"].verify_all(words, weights(3, 3), pw)
    assert (got.tolist(), path) == ([4, 4, 4], 0)
    assert m["verifier"].verify(words, pw).tolist() == [4, 4, 4]


def test_a_stored_proof_that_does_not_unpack_gets_verdict_2_and_the_rest_aggregates(prover):
    import cityprover as cp
    m = made(prover, 3)
    proofs, pubs = batch(m, 65)
    _, pw = arrays(m, proofs, pubs)
    blobs = [cp.groth16_pack_city(*p) for p in proofs]
    b = bytearray(blobs[64])
    b[0:48] = P.to_bytes(48, "little")        # pi_a: x = p
    blobs[64] = bytes(b)
    want = m["verifier"].verify_city(blobs, pw)
    assert want.tolist() == [0] * 64 + [2]
    got, path = m["verifier"].verify_all_city(blobs, weights(65, 1), pw)
    assert got.tobytes() == want.tobytes() and path == 0


# ---- the aggregate really runs, and the weights really enter it ----
def test_a_cancelling_pair_passes_only_under_equal_weights(prover):
    """C_1 + D and C_2 - D: each proof alone is rejected, and sum rho_i C_i is unchanged exactly when rho_1 = rho_2 - the
    documented consequence of weights the maker of the proofs can predict"""
    m = made(prover, 3)
    (p1, p2), pubs = batch(m, 2)
    D = PC.g1_mul(0xd15ea5e)
    proofs = [(p1[0], p1[1], O.bls_g1_add(p1[2], D)), (p2[0], p2[1], O.bls_g1_add(p2[2], PC.g1_neg(D)))]
    words, pw = arrays(m, proofs, pubs)
    assert m["verifier"].verify(words, pw).tolist() == [1, 1]
    got, path = m["verifier"].verify_all(words, weights(2, 2), pw)
    assert (got.tolist(), path) == ([1, 1], 1)
    got, path = m["verifier"].verify_all(words, [1, 1], pw)
    assert (got.tolist(), path) == ([0, 0], 0)
    got, path = m["verifier"].verify_all(words, [0x1234 << 64, 0x1234 << 64], pw)       # equal, and not one
    assert (got.tolist(), path) == ([0, 0], 0)


# ---- refusals ----
def test_refusals_leave_the_output_and_the_context_alone(prover):
    import cityprover as cp
    m, m1 = made(prover, 3), made(prover, 1)
    lib, h = prover.lib, m["verifier"].handle
    proofs, pubs = batch(m, 5)
    words, pw = arrays(m, proofs, pubs)
    blobs = np.frombuffer(b"".join(cp.groth16_pack_city(*p) for p in proofs), np.uint8).copy()
    w = cp._weights128(weights(5, 9), 5)
    w0 = w.copy()
    w0[3] = 0
    out, path = np.full(5, 9, np.uint8), ctypes.c_int(9)
    pp, bp, xp, wp, w0p, op, tp = (words.ctypes.data_as(u64p), blobs.ctypes.data_as(u8p), pw.ctypes.data_as(u64p), w.ctypes.data_as(u64p),
                                   w0.ctypes.data_as(u64p), out.ctypes.data_as(u8p), ctypes.byref(path))
    for fn, prf in ((lib.cp_groth16_verify_all_bls12381, pp), (lib.cp_groth16_verify_all_city_bls12381, bp)):
        for args, msg in (((h, prf, xp, 5, None, 0, op, tp), "weights_host is NULL"),
                          ((h, prf, xp, 5, w0p, 0, op, tp), "weight 3 is zero"),
                          ((h, prf, xp, 5, wp, 2, op, tp), "unknown flag bits 0x2"),
                          ((None, prf, xp, 5, wp, 0, op, tp), "verifier is NULL"),
                          ((h, None, xp, 5, wp, 0, op, tp), "NULL argument"),
                          ((h, prf, xp, 5, wp, 0, None, tp), "NULL argument"),
                          ((h, prf, None, 5, wp, 0, op, tp), "public_inputs_host is NULL"),
                          ((h, prf, xp, 0, wp, 0, op, tp), "at least 1")):
            assert fn(prover.ctx, *args) == -1, msg
            assert msg.encode() in lib.cp_last_error(prover.ctx), msg
            assert (out == 9).all() and path.value == 9
        assert fn(prover.ctx, h, prf, xp, 5, wp, 0, op, None) == 0      # path_out may be NULL
        assert out.tolist() == [0] * 5
        out[:] = 9
    # no public input beside wire 0: NULL is fine
    p1, _ = batch(m1, 2)
    got, path = m1["verifier"].verify_all(np.stack([proof_words(*p) for p in p1]), weights(2, 1))
    assert (got.tolist(), path) == ([0, 0], 0)


def walk(call, want):
    """cp_fault_inject(CP_FAULT_DEVMEM, j) for j = 0, 1, ... on a fresh context with an empty pool until the call gets through:
    each refusal is out of memory, and the same call on the same context then gives the expected result"""
    import cityprover as cp
    lib = cp.load_library()
    refused = 0
    try:
        for j in range(MAX_WALK):
            p = cp.Prover(0)
            try:
                cp.batch_pool_trim(p)
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    got = call(p)
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert "[-4]" in str(e) and "out of memory" in str(e), (j, str(e))
                    refused += 1
                    assert call(p) == want, "allocation %d refused: the context did not recover" % j
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                assert got == want
                return refused
            finally:
                lib.cp_fault_inject(DEVMEM, -1)
                p.close()
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    pytest.fail("the walk did not end before j = %d" % MAX_WALK)


@pytest.mark.parametrize("bad", [False, True])
def test_injected_allocation_failures(prover, bad):
    """every allocation of the call on a cold context: the call's one array and the MSM workspace. With a bad proof in the batch
    the walk also passes the array of the per-proof check behind them; a refusal there may be absorbed (the aggregated attempt
    has just parked its array in the pool, which is emptied before an allocation is given up), so it is not counted on"""
    import cityprover as cp
    m = made(prover, 3)
    proofs, pubs = batch(m, 3)
    if bad:
        proofs[1] = (PC.g1_neg(proofs[1][0]), proofs[1][1], proofs[1][2])
    words, pw = arrays(m, proofs, pubs)
    blobs = [cp.groth16_pack_city(*p) for p in proofs]
    w = weights(3, 3)
    want = ([0, 1, 0], 1) if bad else ([0, 0, 0], 0)

    def plain(p):
        got, path = m["verifier"].verify_all(words, w, pw, prover=p)
        return got.tolist(), path

    def stored(p):
        got, path = m["verifier"].verify_all_city(blobs, w, pw, prover=p)
        return got.tolist(), path
    assert walk(plain, want) >= 2
    assert walk(stored, want) >= 2
