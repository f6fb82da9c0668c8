"""cp_groth16_verify_bls12381 on the device: real proofs of real keys (cp_groth16_setup_bls12381 and
cp_groth16_prove_r1cs_bls12381) are accepted without the trapdoor, altered ones are rejected, and batches of proofs simulated
from the trapdoor (a, b random, c = (a b - alpha beta - gamma sum x_i ic_i) / delta, the points by the oracle) get the right
verdict item by item. The injected allocation failures are refused allocations that return a status (the pattern of
tests/test_gpu_alloc_faults.py): nothing here faults the device."""
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


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    for m in _made.values():      # the keys and verifiers of the module
        m["verifier"].close()
        m["key"].free()
    _made.clear()
    p.close()


def setup(prover, case):
    import cityprover as cp
    s = case["system"]
    return cp.Groth16Key.setup(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], case["n_pub"], **case["td"])


def proof_words(A, B, Cc):
    return np.concatenate([PC.g1_words(A), PC.g2_words(B), PC.g1_words(Cc)])


def publics_words(xs):
    """public inputs (wires 1 ..) of one proof -> (len, 4) u64"""
    return np.array([[(x >> (64 * j)) & PC.MASK for j in range(4)] for x in xs], np.uint64).reshape(len(xs), 4)


def real_proof(prover, key, case, seed):
    """(A, B, C) by the library's prover from the witness, and the public inputs"""
    import cityprover as cp
    sysm = case["system"]
    r, s = (x % R for x in GC.random_scalars(2, seed))
    h = cp.R1cs(prover, sysm["n"], sysm["n_wires"], RC.limbs4(sysm["coeffs"]), sysm["mats"])
    dw = prover.to_device(RC.limbs4(sysm["w"]))
    try:
        A, B, Cc = cp.groth16_prove_r1cs(prover, key.pk(), h, dw.ptr, r, s)
    finally:
        dw.free()
        h.free()
    return (A, B, Cc), [int(x) for x in sysm["w"][1:case["n_pub"]]]


_made = {}


def made(prover, name):
    """case, key, verifier, one real proof: once per module"""
    import cityprover as cp
    if name not in _made:
        n, kw = {"2^3": (8, {}), "2^5": (32, {"unused_public": True}), "one_public": (8, {})}[name]
        case = GC.small_case(n, 1 if name == "one_public" else 3, 3 if n == 8 else 6, 7000 + n + len(name), **kw)
        key = setup(prover, case)
        proof, pub = real_proof(prover, key, case, 7100 + n)
        _made[name] = {"case": case, "key": key, "verifier": cp.Groth16Verifier.from_key(prover, key), "proof": proof, "pub": pub}
    return _made[name]


def verdict(m, proof, pub, flags=0):
    pubs = publics_words(pub)[None] if pub else None
    return int(m["verifier"].verify(proof_words(*proof)[None], pubs, flags=flags)[0])


@pytest.mark.parametrize("name", ["2^3", "2^5", "one_public"])
def test_real_proofs_are_accepted(prover, name):
    import cityprover as cp
    m = made(prover, name)
    if name == "2^5":   # the case has what it says: a public wire that occurs nowhere, a flagged IC entry
        assert m["case"]["exp"]["ic"][2] == 0 and m["key"].vk()["ic"][2] is None
    assert verdict(m, m["proof"], m["pub"]) == 0
    assert verdict(m, m["proof"], m["pub"], flags=cp.PAIRING_TRUSTED) == 0


def test_a_rerandomised_triple_is_accepted(prover):
    """([t] A, [1/t] B, C) is another valid proof: no comparison of points reproduces this verdict"""
    m = made(prover, "2^3")
    A, B, Cc = m["proof"]
    t = 0x1234567890abcdef1234567
    other = (O.bls_g1_mul(A, t), O.bls_g2_mul(B, pow(t, -1, R)), Cc)
    assert other[0] != A and other[1] != B
    assert verdict(m, other, m["pub"]) == 0


def test_altered_proofs_and_inputs_are_rejected(prover):
    m, m5 = made(prover, "2^3"), made(prover, "2^5")
    A, B, Cc = m["proof"]
    pub = m["pub"]
    assert pub[0] != pub[1]
    assert verdict(m, (O.bls_g1_add(A, PR.G1), B, Cc), pub) == 1
    assert verdict(m, (A, B, O.bls_g1_add(Cc, PR.G1)), pub) == 1
    assert verdict(m, (A, O.bls_g2_add(B, PR.G2), Cc), pub) == 1
    assert verdict(m, m["proof"], [(pub[0] + 1) % R, pub[1]]) == 1
    assert verdict(m, m["proof"], [pub[1], pub[0]]) == 1
    assert verdict(m5, m["proof"], pub) == 1                 # the proof of one key under the other key's verifier
    assert verdict(m, m5["proof"], m5["pub"]) == 1
    assert verdict(m, m["proof"], pub) == 0                  # and the unaltered one, last


# ---- proofs simulated from the trapdoor ----
def simulated(case, rng, xs):
    """a valid (A, B, C) for the public inputs xs (wires 1 ..)"""
    td, ic = case["td"], case["exp"]["ic"]
    a, b = (int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1 for _ in range(2))
    pub = (ic[0] + sum(x * y for x, y in zip(xs, ic[1:]))) % R
    c = (a * b - td["alpha"] * td["beta"] - td["gamma"] * pub) * pow(td["delta"], -1, R) % R
    return (PC.g1_mul(a), PC.g2_mul(b), PC.g1_mul(c)), (a, b, c)


def spoil(kind, proof, logs, xs):
    """the item made bad in the way of verdict class `kind`"""
    A, B, Cc = proof
    if kind == 1:
        return (A, B, PC.g1_mul(logs[2] + 1)), xs
    if kind == 2:
        return ((A[0], (A[1] + 1) % P), B, Cc), xs          # off the curve
    if kind == 3:
        return (A, PC.g2_outside_torsion(), Cc), xs
    assert kind == 4
    return proof, [xs[0], R]                                # a public input that is not below r


@pytest.fixture(scope="module")
def batch130(prover):
    m = made(prover, "2^3")
    rng = np.random.default_rng(130)
    items = []
    for i in range(130):
        xs = [int.from_bytes(rng.bytes(40), "little") % R for _ in range(2)]
        proof, logs = simulated(m["case"], rng, xs)
        items.append((proof, logs, xs))
    return items


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
def test_batch_of_130_with_every_verdict_class_at_every_boundary(prover, batch130, rotation):
    """positions 0, 63, 64, 129 hold the classes 1 .. 4, rotated: over the four cases every class sits at every position"""
    m = made(prover, "2^3")
    want = np.zeros(130, np.uint8)
    proofs, pubs = [], []
    for i, (proof, logs, xs) in enumerate(batch130):
        if i in (0, 63, 64, 129):
            kind = ((0, 63, 64, 129).index(i) + rotation) % 4 + 1
            proof, xs = spoil(kind, proof, logs, xs)
            want[i] = kind
        proofs.append(proof_words(*proof))
        pubs.append(publics_words(xs))
    got = m["verifier"].verify(np.stack(proofs), np.stack(pubs))
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("n", [1, 64])
def test_smaller_batches(prover, batch130, n):
    import cityprover as cp
    m = made(prover, "2^3")
    proofs = np.stack([proof_words(*it[0]) for it in batch130[:n]])
    pubs = np.stack([publics_words(it[2]) for it in batch130[:n]])
    assert m["verifier"].verify(proofs, pubs).tolist() == [0] * n
    assert m["verifier"].verify(proofs, pubs, flags=cp.PAIRING_TRUSTED).tolist() == [0] * n
    bad, xs = spoil(1, *batch130[n - 1])
    proofs[n - 1] = proof_words(*bad)
    assert m["verifier"].verify(proofs, pubs).tolist() == [0] * (n - 1) + [1]


def test_public_input_edges(prover):
    m = made(prover, "2^3")
    case, rng = m["case"], np.random.default_rng(5)
    ic = case["exp"]["ic"]
    assert all(ic)
    x2 = int.from_bytes(rng.bytes(40), "little") % R
    to_infinity = [(-(ic[0] + x2 * ic[2]) * pow(ic[1], -1, R)) % R, x2]          # L = [ic_0 + x_1 ic_1 + x_2 ic_2] G1 = infinity
    assert (ic[0] + to_infinity[0] * ic[1] + to_infinity[1] * ic[2]) % R == 0
    for xs in ([0, 0], [R - 1, 0], [0, R - 1], [R - 1, R - 1], to_infinity):
        proof, logs = simulated(case, rng, xs)
        assert verdict(m, proof, xs) == 0, xs
        assert verdict(m, spoil(1, proof, logs, xs)[0], xs) == 1, xs
        other = list(xs)
        other[1] = (other[1] + 1) % R
        assert verdict(m, proof, other) == 1, xs
    # no public input beside wire 0: public_inputs_host is NULL
    m1 = made(prover, "one_public")
    proof, logs = simulated(m1["case"], rng, [])
    assert verdict(m1, proof, []) == 0
    assert verdict(m1, spoil(1, proof, logs, [])[0], []) == 1
    # all-zero coordinates cannot mean infinity: off the curve
    A, B, Cc = proof
    zero = np.concatenate([np.zeros(12, np.uint64), PC.g2_words(B), PC.g1_words(Cc)])
    assert m1["verifier"].verify(zero[None]).tolist() == [2]


def test_create_refuses_bad_key_points_by_name(prover):
    import cityprover as cp
    m = made(prover, "2^3")
    key = m["key"]
    vk = cp.Groth16Vk()
    prover._check(prover.lib.cp_groth16_key_vk(key.handle, ctypes.byref(vk), None, None))
    xy, inf = np.zeros((vk.n_public, 12), np.uint64), np.zeros(vk.n_public, np.uint8)
    prover._check(prover.lib.cp_groth16_key_vk(key.handle, ctypes.byref(vk), xy.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                               inf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))

    def copy_of(vk):
        out = cp.Groth16Vk()
        ctypes.memmove(ctypes.byref(out), ctypes.byref(vk), ctypes.sizeof(vk))
        return out
    bad = copy_of(vk)
    bad.gamma_g2[0] ^= 1
    with pytest.raises(cp.CityProverError, match="gamma_g2 is not on the curve"):
        cp.Groth16Verifier.create(prover, bad, xy, inf)
    bad = copy_of(vk)
    bad.delta_g2[:] = PC.g2_words(PC.g2_outside_torsion()).tolist()
    with pytest.raises(cp.CityProverError, match="delta_g2 is not in the r-torsion"):
        cp.Groth16Verifier.create(prover, bad, xy, inf)
    bad = copy_of(vk)
    bad.alpha_g1[0:6] = PC.w6(P)
    with pytest.raises(cp.CityProverError, match="alpha_g1 has a coordinate"):
        cp.Groth16Verifier.create(prover, bad, xy, inf)
    bad_ic = xy.copy()
    bad_ic[1, 6] ^= 1
    with pytest.raises(cp.CityProverError, match=r"ic\[1\] is not on the curve"):
        cp.Groth16Verifier.create(prover, vk, bad_ic, inf)
    # the same context straight afterwards, through the explicit constructor
    v = cp.Groth16Verifier.create(prover, vk, xy, inf)
    try:
        assert int(v.verify(proof_words(*m["proof"])[None], publics_words(m["pub"])[None])[0]) == 0
    finally:
        v.close()
    # argument refusals of verify
    lib = prover.lib
    out = np.full(1, 9, np.uint8)
    pw, pubw = proof_words(*m["proof"]), publics_words(m["pub"])
    u64p, u8p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8)
    h = m["verifier"].handle
    for args, msg in (((None, pw.ctypes.data_as(u64p), None, 1, 0, out.ctypes.data_as(u8p)), "verifier is NULL"),
                      ((h, None, None, 1, 0, out.ctypes.data_as(u8p)), "NULL argument"),
                      ((h, pw.ctypes.data_as(u64p), None, 1, 0, out.ctypes.data_as(u8p)), "public_inputs_host is NULL"),
                      ((h, pw.ctypes.data_as(u64p), None, 0, 0, out.ctypes.data_as(u8p)), "at least 1"),
                      ((h, pw.ctypes.data_as(u64p), pubw.ctypes.data_as(u64p), 1, 4, out.ctypes.data_as(u8p)), "unknown flag")):
        assert lib.cp_groth16_verify_bls12381(prover.ctx, *args) == -1, msg
        assert msg.encode() in lib.cp_last_error(prover.ctx), msg
        assert out[0] == 9
    assert verdict(m, m["proof"], m["pub"]) == 0


def test_injected_allocation_failures(prover):
    """cp_fault_inject(CP_FAULT_DEVMEM, j) for every j until create and verify both get through: out of memory, nothing held,
    and the same context then verifies"""
    import cityprover as cp
    lib = cp.load_library()
    m = made(prover, "2^3")
    proofs, pubs = proof_words(*m["proof"])[None], publics_words(m["pub"])[None]
    refused_create = refused_verify = 0
    try:
        for j in range(MAX_WALK):
            p = cp.Prover(0)
            try:
                cp.batch_pool_trim(p)
                held = cp.batch_pool_stats(0)["bytes"]
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    v = cp.Groth16Verifier.from_key(p, m["key"])
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert "out of memory" in str(e), (j, str(e))
                    assert cp.batch_pool_stats(0)["bytes"] == held, j
                    refused_create += 1
                    v = cp.Groth16Verifier.from_key(p, m["key"])       # the same context, straight afterwards
                    try:
                        assert v.verify(proofs, pubs).tolist() == [0]
                    finally:
                        v.close()
                    continue
                lib.cp_fault_inject(DEVMEM, -1)
                try:
                    # the verifier is there: now the allocations of verify
                    for i in range(MAX_WALK):
                        assert lib.cp_fault_inject(DEVMEM, i) == 0
                        try:
                            got = v.verify(proofs, pubs)
                        except cp.CityProverError as e:
                            lib.cp_fault_inject(DEVMEM, -1)
                            assert "[-4]" in str(e) and "out of memory" in str(e), (i, str(e))
                            refused_verify += 1
                            assert v.verify(proofs, pubs).tolist() == [0]
                            continue
                        lib.cp_fault_inject(DEVMEM, -1)
                        assert got.tolist() == [0]
                        break
                    else:
                        pytest.fail("the walk over verify did not end")
                finally:
                    v.close()
                break
            finally:
                lib.cp_fault_inject(DEVMEM, -1)
                p.close()
        else:
            pytest.fail("the walk over create did not end before j = %d" % MAX_WALK)
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    assert refused_create >= 5      # the pairing of (alpha, beta) and the verifier's four arrays
    assert refused_verify >= 1      # the one allocation of a call


def test_a_verifier_serves_other_contexts_and_outlives_its_own(prover):
    import cityprover as cp
    m = made(prover, "2^3")
    p = cp.Prover(0)
    v = cp.Groth16Verifier.from_key(p, m["key"])
    proofs, pubs = proof_words(*m["proof"])[None], publics_words(m["pub"])[None]
    assert v.verify(proofs, pubs, prover=prover).tolist() == [0]      # another context of the same device
    p.close()
    assert v.verify(proofs, pubs, prover=prover).tolist() == [0]      # after its own context is gone
    v.close()
    v.close()      # and a second close does nothing
