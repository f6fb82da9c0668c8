"""Stored Groth16 proofs (4 x 48 bytes of compressed points) decompressed and verified on the device:
cp_groth16_proofs_unpack_city_bls12381 against the host function cp_groth16_proof_unpack_city word for word, and
cp_groth16_verify_city_bls12381 against cp_groth16_verify_bls12381 on the unpacked coordinates, item for item. The proofs are
those of tests/test_gpu_groth16_verify.py: real ones of real keys, and batches simulated from the trapdoor. The injected
allocation failures are refused allocations that return a status: nothing here faults the device."""
import ctypes
import json
import os

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
POSITIONS = (0, 63, 64, 129)
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


def made(prover, name):
    """case, key, verifier and one real proof of the key, once per module"""
    import cityprover as cp
    if name not in _made:
        n, kw = {"2^3": (8, {}), "2^5": (32, {"unused_public": True}), "one_public": (8, {})}[name]
        case = GC.small_case(n, 1 if name == "one_public" else 3, 3 if n == 8 else 6, 7000 + n + len(name), **kw)
        s = case["system"]
        key = cp.Groth16Key.setup(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], case["n_pub"], **case["td"])
        r, t = (x % R for x in GC.random_scalars(2, 7100 + n))
        h = cp.R1cs(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"])
        dw = prover.to_device(RC.limbs4(s["w"]))
        try:
            proof = cp.groth16_prove_r1cs(prover, key.pk(), h, dw.ptr, r, t)
        finally:
            dw.free()
            h.free()
        _made[name] = {"case": case, "key": key, "verifier": cp.Groth16Verifier.from_key(prover, key), "proof": proof,
                       "pub": [int(x) for x in s["w"][1:case["n_pub"]]]}
    return _made[name]


def simulated(case, rng, xs):
    """a valid (A, B, C) for the public inputs xs from the trapdoor, and the logarithms"""
    td, ic = case["td"], case["exp"]["ic"]
    a, b = (int.from_bytes(rng.bytes(40), "little") % (R - 1) + 1 for _ in range(2))
    pub = (ic[0] + sum(x * y for x, y in zip(xs, ic[1:]))) % R
    c = (a * b - td["alpha"] * td["beta"] - td["gamma"] * pub) * pow(td["delta"], -1, R) % R
    return (PC.g1_mul(a), PC.g2_mul(b), PC.g1_mul(c)), (a, b, c)


@pytest.fixture(scope="module")
def batch130(prover):
    """130 valid proofs of the "2^3" key with their public inputs, packed: (proof, logs, xs, blob)"""
    import cityprover as cp
    m = made(prover, "2^3")
    rng = np.random.default_rng(130)
    items = []
    for i in range(130):
        xs = [int.from_bytes(rng.bytes(40), "little") % R for _ in range(2)]
        proof, logs = simulated(m["case"], rng, xs)
        items.append((proof, logs, xs, cp.groth16_pack_city(*proof)))
    return items


def host_words(blob):
    """cp_groth16_proof_unpack_city -> 48 u64, or None where it refuses"""
    import cityprover as cp
    try:
        return proof_words(*cp.groth16_unpack_city(blob))
    except cp.CityProverError:
        return None


def check_against_host(prover, blobs):
    import cityprover as cp
    coords, status = cp.groth16_unpack_city_batch(prover, blobs)
    assert coords.shape == (len(blobs), 48) and status.shape == (len(blobs),)
    for i, blob in enumerate(blobs):
        want = host_words(blob)
        assert (status[i] == 0) == (want is not None), i
        assert coords[i].tolist() == (want.tolist() if want is not None else [0] * 48), i
    return coords, status


def neg1(pt):
    return (pt[0], -pt[1] % P)


def neg2(pt):
    return (pt[0], PR.f2_sub((0, 0), pt[1]))


# ---- unpack against the host function ----
def test_unpack_reference_samples_and_the_on_chain_key(prover, golden_dir):
    samples = json.load(open(os.path.join(golden_dir, "groth16_proof_samples.json")))
    blobs = [b"".join(bytes.fromhex(s[k]) for k in ("pi_a", "pi_b_a0", "pi_b_a1", "pi_c")) for s in samples]
    vk = b"".join(bytes.fromhex(c) for c in json.load(open(os.path.join(golden_dir, "groth16_verifier_data.json")))["chunks"])
    g1 = [vk[o:o + 48] for o in (0, 48, 96, 144)]
    g2 = [vk[o:o + 96] for o in (192, 288, 384)]
    blobs += [g1[a] + g2[b] + g1[c] for a, b, c in ((0, 0, 1), (2, 1, 3), (1, 2, 0))]
    assert len(blobs) == 5
    _, status = check_against_host(prover, blobs)
    assert status.tolist() == [0] * 5
    as_array = np.frombuffer(b"".join(blobs), np.uint8).reshape(5, 192)      # the other accepted argument form
    import cityprover as cp
    assert (cp.groth16_unpack_city_batch(prover, as_array)[0] == cp.groth16_unpack_city_batch(prover, blobs)[0]).all()


def test_unpack_130_with_both_signs_and_the_calls_of_1_and_64(prover, batch130):
    """proof i carries -A, -B, -C by the bits of i: every element with both signs of y, in every part of a workgroup"""
    import cityprover as cp
    blobs, want = [], []
    for i, (proof, _, _, _) in enumerate(batch130):
        A, B, Cc = proof
        t = (neg1(A) if i & 1 else A, neg2(B) if i & 2 else B, neg1(Cc) if i & 4 else Cc)
        blobs.append(cp.groth16_pack_city(*t))
        want.append(proof_words(*t))
    flags = np.array([[b[47] >> 7, b[143] >> 7, b[191] >> 7] for b in blobs])
    assert (flags.min(axis=0) == 0).all() and (flags.max(axis=0) == 1).all()
    coords, status = check_against_host(prover, blobs)
    assert status.tolist() == [0] * 130
    assert (coords == np.stack(want)).all()                                  # and the points that were packed
    for n in (1, 64):
        c, s = cp.groth16_unpack_city_batch(prover, blobs[:n])
        assert s.tolist() == [0] * n and (c == coords[:n]).all()


def twist_points_with_a_zero_half():
    """x = (s, t) with s^2 = (t^3 - 4) / (3 t): the u part of x^3 + 4 + 4 u vanishes, so y^2 = v lies in F_p and
    y = (sqrt v, 0) where v is a residue (the sign falls to c0), y = (0, sqrt -v) where it is not. One of each, t from 1 up."""
    found = {}
    t = 0
    while len(found) < 2:
        t += 1
        s = PC.fp_sqrt((t**3 - 4) * pow(3 * t, -1, P) % P)
        if s is None:
            continue
        v = (s**3 - 3 * s * t * t + 4) % P
        y0 = PC.fp_sqrt(v)
        kind = "real" if y0 is not None else "imaginary"
        if kind in found:
            continue
        y = (y0, 0) if y0 is not None else (0, PC.fp_sqrt(-v % P))
        x = (s, t)
        assert PR.f2_mul(y, y) == PR.f2_add(PR.f2_mul(PR.f2_mul(x, x), x), (4, 4))
        found[kind] = (x, y)
    return found


def test_twist_points_whose_y_has_a_zero_half(prover):
    import cityprover as cp
    m = made(prover, "2^3")
    found = twist_points_with_a_zero_half()
    assert found["real"][1][1] == 0 and found["imaginary"][1][0] == 0
    blobs, want = [], []
    for kind in ("real", "imaginary"):
        for Q in (found[kind], neg2(found[kind])):
            blobs.append(cp.groth16_pack_city(PR.G1, Q, PR.G1))
            want.append(proof_words(PR.G1, Q, PR.G1))
    assert sorted(b[143] >> 7 for b in blobs) == [0, 0, 1, 1]
    coords, status = check_against_host(prover, blobs)
    assert status.tolist() == [0] * 4 and (coords == np.stack(want)).all()
    pubs = np.stack([publics_words([1, 2])] * 4)
    assert m["verifier"].verify_city(blobs, pubs).tolist() == [3] * 4        # on the twist, outside the r-torsion


# ---- defects ----
def first_x_off_the_curve():
    x = 1
    while PC.fp_sqrt((x**3 + 4) % P) is not None:
        x += 1
    return x


def first_x_off_the_twist():
    k = 1
    while PC.f2_sqrt(PR.f2_add(PR.f2_mul(PR.f2_mul((k, 1), (k, 1)), (k, 1)), (4, 4))) is not None:
        k += 1
    return (k, 1)


def with_byte(blob, at, bits):
    b = bytearray(blob)
    b[at] |= bits
    return bytes(b)


def with_x(blob, at, x, keep_sign=True):
    b = bytearray(blob)
    sign = b[at + 47] & 0x80 if keep_sign else 0
    b[at:at + 48] = x.to_bytes(48, "little")
    b[at + 47] |= sign
    return bytes(b)


def twist_x(blob, x):
    return with_x(with_x(blob, 48, x[0], keep_sign=False), 96, x[1])


DEFECTS = [
    ("0x40 on pi_a", 1, lambda b: with_byte(b, 47, 0x40)),
    ("0x40 on pi_b_a1", 1, lambda b: with_byte(b, 143, 0x40)),
    ("0x40 on pi_c", 1, lambda b: with_byte(b, 191, 0x40)),
    ("0x80 on pi_b_a0", 1, lambda b: with_byte(b, 95, 0x80)),
    ("0x40 on pi_b_a0", 1, lambda b: with_byte(b, 95, 0x40)),
    ("pi_a: x = p", 2, lambda b: with_x(b, 0, P)),
    ("pi_b: c0 = p", 2, lambda b: with_x(b, 48, P, keep_sign=False)),
    ("pi_a: no curve point", 3, lambda b: with_x(b, 0, first_x_off_the_curve())),
    ("pi_b: no twist point", 3, lambda b: twist_x(b, first_x_off_the_twist())),
]


@pytest.mark.parametrize("rotation", range(len(DEFECTS)))
def test_one_defect_per_proof_at_the_workgroup_boundaries(prover, batch130, rotation):
    """positions 0, 63, 64, 129 hold four of the nine defects, rotated: over the cases every defect sits at every position"""
    import cityprover as cp
    m = made(prover, "2^3")
    blobs = [it[3] for it in batch130]
    want = np.zeros(130, np.uint8)
    for k, i in enumerate(POSITIONS):
        name, cls, spoil = DEFECTS[(k + rotation) % len(DEFECTS)]
        blobs[i] = spoil(blobs[i])
        want[i] = cls
        with pytest.raises(cp.CityProverError):
            cp.groth16_unpack_city(blobs[i])                                 # the host function refuses the same proof
    coords, status = cp.groth16_unpack_city_batch(prover, blobs)
    assert status.tolist() == want.tolist()
    for i in range(130):
        if want[i]:
            assert not coords[i].any(), i
        else:
            assert coords[i].tolist() == proof_words(*batch130[i][0]).tolist(), i
    pubs = np.stack([publics_words(it[2]) for it in batch130])
    assert m["verifier"].verify_city(blobs, pubs).tolist() == [2 if w else 0 for w in want]


def test_two_defects_in_one_proof(prover, batch130):
    import cityprover as cp
    m = made(prover, "2^3")
    blobs = [it[3] for it in batch130[:6]]
    pairs = ((0, 5), (5, 8), (7, 8), (2, 6), (7, 3))
    for i, (a, b) in enumerate(pairs):
        blobs[i] = DEFECTS[b][2](DEFECTS[a][2](blobs[i]))
    coords, status = check_against_host(prover, blobs)
    assert all(status[:5]) and status[5] == 0
    pubs = np.stack([publics_words(it[2]) for it in batch130[:6]])
    assert m["verifier"].verify_city(blobs, pubs).tolist() == [2] * 5 + [0]


# ---- verdicts ----
def spoil(kind, proof, logs, xs):
    A, B, Cc = proof
    if kind == 1:
        return (A, B, PC.g1_mul(logs[2] + 1)), xs
    if kind == 3:
        return (A, PC.g2_outside_torsion(), Cc), xs
    assert kind == 4
    return proof, [xs[0], R]


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
def test_verdicts_equal_those_of_the_unpacked_proofs(prover, batch130, rotation):
    """classes 1, 3, 4 (a proof of class 2 has no stored form) at positions 0, 63, 64, 129, rotated"""
    import cityprover as cp
    m = made(prover, "2^3")
    want = np.zeros(130, np.uint8)
    blobs, words, pubs = [], [], []
    for i, (proof, logs, xs, blob) in enumerate(batch130):
        if i in POSITIONS:
            kind = (1, 3, 4, 1)[(POSITIONS.index(i) + rotation) % 4]
            proof, xs = spoil(kind, proof, logs, xs)
            blob = cp.groth16_pack_city(*proof)
            want[i] = kind
        blobs.append(blob)
        words.append(proof_words(*proof))
        pubs.append(publics_words(xs))
    pubs = np.stack(pubs)
    got = m["verifier"].verify_city(blobs, pubs)
    assert got.tolist() == m["verifier"].verify(np.stack(words), pubs).tolist()
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("n", [1, 64])
def test_trusted_batches(prover, batch130, n):
    import cityprover as cp
    m = made(prover, "2^3")
    blobs = [it[3] for it in batch130[:n]]
    pubs = np.stack([publics_words(it[2]) for it in batch130[:n]])
    assert m["verifier"].verify_city(blobs, pubs, flags=cp.PAIRING_TRUSTED).tolist() == [0] * n
    assert m["verifier"].verify_city(blobs, pubs).tolist() == [0] * n


@pytest.mark.parametrize("name", ["2^3", "2^5", "one_public"])
def test_real_proofs_and_their_negations(prover, name):
    """flipping 0x80 of pi_a gives (-A, B, C): well formed, and the equation does not hold"""
    import cityprover as cp
    m = made(prover, name)
    blob = cp.groth16_pack_city(*m["proof"])
    neg = bytearray(blob)
    neg[47] ^= 0x80
    A, B, Cc = m["proof"]
    assert cp.groth16_unpack_city(bytes(neg)) == (neg1(A), B, Cc)
    pubs = np.stack([publics_words(m["pub"])] * 2) if m["pub"] else None
    assert m["verifier"].verify_city([blob, bytes(neg)], pubs).tolist() == [0, 1]


# ---- refusals, refused allocations, other contexts ----
def test_refusals_leave_the_output_and_the_context_alone(prover, batch130):
    m, m1 = made(prover, "2^3"), made(prover, "one_public")
    lib, h = prover.lib, m["verifier"].handle
    blob = np.frombuffer(batch130[0][3], np.uint8).copy()
    pubw = publics_words(batch130[0][2])
    out = np.full(1, 9, np.uint8)
    bp, pp, op = blob.ctypes.data_as(u8p), pubw.ctypes.data_as(u64p), out.ctypes.data_as(u8p)
    for args, msg in (((None, bp, pp, 1, 0, op), "verifier is NULL"),
                      ((h, None, pp, 1, 0, op), "NULL argument"),
                      ((h, bp, pp, 1, 0, None), "NULL argument"),
                      ((h, bp, pp, 0, 0, op), "at least 1"),
                      ((h, bp, pp, 1, 4, op), "unknown flag"),
                      ((h, bp, None, 1, 0, op), "public_inputs_host is NULL")):
        assert lib.cp_groth16_verify_city_bls12381(prover.ctx, *args) == -1, msg
        assert msg.encode() in lib.cp_last_error(prover.ctx), msg
        assert out[0] == 9
    assert m["verifier"].verify_city([batch130[0][3]], pubw[None]).tolist() == [0]
    import cityprover as cp
    assert m1["verifier"].verify_city([cp.groth16_pack_city(*m1["proof"])]).tolist() == [0]      # no public input: NULL is fine
    words, st = np.full(48, 9, np.uint64), np.full(1, 9, np.uint8)
    wp, sp = words.ctypes.data_as(u64p), st.ctypes.data_as(u8p)
    for args, msg in (((None, 1, wp, sp), "NULL argument"), ((bp, 1, None, sp), "NULL argument"), ((bp, 1, wp, None), "NULL argument"),
                      ((bp, 0, wp, sp), "at least 1"), ((bp, (1 << 24) // 3 + 1, wp, sp), "2^24 / 3")):
        assert lib.cp_groth16_proofs_unpack_city_bls12381(prover.ctx, *args) == -1, msg
        assert msg.encode() in lib.cp_last_error(prover.ctx), msg
        assert (words == 9).all() and st[0] == 9
    assert cp.groth16_unpack_city_batch(prover, [batch130[0][3]])[1].tolist() == [0]


def walk(prover, lib, call, want):
    """cp_fault_inject(CP_FAULT_DEVMEM, i) for every i until the call gets through: each refusal is out of memory, and the same
    context succeeds straight afterwards. Returns the number of refusals. (The pool is emptied first: a refused allocation is
    tried again after the pool has given back what it holds, and the injected refusal fires once.)"""
    import cityprover as cp
    refused = 0
    try:
        for i in range(MAX_WALK):
            cp.batch_pool_trim(prover)
            assert lib.cp_fault_inject(DEVMEM, i) == 0
            try:
                got = call()
            except cp.CityProverError as e:
                lib.cp_fault_inject(DEVMEM, -1)
                assert "[-4]" in str(e) and "out of memory" in str(e), (i, str(e))
                refused += 1
                assert call().tolist() == want
                continue
            lib.cp_fault_inject(DEVMEM, -1)
            assert got.tolist() == want
            return refused
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    pytest.fail("the walk did not end")


def test_injected_allocation_failures(prover, batch130):
    import cityprover as cp
    lib = cp.load_library()
    m = made(prover, "2^3")
    blobs = [it[3] for it in batch130[:2]]
    pubs = np.stack([publics_words(it[2]) for it in batch130[:2]])
    assert walk(prover, lib, lambda: m["verifier"].verify_city(blobs, pubs), [0, 0]) == 1      # the one allocation of a call
    assert walk(prover, lib, lambda: cp.groth16_unpack_city_batch(prover, blobs)[1], [0, 0]) == 1


def test_a_verifier_serves_other_contexts_and_outlives_its_own(prover, batch130):
    import cityprover as cp
    m = made(prover, "2^3")
    p = cp.Prover(0)
    v = cp.Groth16Verifier.from_key(p, m["key"])
    blobs, pubs = [batch130[0][3]], publics_words(batch130[0][2])[None]
    assert v.verify_city(blobs, pubs, prover=prover).tolist() == [0]
    p.close()
    assert v.verify_city(blobs, pubs, prover=prover).tolist() == [0]
    v.close()
