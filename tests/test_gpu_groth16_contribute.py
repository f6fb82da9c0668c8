"""cp_groth16_key_contribute_bls12381 and cp_groth16_key_check_contribution_bls12381 against the trapdoor: a contribution d on a
key of trapdoor delta must be, byte for byte, the key cp_groth16_setup_bls12381 returns for delta d mod r; and the check must
accept exactly the pairs that are such a step. Tampered keys are made through the raw key-file route: save, splice, fix the
checksum (tests/groth16_keyfile_cases.py), load."""
import numpy as np
import pytest

import groth16_keyfile_cases as KC
import groth16_setup_cases as GC
import groth16_srs_cases as SC
import oracle_lib as O
import pairing_cases as PC
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
R = GC.R
D255 = int.from_bytes(np.random.default_rng(255).bytes(32), "little") % (1 << 254) | (1 << 254)   # a seeded 255-bit value
assert D255.bit_length() == 255 and D255 < R


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


def weights_for(key, seed=9):
    pk = key.pk()
    n = pk.n_private + (1 << pk.log_domain) - 1
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(16), "little") | 1 for _ in range(n)]


def verdict(prover, before, after, weights=None):
    import cityprover as cp
    return cp.Groth16Key.check_contribution(prover, before, after, weights_for(before) if weights is None else weights)


def with_delta(case, d):
    return dict(case["td"], delta=case["td"]["delta"] * d % R)


@pytest.fixture(scope="module")
def base(prover):
    case = SC.case_of("2^5")
    key = SC.setup_trapdoor(prover, case)
    yield case, key
    key.free()


@pytest.mark.parametrize("d", [1, 2, R - 1, D255], ids=["1", "2", "r-1", "255-bit"])
def test_a_contribution_is_the_key_of_the_multiplied_delta(prover, base, d):
    case, key = base
    before = SC.key_bytes(key)
    out = key.contribute(d)
    ref = SC.setup_trapdoor(prover, case, td=with_delta(case, d))
    try:
        assert SC.key_bytes(out) == SC.key_bytes(ref)
        assert SC.key_bytes(key) == before                # the input key is not modified
        assert verdict(prover, key, out)[0] == 0
        assert verdict(prover, key, ref)[0] == 0           # a key is a key, whoever made it
        if d != 1:
            assert SC.key_bytes(out)[0][3] != before[0][3] and SC.key_bytes(out)[0][4] != before[0][4]   # K and Z moved
            assert SC.key_bytes(out)[0][:3] == before[0][:3] and SC.key_bytes(out)[0][5:] == before[0][5:]
    finally:
        out.free()
        ref.free()


def test_two_contributions_are_one_with_the_product(prover, base):
    case, key = base
    d1, d2 = 0x1234567, D255
    first = key.contribute(d1)
    second = first.contribute(d2)
    once = key.contribute(d1 * d2 % R)
    try:
        assert SC.key_bytes(second) == SC.key_bytes(once)
        assert verdict(prover, first, second)[0] == 0 and verdict(prover, key, second)[0] == 0
    finally:
        for k in (first, second, once):
            k.free()


def prove(prover, key, case, r, s):
    import cityprover as cp
    sysm = case["system"]
    h = cp.R1cs(prover, sysm["n"], sysm["n_wires"], RC.limbs4(sysm["coeffs"]), sysm["mats"])
    dw = prover.to_device(RC.limbs4(sysm["w"]))
    try:
        a, b, c = cp.groth16_prove_r1cs(prover, key.pk(), h, dw.ptr, r, s)
        return np.concatenate([PC.g1_words(a), PC.g2_words(b), PC.g1_words(c)])
    finally:
        dw.free()
        h.free()


def test_a_contribution_on_an_srs_key(prover):
    import cityprover as cp
    case = SC.case_of("2^3")
    d = D255
    srs = SC.make_srs(prover, SC.srs_arrays(prover, case["td"], 3))
    plain = SC.setup_srs(prover, case, srs)
    key = plain.contribute(d)
    ref = SC.setup_trapdoor(prover, case, td=dict(case["td"], gamma=1, delta=d))
    own, old = cp.Groth16Verifier.from_key(prover, key), cp.Groth16Verifier.from_key(prover, plain)
    try:
        assert SC.key_bytes(key) == SC.key_bytes(ref)
        assert verdict(prover, plain, key)[0] == 0
        r, s = (x % R for x in GC.random_scalars(2, 3))
        proof = prove(prover, key, case, r, s).reshape(1, 48)
        pub = RC.limbs4(case["system"]["w"][1:case["n_pub"]]).reshape(1, -1, 4)
        assert own.verify(proof, pub).tolist() == [0]
        assert old.verify(proof, pub).tolist() == [1]     # the uncontributed key's delta does not fit the proof
    finally:
        own.close()
        old.close()
        for k in (plain, key, ref):
            k.free()
        srs.free()


def test_a_contribution_with_no_private_wires(prover):
    case = SC.case_of("2^3")
    m = case["system"]["n_wires"]
    key = SC.setup_trapdoor(prover, case, n_pub=m)
    out = key.contribute(D255)
    ref = SC.setup_trapdoor(prover, case, td=with_delta(case, D255), n_pub=m)
    try:
        assert key.pk().n_private == 0
        a, b = SC.key_bytes(out), SC.key_bytes(ref)
        assert a == b
        assert a[0][4] != SC.key_bytes(key)[0][4] and a[1][2] != SC.key_bytes(key)[1][2]   # Z and delta_g1 still move
        assert verdict(prover, key, out)[0] == 0
    finally:
        for k in (key, out, ref):
            k.free()


def one_coefficient_changed(case, mat, wire):
    """the system with the coefficient of the first term of `wire` in matrix `mat` replaced by another value"""
    s = case["system"]
    mats = [tuple(a.copy() for a in M) for M in s["mats"]]
    t = int(np.nonzero(mats[mat][1] == wire)[0][0])
    coeffs = list(s["coeffs"]) + [(s["coeffs"][int(mats[mat][2][t])] + 12345) % R]
    mats[mat][2][t] = len(coeffs) - 1
    return dict(s, coeffs=coeffs, mats=mats)


def test_a_part_that_must_not_change_gives_verdict_1(prover, base):
    case, key = base
    s, n_pub = case["system"], case["n_pub"]
    private_in_a = int(next(w for w in s["mats"][0][1] if w >= n_pub))
    private_in_b = int(next(w for w in s["mats"][1][1] if w >= n_pub))
    public_in_a = int(next(w for w in s["mats"][0][1] if 0 < w < n_pub))
    for mat, wire, part in ((0, private_in_a, "a_g1"), (1, private_in_b, "b_g1"), (0, public_in_a, "IC")):
        other = SC.setup_trapdoor(prover, case, system=one_coefficient_changed(case, mat, wire))
        after = other.contribute(77)
        try:
            v, why = verdict(prover, key, after)
            assert v == 1 and "differs" in why, (part, v, why)
            if part == "IC":
                assert "IC point" in why
            assert verdict(prover, other, after)[0] == 0
        finally:
            other.free()
            after.free()
    # a wire that leaves B: b_inf differs
    mats = [tuple(a.copy() for a in M) for M in s["mats"]]
    coeffs = list(s["coeffs"]) + [0]
    mats[1][2][mats[1][1] == private_in_b] = len(coeffs) - 1
    other = SC.setup_trapdoor(prover, case, system=dict(s, coeffs=coeffs, mats=mats))
    after = other.contribute(78)
    try:
        assert SC.key_bytes(after)[0][6] != SC.key_bytes(key)[0][6]
        assert verdict(prover, key, after)[0] == 1
    finally:
        other.free()
        after.free()
    # keys of another size
    small = SC.setup_trapdoor(prover, SC.case_of("2^3"))
    try:
        v, why = verdict(prover, key, small)
        assert v == 1 and "sizes" in why
    finally:
        small.free()


def raw_file(key, tmp_path, name):
    path = str(tmp_path / name)
    key.save(path, raw=True)
    return bytearray(open(path, "rb").read())


def load_bytes(prover, data, tmp_path, name):
    import cityprover as cp
    path = str(tmp_path / name)
    open(path, "wb").write(KC.with_checksum(data))
    return cp.Groth16Key.load(prover, path)


DELTA_G1 = 8 * 8 + 2 * 96         # header, alpha_g1, beta_g1
DELTA_G2 = 8 * 8 + 3 * 96 + 192   # ..., delta_g1, beta_g2


def test_tampered_keys_get_verdicts_2_and_3(prover, base, tmp_path):
    case, key = base
    d, d_other = D255, 0xabcdef
    lay = KC.layout(case["exp"]["log_domain"], case["system"]["n_wires"], case["n_pub"], True)
    good, other, wrong_way = key.contribute(d), key.contribute(d_other), key.contribute(pow(d, -1, R))
    loaded = []
    try:
        f_good, f_other, f_wrong = (raw_file(k, tmp_path, "k%d" % i) for i, k in enumerate((good, other, wrong_way)))
        same = load_bytes(prover, f_good, tmp_path, "same")
        loaded.append(same)
        assert SC.key_bytes(same) == SC.key_bytes(good) and verdict(prover, key, same)[0] == 0
        # delta_g2 of one multiplier, delta_g1 of another
        mixed = bytearray(f_good)
        mixed[DELTA_G1:DELTA_G1 + 96] = f_other[DELTA_G1:DELTA_G1 + 96]
        assert mixed != f_good and mixed[DELTA_G2:DELTA_G2 + 192] == f_good[DELTA_G2:DELTA_G2 + 192]
        k = load_bytes(prover, mixed, tmp_path, "mixed")
        loaded.append(k)
        assert verdict(prover, key, k)[0] == 2
        # one K point, and separately one Z point, replaced by another point of the curve
        for name in ("k_g1", "z_g1"):
            off, n, size = lay[name]
            assert n >= 2 and size == 96
            swapped = bytearray(f_good)
            swapped[off + size:off + 2 * size] = f_good[off:off + size]          # point 1 := point 0
            assert swapped != f_good
            k = load_bytes(prover, swapped, tmp_path, "swapped_" + name)
            loaded.append(k)
            v, why = verdict(prover, key, k)
            assert v == 3, (name, v, why)
        # K scaled by d instead of 1 / d
        off, n, size = lay["k_g1"]
        scaled = bytearray(f_good)
        scaled[off:off + n * size] = f_wrong[off:off + n * size]
        k = load_bytes(prover, scaled, tmp_path, "scaled")
        loaded.append(k)
        assert verdict(prover, key, k)[0] == 3
        # a delta outside the r-torsion
        outside = bytearray(f_good)
        outside[DELTA_G1:DELTA_G1 + 96] = KC.g1_raw(PC.g1_outside_torsion())
        k = load_bytes(prover, outside, tmp_path, "outside")
        loaded.append(k)
        assert verdict(prover, key, k)[0] == 4
    finally:
        for k in [good, other, wrong_way] + loaded:
            k.free()


def test_bad_weights_and_bad_scalars_are_refused(prover, base):
    import cityprover as cp
    case, key = base
    out = key.contribute(5)
    try:
        w = weights_for(key)
        w[7] = 0
        with pytest.raises(cp.CityProverError, match=r"\[-1\] contribution check: weight 7 is zero"):
            verdict(prover, key, out, w)
        with pytest.raises(cp.CityProverError, match=r"\[-1\] contribution check: weights is NULL"):
            cp.Groth16Key.check_contribution(prover, key, out, None)
        assert verdict(prover, key, out)[0] == 0
    finally:
        out.free()
    for d, msg in ((0, "contribution: d is zero"), (R, r"contribution: d is not canonical \(>= r\)"), (2**256 - 1, "d is not canonical")):
        with pytest.raises(cp.CityProverError, match=msg):
            key.contribute(d)
    again = key.contribute(1)                                 # the first case, on the same context
    try:
        assert SC.key_bytes(again) == SC.key_bytes(key)
    finally:
        again.free()
