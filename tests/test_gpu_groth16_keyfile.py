"""Groth16 keys as files (cp_groth16_key_save_file / cp_groth16_key_load_file): the file a key is saved to is, byte for byte, the
file tests/groth16_keyfile_cases.py builds from the trapdoor in Python integers - in neither direction does an expected byte come
from the code under test - and a key loaded from it is, byte for byte, the key that was saved, proves what it proves and verifies
what it verifies. Every refusal of the loader names the set and the lowest index, and leaves the context able to load the good
file. The injected allocation failures are refused allocations that return a status (the pattern of
tests/test_gpu_alloc_faults.py): nothing here faults the device."""
import os
import re

import numpy as np
import pytest

import groth16_keyfile_cases as KC
import groth16_setup_cases as GC
import oracle_lib as O
import pairing_cases as PC
import r1cs_cases as RC

pytestmark = pytest.mark.gpu
R, P = GC.R, PC.P
DEVMEM = 3   # CP_FAULT_DEVMEM
MAX_WALK = 48
NAMES = ("2^3", "2^5", "sat", "2^7")
_cases = {}


def case_of(name):
    if name not in _cases:
        _cases[name] = {"2^3": lambda: GC.small_case(8, 3, 3, 208),
                        "2^5": lambda: GC.small_case(32, 3, 6, 232, a_only=True, b_only=True, unused_public=True),
                        "sat": lambda: GC.satisfied_case(64, 64, 3),       # real infinity patterns in the A and B queries
                        "2^7": lambda: GC.small_case(128, 2, 3, 228)}[name]()   # 133 wires, 127 Z points: lanes cross 64 and 128
    return _cases[name]


@pytest.fixture(scope="module")
def prover():
    import cityprover
    p = cityprover.Prover(0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def keys(prover):
    """the keys of the cases, set up on first use and freed with the module"""
    import cityprover as cp
    made = {}

    def get(name):
        if name not in made:
            case = case_of(name)
            s = case["system"]
            made[name] = cp.Groth16Key.setup(prover, s["n"], s["n_wires"], RC.limbs4(s["coeffs"]), s["mats"], case["n_pub"], **case["td"])
        return made[name]
    yield get
    for k in made.values():
        k.free()


def key_bytes(key):
    """everything the key holds, as bytes: the five point arrays and the two flag arrays as they lie on the device, the single points"""
    pk, sets = key.pk(), key.point_sets()
    raw = [sets[k].buf.download().tobytes() for k in KC.SETS] + [sets["a_inf"].tobytes(), sets["b_inf"].tobytes()]
    singles = [bytes(bytearray(getattr(pk, f))) for f in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")]
    return raw, singles, (pk.n_wires, pk.n_private, pk.log_domain), repr(key.vk())


def lay_of(case, raw=False):
    return KC.layout(case["exp"]["log_domain"], case["system"]["n_wires"], case["n_pub"], raw)


# ---- the file is what the definition says ----
@pytest.mark.parametrize("raw", [False, True], ids=["compressed", "raw"])
@pytest.mark.parametrize("name", NAMES)
def test_the_saved_file_is_the_file_built_from_the_trapdoor(prover, keys, tmp_path, name, raw):
    path = tmp_path / "key.cpg16"
    keys(name).save(path, raw=raw)
    got, want = path.read_bytes(), KC.build_file(case_of(name), raw)
    assert len(got) == len(want)
    assert got[:64] == want[:64], "header (checksum included)"
    assert got == want
    assert os.listdir(tmp_path) == ["key.cpg16"]      # no temporary file stays behind


def test_the_cases_reach_both_roots_and_every_infinity():
    """across the cases both values of the 0x80 bit occur in G1 and in G2, and 0x40 occurs in a_g1, b_g1 and b_g2: asserted on
    the files built in Python, which the saved files were just held against"""
    seen = {}
    for name in NAMES:
        case = case_of(name)
        data, lay = KC.build_file(case), lay_of(case)
        for s in KC.SETS:
            off, n, size = lay[s]
            for i in range(n):
                top = data[off + (i + 1) * size - 1]
                seen.setdefault((s, top & 0xC0), 0)
                seen[(s, top & 0xC0)] += 1
    for s in KC.SETS:
        assert seen.get((s, 0x80), 0) > 0 and seen.get((s, 0x00), 0) > 0, s    # G1: four sets; G2: b_g2
    for s in ("a_g1", "b_g1", "b_g2"):
        assert seen.get((s, 0x40), 0) > 0, s
    for s in ("k_g1", "z_g1"):
        assert (s, 0x40) not in seen


# ---- round trip ----
def prove(p, key, case, r, s, out=None):
    import cityprover as cp
    sysm = case["system"]
    h = cp.R1cs(p, sysm["n"], sysm["n_wires"], RC.limbs4(sysm["coeffs"]), sysm["mats"])
    dw = p.to_device(RC.limbs4(sysm["w"]))
    try:
        return cp.groth16_prove_r1cs(p, key.pk(), h, dw.ptr, r, s, out)
    finally:
        dw.free()
        h.free()


@pytest.mark.parametrize("name", NAMES)
def test_a_loaded_key_is_the_saved_key(prover, keys, tmp_path, name):
    import cityprover as cp
    case, key = case_of(name), keys(name)
    want = key_bytes(key)
    G1, G2 = O.bls_constants()[2], O.bls_g2_generator()
    r, s = (x % R for x in GC.random_scalars(2, 91))
    logs = GC.proof_logs(case["system"], case["n_pub"], case["td"], case["exp"], r, s)     # asserts the verification equation
    proof_want = (O.bls_g1_mul(G1, logs[0]), O.bls_g2_mul(G2, logs[1]), O.bls_g1_mul(G1, logs[2]))
    p2 = cp.Prover(0)          # a second context of the same device
    loaded = []
    try:
        for raw in (False, True):
            path = tmp_path / ("key%d.cpg16" % raw)
            key.save(path, raw=raw)
            loaded.append(cp.Groth16Key.load(p2, path))
            assert key_bytes(loaded[-1]) == want, "raw" if raw else "compressed"
            assert loaded[-1].vk() == key.vk()
        out = (np.zeros(12, np.uint64), np.zeros(24, np.uint64), np.zeros(12, np.uint64))
        assert prove(prover, key, case, r, s) == proof_want
        assert prove(p2, loaded[0], case, r, s, out) == proof_want
        v = cp.Groth16Verifier.from_key(p2, loaded[0])
        try:
            proof = np.concatenate(out)
            publics = np.array(RC.limbs4(case["system"]["w"][1:case["n_pub"]]), np.uint64).reshape(1, case["n_pub"] - 1, 4)
            altered = np.concatenate([out[2], out[1], out[0]])        # A and C exchanged: three points of the groups, another equation
            assert v.verify(np.stack([proof, altered]), np.concatenate([publics, publics])).tolist() == [0, 1]
        finally:
            v.close()
    finally:
        p2.close()             # the loaded keys outlive their context
        for k in loaded:
            k.free()
            k.free()           # and a second free does nothing


# ---- chunking ----
@pytest.mark.parametrize("chunk", [1, 5, 64, 0])
def test_every_chunk_size_gives_the_same_file_and_the_same_key(prover, keys, tmp_path, chunk):
    """133 wires and 127 Z points: 5 splits every set in the middle of a pass, 64 leaves a last pass of 5 and of 63"""
    import cityprover as cp
    case, key = case_of("2^7"), keys("2^7")
    want = key_bytes(key)
    for raw in (False, True):
        path = tmp_path / ("key%d.cpg16" % raw)
        key.save(path, raw=raw, chunk_points=chunk)
        assert path.read_bytes() == KC.build_file(case, raw)
        loaded = cp.Groth16Key.load(prover, path, chunk_points=chunk)
        try:
            assert key_bytes(loaded) == want
        finally:
            loaded.free()


# ---- refusals on load ----
def test_refused_points_are_named_and_the_context_loads_the_good_file(prover, keys, tmp_path):
    import cityprover as cp
    case, key = case_of("2^5"), keys("2^5")
    want = key_bytes(key)
    good = {raw: KC.build_file(case, raw) for raw in (False, True)}
    good_paths = {}
    for raw in good:
        good_paths[raw] = tmp_path / ("good%d.cpg16" % raw)
        good_paths[raw].write_bytes(good[raw])
    bad_path = tmp_path / "bad.cpg16"
    edits = KC.refusal_edits(case)
    for n, (label, raw, changes, (cls, s_bad, i_bad)) in enumerate(edits):
        msg = r"%s\[%d\] %s" % (s_bad, i_bad, KC.CLASS_TEXT[cls])
        data, lay = good[raw], lay_of(case, raw)
        for s, idx, new in changes:
            off, size = KC.point_at(data, lay, s, idx)
            assert len(new) == size and data[off:off + size] != new, (label, s, idx)
            data = KC.replace(data, off, new)
        bad_path.write_bytes(KC.with_checksum(data))      # so that the point checks are reached
        with pytest.raises(cp.CityProverError, match=msg):
            cp.Groth16Key.load(prover, bad_path, chunk_points=5).free()
        k = cp.Groth16Key.load(prover, good_paths[raw], chunk_points=5)      # the same context, straight afterwards
        try:
            assert k.vk() == key.vk()
            if n % 6 == 0:
                assert key_bytes(k) == want
        finally:
            k.free()


def test_unknown_flags_and_a_missing_file_are_refused(prover, keys, tmp_path):
    import cityprover as cp
    lib, key = prover.lib, keys("2^3")
    path = tmp_path / "key.cpg16"
    assert lib.cp_groth16_key_save_file(prover.ctx, key.handle, os.fsencode(str(path)), 2, 0) == -1
    assert b"unknown flag bits" in lib.cp_last_error(None) and not path.exists()
    assert lib.cp_groth16_key_save_file(prover.ctx, None, os.fsencode(str(path)), 0, 0) == -1
    assert lib.cp_groth16_key_save_file(prover.ctx, key.handle, None, 0, 0) == -1
    key.save(path)
    assert not lib.cp_groth16_key_load_file(prover.ctx, os.fsencode(str(path)), 2, 0)
    assert b"unknown flag bits" in lib.cp_last_error(None)
    assert not lib.cp_groth16_key_load_file(prover.ctx, None, 0, 0)
    with pytest.raises(cp.CityProverError, match="No such file"):
        cp.Groth16Key.load(prover, tmp_path / "absent.cpg16")
    cp.Groth16Key.load(prover, path).free()


# ---- checksum ----
def test_a_flipped_bit_is_a_checksum_mismatch_whatever_it_hit(prover, tmp_path):
    import cityprover as cp
    case = case_of("2^3")
    path = tmp_path / "flipped.cpg16"
    for raw in (False, True):
        data, lay = KC.build_file(case, raw), lay_of(case, raw)
        # a header point, an IC point, an IC flag, a point of every set (its flag byte: the point checks would refuse it too), the last byte
        spots = [8 * 8, 8 * 50 + 3, lay["ic"] + 5, lay["ic_flags"]] + [lay[s][0] + lay[s][2] - 1 for s in KC.SETS] + [lay["total"] - 1]
        for at in spots:
            m = bytearray(data)
            m[at] ^= 0x40
            path.write_bytes(bytes(m))
            with pytest.raises(cp.CityProverError, match="checksum mismatch"):
                cp.Groth16Key.load(prover, path).free()
    path.write_bytes(data)
    cp.Groth16Key.load(prover, path).free()


# ---- torsion ----
def test_points_outside_the_r_torsion_are_refused_only_when_asked(prover, keys, tmp_path):
    import cityprover as cp
    case, key = case_of("2^3"), keys("2^3")
    want = key_bytes(key)
    i = [n for n, x in enumerate(case["exp"]["u"]) if x][-1]
    j = [n for n, x in enumerate(case["exp"]["v"]) if x][-1]
    out1, out2 = PC.g1_outside_torsion(), PC.g2_outside_torsion()
    path = tmp_path / "key.cpg16"
    for raw in (False, True):
        good, lay = KC.build_file(case, raw), lay_of(case, raw)
        e1, e2 = (KC.g1_raw, KC.g2_raw) if raw else (KC.g1_compressed, KC.g2_compressed)
        for s, idx, new in (("a_g1", i, e1(out1)), ("b_g2", j, e2(out2))):
            path.write_bytes(KC.with_checksum(KC.replace(good, KC.point_at(good, lay, s, idx)[0], new)))
            with pytest.raises(cp.CityProverError, match=r"%s\[%d\] is outside the r-torsion" % (s, idx)):
                cp.Groth16Key.load(prover, path, check_torsion=True).free()
            k = cp.Groth16Key.load(prover, path)          # without the flag: accepted, the flag's documented meaning
            try:
                got = k.point_sets()[s].to_host([idx])[0]
                assert got == (out1 if s == "a_g1" else out2)
            finally:
                k.free()
        path.write_bytes(good)
        for check in (True, False):
            k = cp.Groth16Key.load(prover, path, check_torsion=check, chunk_points=5)
            try:
                assert key_bytes(k) == want, (raw, check)
            finally:
                k.free()


# ---- the save side ----
def test_a_failed_save_leaves_the_old_file_and_no_temporary_file(prover, keys, tmp_path):
    import cityprover as cp
    lib, key = prover.lib, keys("2^3")
    with pytest.raises(cp.CityProverError, match=r"^\[-1\].*No such file"):
        key.save(tmp_path / "no" / "such" / "directory" / "key.cpg16")
    assert os.listdir(tmp_path) == []
    path = tmp_path / "key.cpg16"
    key.save(path, raw=True)
    old = path.read_bytes()
    assert old == KC.build_file(case_of("2^3"), True)
    refused = 0
    try:
        for j in range(MAX_WALK):
            cp.batch_pool_trim(prover)
            assert lib.cp_fault_inject(DEVMEM, j) == 0
            try:
                key.save(path)                     # the compressed form over the raw file: the header is written before the staging is asked for
            except cp.CityProverError as e:
                lib.cp_fault_inject(DEVMEM, -1)
                assert str(e).startswith("[-4]") and re.search("(?i)memory", str(e)), (j, str(e))
                assert path.read_bytes() == old, j
                assert os.listdir(tmp_path) == ["key.cpg16"], j
                refused += 1
                continue
            lib.cp_fault_inject(DEVMEM, -1)
            break
        else:
            pytest.fail("the walk did not end before j = %d" % MAX_WALK)
    finally:
        lib.cp_fault_inject(DEVMEM, -1)
    assert refused >= 1
    assert path.read_bytes() == KC.build_file(case_of("2^3"), False)
    assert os.listdir(tmp_path) == ["key.cpg16"]


def test_injected_allocation_failures(prover, keys, tmp_path):
    """cp_fault_inject(CP_FAULT_DEVMEM, j) for every j until a save and a load both get through: each refusal is out of memory, the
    pool holds what it held, and the same context then saves the same file and loads the same key"""
    import cityprover as cp
    lib, key = prover.lib, keys("2^3")
    path = tmp_path / "key.cpg16"
    want = (KC.build_file(case_of("2^3"), False), key_bytes(key))

    def call_on(p):
        if path.exists():
            path.unlink()
        p._check(p.lib.cp_groth16_key_save_file(p.ctx, key.handle, os.fsencode(str(path)), 0, 5))
        k = cp.Groth16Key.load(p, path, check_torsion=True, chunk_points=5)
        try:
            return path.read_bytes(), key_bytes(k)
        finally:
            k.free()
    assert call_on(prover) == want
    refused = 0
    try:
        for j in range(MAX_WALK):
            p = cp.Prover(0)
            try:
                cp.batch_pool_trim(p)
                held = cp.batch_pool_stats(0)["bytes"]
                assert lib.cp_fault_inject(DEVMEM, j) == 0
                try:
                    got = call_on(p)
                except cp.CityProverError as e:
                    lib.cp_fault_inject(DEVMEM, -1)
                    assert re.search("(?i)out of memory", str(e)), (j, str(e))
                    if str(e).startswith("["):
                        assert str(e).startswith("[-4]"), (j, str(e))       # CP_ERR_OOM
                    assert cp.batch_pool_stats(0)["bytes"] == held, j
                    assert sorted(os.listdir(tmp_path)) in ([], ["key.cpg16"]), j
                    refused += 1
                    assert call_on(p) == want, "allocation %d refused: the context did not recover" % j
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
    assert refused >= 10   # the staging of the save; the key's seven arrays, the staging and the report word of the load
