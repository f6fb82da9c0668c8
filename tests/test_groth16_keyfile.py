"""Groth16 key files at the C ABI, without a GPU: the three entry points are declared, exported and bound; NULL and zero
arguments give a status and a message without a context; cp_groth16_key_file_info reads files this test writes itself for a
key of 8 constraints (tests/groth16_keyfile_cases.py: every point from the trapdoor, the layout from its description) and
refuses every malformed variant with a status - never a crash. The code one lane of the key-file kernels runs - a point from
the file's form to the key's and back (csrc/groth16_keyfile.h) - is built for the CPU (tests/keyfilesim) and held against the
same Python points and against every spoiled point the GPU test writes into a file."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cityprover
import groth16_keyfile_cases as KC
import groth16_setup_cases as GC
import pairing_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cp_groth16_key_save_file", "cp_groth16_key_load_file", "cp_groth16_key_file_info")
INVALID_ARG, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def case():
    return GC.small_case(8, 3, 3, 108, unused_public=True)   # the last public wire occurs nowhere: an IC point at infinity


@pytest.fixture(scope="module")
def good(case):
    return {raw: KC.build_file(case, raw) for raw in (False, True)}


def info_rc(path, verify=1):
    lib = cityprover.load_library()
    info, vk = cityprover.Groth16KeyFileInfo(), cityprover.Groth16Vk()
    rc = lib.cp_groth16_key_file_info(os.fsencode(str(path)), verify, ctypes.byref(info), ctypes.byref(vk), None, None)
    return rc, lib.cp_last_error(None).decode()


def write(tmp_path, data, name="key.cpg16"):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def test_the_entry_points_are_declared_exported_and_bound():
    lib = cityprover.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cityprover.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert hasattr(lib, s), s
        assert s in cityprover.ABI, s
        assert "pub fn " + s + "(" in ffi, s
    assert lib.cp_abi_version() == 4
    for name in ("CP_GROTH16_KEY_FILE_VERSION 1", "CP_GROTH16_KEY_FILE_RAW 1u", "CP_GROTH16_KEY_LOAD_CHECK_TORSION 1u"):
        assert "#define " + name in hdr, name
    for m in ("save", "load"):
        assert hasattr(cityprover.Groth16Key, m), m
    assert hasattr(cityprover, "groth16_key_file_info")


def test_the_ctypes_mirror_has_the_size_the_c_compiler_gives(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cityprover.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(struct cp_groth16_key_file_info), '
                   'offsetof(struct cp_groth16_key_file_info, n_wires), offsetof(struct cp_groth16_key_file_info, checksum)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    I = cityprover.Groth16KeyFileInfo
    assert got == [ctypes.sizeof(I), I.n_wires.offset, I.checksum.offset]


def test_null_and_zero_arguments_give_a_status_and_a_message_without_a_context(tmp_path):
    lib = cityprover.load_library()
    assert lib.cp_groth16_key_save_file(None, None, None, 0, 0) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_groth16_key_save_file(None, None, os.fsencode(str(tmp_path / "x")), 0, 0) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert not (tmp_path / "x").exists()
    assert not lib.cp_groth16_key_load_file(None, None, 0, 0)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert not lib.cp_groth16_key_load_file(None, os.fsencode(str(tmp_path / "x")), 0, 0)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_groth16_key_file_info(None, 1, None, None, None, None) == INVALID_ARG
    assert b"path is NULL" in lib.cp_last_error(None)
    rc, msg = info_rc(tmp_path / "does" / "not" / "exist")
    assert rc == INVALID_ARG and "No such file" in msg          # errno's text


@pytest.mark.parametrize("raw", [False, True])
def test_file_info_returns_the_fields_the_verifying_key_and_the_ic(tmp_path, case, good, raw):
    data = good[raw]
    path = write(tmp_path, data)
    pts = KC.key_points(case)
    m, n_pub = case["system"]["n_wires"], case["n_pub"]
    got = cityprover.groth16_key_file_info(path)
    assert (got["version"], got["flags"], got["log_domain"], got["n_wires"], got["n_public"], got["n_private"], got["file_bytes"]) == \
        (1, int(raw), 3, m, n_pub, m - n_pub, len(data))
    assert got["checksum"] == KC.checksum(np.frombuffer(data, np.uint64)) == int(np.frombuffer(data, np.uint64)[2])
    vk = got["vk"]
    assert vk.n_public == n_pub
    assert list(vk.alpha_g1) == PC.g1_words(pts["alpha_g1"]).tolist()
    for name in ("beta_g2", "gamma_g2", "delta_g2"):
        assert list(getattr(vk, name)) == PC.g2_words(pts[name]).tolist(), name
    assert got["ic_inf"].tolist() == [0, 0, 1] == [int(pt is None) for pt in pts["ic"]]
    assert got["ic_xy"].tolist() == [PC.g1_words(pt if pt is not None else pts["G1"]).tolist() for pt in pts["ic"]]
    # every out pointer may be NULL
    assert cityprover.load_library().cp_groth16_key_file_info(os.fsencode(str(path)), 1, None, None, None, None) == 0


def header_edit(data, word, value):
    w = np.frombuffer(data, np.uint64).copy()
    w[word] = value
    return KC.with_checksum(w.tobytes())


def test_file_info_refuses_a_malformed_header(tmp_path, case, good):
    data = good[False]
    m = case["system"]["n_wires"]
    p_words = [(PC.P >> (64 * i)) & PC.MASK for i in range(6)]
    variants = [("magic", header_edit(data, 0, KC.MAGIC ^ 1), INVALID_ARG, "bad magic"),
                ("version", header_edit(data, 1, 2), UNSUPPORTED, "version 2"),
                ("flag", header_edit(data, 3, 2), INVALID_ARG, "reserved flag"),
                ("flag high", header_edit(data, 3, 1 << 63), INVALID_ARG, "reserved flag"),
                ("n_public 0", header_edit(data, 6, 0), INVALID_ARG, "n_public out of range"),
                ("n_public above", header_edit(data, 6, m + 1), INVALID_ARG, "n_public out of range"),
                ("log_domain 0", header_edit(data, 4, 0), INVALID_ARG, "log_domain out of range"),
                ("log_domain 29", header_edit(data, 4, 29), INVALID_ARG, "log_domain out of range"),
                ("n_wires 0", header_edit(data, 5, 0), INVALID_ARG, "n_wires out of range"),
                ("word 7", header_edit(data, 7, 1), INVALID_ARG, "word 7"),
                ("short", KC.with_checksum(data[:-8]), INVALID_ARG, "its header needs"),
                ("long", KC.with_checksum(data + bytes(8)), INVALID_ARG, "its header needs")]
    # a header point >= p: each of the six single points in turn, x = p exactly, and an IC coordinate
    for name, word in (("alpha_g1", 8), ("beta_g1", 20 + 6), ("delta_g1", 32), ("beta_g2", 44 + 18), ("delta_g2", 68 + 6), ("gamma_g2", 92 + 12)):
        d = data
        for i, v in enumerate(p_words):
            d = header_edit(d, word + i, v)
        variants.append((name + " = p", d, INVALID_ARG, name + " has a coordinate that is not canonical"))
    d = data
    for i, v in enumerate(p_words):
        d = header_edit(d, KC.FIXED_WORDS + 12 + 6 + i, v)     # y of ic[1]
    variants.append(("ic = p", d, INVALID_ARG, r"ic\[1\] has a coordinate that is not canonical"))
    for name, d, rc_want, msg_want in variants:
        rc, msg = info_rc(write(tmp_path, d))
        assert rc == rc_want and re.search(msg_want, msg), (name, rc, msg)
    assert info_rc(write(tmp_path, data))[0] == 0


@pytest.mark.parametrize("raw", [False, True])
def test_file_info_refuses_a_cut_at_every_section_boundary_and_a_flipped_payload_bit(tmp_path, case, good, raw):
    data = good[raw]
    lay = KC.layout(3, case["system"]["n_wires"], case["n_pub"], raw)
    cuts = [0, 8, 64, KC.FIXED_WORDS * 8, lay["ic_flags"]] + [lay[s][0] for s in KC.SETS] + [lay["total"] - 8]
    for cut in cuts:
        rc, msg = info_rc(write(tmp_path, data[:cut]))
        assert rc == INVALID_ARG and ("truncated" in msg or "its header needs" in msg), (cut, rc, msg)
    # one bit of the payload, in every set: refused with the checksum, accepted without (the parameter's documented meaning)
    for s in KC.SETS:
        off, n, size = lay[s]
        if n == 0:
            continue
        flipped = bytearray(data)
        flipped[off + size // 2] ^= 4
        path = write(tmp_path, bytes(flipped))
        rc, msg = info_rc(path, verify=1)
        assert rc == INVALID_ARG and "checksum mismatch" in msg, (s, rc, msg)
        assert info_rc(path, verify=0)[0] == 0, s


def test_no_header_bit_and_no_truncation_crashes_the_parser(tmp_path, good):
    """one bit in every word of the header and of the IC section, and a cut at every multiple of 8 bytes: a status or an
    accepted parse each time, and the process is still alive at the end"""
    lib = cityprover.load_library()
    data = good[False]
    head_words = KC.FIXED_WORDS + 12 * 3 + 1
    path = tmp_path / "mutant.cpg16"
    outcomes = {}
    for word in range(head_words):
        for bit in (0, 31, 63):
            m = bytearray(data)
            m[8 * word + bit // 8] ^= 1 << (bit % 8)
            for d in (bytes(m), KC.with_checksum(bytes(m))):
                path.write_bytes(d)
                for verify in (0, 1):
                    rc = lib.cp_groth16_key_file_info(os.fsencode(str(path)), verify, None, None, None, None)
                    assert rc in (0, INVALID_ARG, UNSUPPORTED), (word, bit, rc)
                    outcomes[rc] = outcomes.get(rc, 0) + 1
    for cut in range(0, len(data), 8):
        path.write_bytes(data[:cut])
        rc = lib.cp_groth16_key_file_info(os.fsencode(str(path)), 1, None, None, None, None)
        assert rc == INVALID_ARG, cut
    assert outcomes.get(0, 0) > 0 and outcomes.get(INVALID_ARG, 0) > 0 and outcomes.get(UNSUPPORTED, 0) > 0
    path.write_bytes(data)
    assert lib.cp_groth16_key_file_info(os.fsencode(str(path)), 1, None, None, None, None) == 0


# ---- the per-lane code of the key-file kernels on the CPU (tests/keyfilesim) ------------------------------------------------
u8p, u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
CLASS_CODE = {"flag": 1, "range": 2, "no_point": 3}      # the classes a point has on its own; the others depend on its set


@pytest.fixture(scope="module")
def ks():
    import sys
    import simlibs
    lib = ctypes.CDLL(simlibs.build("keyfilesim"))
    for f in (lib.ks_unpack_g1, lib.ks_unpack_g2):
        f.argtypes, f.restype = [u8p, ctypes.c_int, u64p, ctypes.POINTER(ctypes.c_int)], ctypes.c_int
    for f in (lib.ks_pack_g1, lib.ks_pack_g2):
        f.argtypes, f.restype = [u64p, ctypes.c_int, ctypes.c_int, u8p], None
    return lib


@pytest.fixture(scope="module")
def case32():
    return GC.small_case(32, 3, 6, 232, a_only=True, b_only=True, unused_public=True)


def ks_unpack(ks, g2, blob, raw):
    """(class, is_inf, the point or None)"""
    src = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
    xy, inf = np.zeros(24 if g2 else 12, np.uint64), ctypes.c_int(-1)
    st = (ks.ks_unpack_g2 if g2 else ks.ks_unpack_g1)(src, int(raw), xy.ctypes.data_as(u64p), ctypes.byref(inf))
    val = lambda a: sum(int(v) << (64 * j) for j, v in enumerate(a))
    if st != 0 or inf.value:
        return st, inf.value, None
    c = [val(xy[6 * k:6 * k + 6]) for k in range(len(xy) // 6)]
    return st, 0, ((c[0], c[1]), (c[2], c[3])) if g2 else (c[0], c[1])


def ks_pack(ks, g2, pt, raw):
    n = (96 if g2 else 48) * (2 if raw else 1)
    out = (ctypes.c_uint8 * n)()
    words = (PC.g2_words if g2 else PC.g1_words)(pt if pt is not None else (PC.PR.G2 if g2 else PC.PR.G1))     # under a flag the entry holds the generator
    (ks.ks_pack_g2 if g2 else ks.ks_pack_g1)(words.ctypes.data_as(u64p), int(pt is None), int(raw), out)
    return bytes(out)


@pytest.mark.parametrize("raw", [False, True])
def test_every_point_of_a_file_unpacks_to_its_point_and_packs_to_its_bytes(ks, case32, raw):
    """the code of one lane of k_unpack and of k_pack on every point of a key with infinities in a_g1, b_g1 and b_g2: both roots occur"""
    data, lay, pts = KC.build_file(case32, raw), KC.layout(5, case32["system"]["n_wires"], 3, raw), KC.key_points(case32)
    tops = set()
    for s in KC.SETS:
        off, n, size = lay[s]
        for i in range(n):
            blob, want = data[off + i * size:off + (i + 1) * size], pts[s][i]
            assert ks_unpack(ks, s == "b_g2", blob, raw) == (0, int(want is None), want), (s, i)
            assert ks_pack(ks, s == "b_g2", want, raw) == blob, (s, i)
            tops.add((s == "b_g2", blob[-1] & 0xC0))
    if not raw:
        assert tops == {(g2, t) for g2 in (False, True) for t in (0, 0x40, 0x80)}


def test_every_spoiled_point_gets_its_class(ks, case32):
    """the edits the GPU test makes to whole files, point by point: flag, range and no-point are classes of the point alone;
    infinity and a finite point that only their set refuses come out as what they are"""
    seen = set()
    for label, raw, changes, (cls, s_bad, i_bad) in KC.refusal_edits(case32):
        for s, idx, new in changes:
            st, inf, pt = ks_unpack(ks, s == "b_g2", new, raw)
            if (s, idx) == (s_bad, i_bad) and cls in CLASS_CODE:
                assert st == CLASS_CODE[cls], (label, s, idx, st)
                seen.add(cls)
            elif cls in ("infinity", "disagree") and len(changes) == 1:
                assert st == 0, (label, st)
                seen.add("inf" if inf else "finite")
    assert seen == {"flag", "range", "no_point", "inf", "finite"}
    # the outside-torsion points of the GPU test are points of the curve and the twist: accepted here, in both forms
    for g2, pt in ((False, PC.g1_outside_torsion()), (True, PC.g2_outside_torsion())):
        for raw, enc in ((False, KC.g2_compressed if g2 else KC.g1_compressed), (True, KC.g2_raw if g2 else KC.g1_raw)):
            assert ks_unpack(ks, g2, enc(pt), raw) == (0, 0, pt)
