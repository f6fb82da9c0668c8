"""The device-resident R1CS at the C ABI, without a GPU: the symbols exist and are bound, NULL handles give a status and a
message, the ctypes mirrors of the three structures have the size the C compiler gives them, and the host-side arithmetic the
kernels share (the one-limb multiplication, the limb split) agrees with Python integers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cityprover
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.bls_constants()[1]
NEW = ("cp_r1cs_bls12381_create", "cp_r1cs_bls12381_destroy", "cp_r1cs_bls12381_get_info", "cp_r1cs_bls12381_eval_dev",
       "cp_r1cs_bls12381_check_dev", "cp_groth16_prove_r1cs_bls12381")


def test_new_symbols_are_exported_and_bound():
    lib = cityprover.load_library()
    for s in NEW:
        assert s in cityprover.ABI, s
        assert hasattr(lib, s), s
    assert lib.cp_abi_version() == 4
    for name in ("R1csMatrix", "R1csDesc", "R1csInfo", "R1cs", "groth16_prove_r1cs"):
        assert hasattr(cityprover, name), name


def test_create_without_a_context_is_refused_without_touching_a_gpu():
    lib = cityprover.load_library()
    desc, keep = cityprover.r1cs_desc(1, 1, np.array([[1, 0, 0, 0]], np.uint64),
                                      [(np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([0], np.uint32))] * 3)
    assert not lib.cp_r1cs_bls12381_create(None, ctypes.byref(desc))
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert not lib.cp_r1cs_bls12381_create(None, None)
    assert b"ctx is NULL" in lib.cp_last_error(None)


def test_null_handles_give_a_status_and_a_message():
    lib = cityprover.load_library()
    n, first = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert lib.cp_r1cs_bls12381_eval_dev(None, None, None, None, None, None) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_r1cs_bls12381_check_dev(None, None, None, ctypes.byref(n), ctypes.byref(first)) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert (n.value, first.value) == (7, 7)
    assert lib.cp_groth16_prove_r1cs_bls12381(None, None, None, None, None, None, None, None, None) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    info = cityprover.R1csInfo()
    assert lib.cp_r1cs_bls12381_get_info(None, ctypes.byref(info)) != 0
    assert b"NULL" in lib.cp_last_error(None)
    lib.cp_r1cs_bls12381_destroy(None)      # a no-op


def test_ctypes_mirrors_have_the_sizes_the_c_compiler_gives(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "cityprover.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(cp_r1cs_matrix), sizeof(cp_r1cs_desc), sizeof(cp_r1cs_info)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(cityprover.R1csMatrix), ctypes.sizeof(cityprover.R1csDesc), ctypes.sizeof(cityprover.R1csInfo)]
    # and the fields sit where the header puts them: offsets of the last member of each
    assert cityprover.R1csDesc.flags.offset == 4 * ctypes.sizeof(ctypes.c_size_t) + 3 * ctypes.sizeof(cityprover.R1csMatrix)
    assert cityprover.R1csInfo.n_terms_class.offset + 6 * ctypes.sizeof(ctypes.c_size_t) == ctypes.sizeof(cityprover.R1csInfo)


# ---- the arithmetic of the kernels on the host (tests/r1cs_hostsim: the __host__ __device__ functions of csrc/r1cs.h) ----------
@pytest.fixture(scope="module")
def hs():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("r1cs_hostsim"))
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.hs_r1cs_mul_small.argtypes = [u64p, ctypes.c_uint32, u64p]
    lib.hs_r1cs_term.argtypes = [u64p, u64p, u64p, u64p]
    lib.hs_r1cs_classify.argtypes = [u64p, ctypes.POINTER(ctypes.c_uint32)]
    lib.hs_r1cs_classify.restype = ctypes.c_uint32
    return lib


def _limbs(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * i)) & (2**64 - 1) for i in range(4)])


def _val(a):
    return sum(int(a[i]) << (64 * i) for i in range(4))


def test_one_limb_product_is_exact(hs):
    """mul_small(w, c) = c w mod r for every edge of its quotient estimate: the largest constants on the largest values, values
    around multiples of r / c, and random ones"""
    rng = np.random.default_rng(7)
    cs = [2, 3, 7, 8, 12345, (1 << 27), (1 << 28) - 2, (1 << 28) - 1] + [int(x) for x in rng.integers(2, 1 << 28, 40)]
    ws = [0, 1, 2, R - 1, R - 2, R >> 1, (R >> 1) + 1, (1 << 224) - 1, 1 << 224, (1 << 252), (1 << 254), (1 << 28) - 1]
    ws += [int.from_bytes(rng.bytes(40), "little") % R for _ in range(200)]
    out = (ctypes.c_uint64 * 4)()
    for c in cs:
        edge = [(k * R) // c + d for k in (1, 2, c // 2, c - 1) for d in (-1, 0, 1)]    # c w just below / at / above a multiple of r
        for w in ws + [e % R for e in edge]:
            hs.hs_r1cs_mul_small(_limbs(w), c, out)
            assert _val(out) == c * w % R, (c, w)


def test_every_term_class_adds_what_python_adds(hs):
    """one term into a running sum, through the same classification and the same per-class arithmetic as the kernels"""
    rng = np.random.default_rng(8)
    coeffs = [0, 1, R - 1, 2, R - 2, 12345, (1 << 28) - 1, 1 << 28, R - (1 << 28) + 1, R - (1 << 28), R - 12345, (1 << 64) - 1]
    coeffs += [int.from_bytes(rng.bytes(40), "little") % R for _ in range(20)]
    want_cls = {0: 100, 1: 0, R - 1: 1, 2: 2, R - 2: 3, 12345: 2, (1 << 28) - 1: 2, 1 << 28: 4, R - (1 << 28) + 1: 3, R - (1 << 28): 4, R - 12345: 3}
    small = ctypes.c_uint32()
    out = (ctypes.c_uint64 * 4)()
    vals = [0, 1, R - 1, R - 2] + [int.from_bytes(rng.bytes(40), "little") % R for _ in range(12)]
    for c in coeffs:
        cls = hs.hs_r1cs_classify(_limbs(c), ctypes.byref(small))
        if c in want_cls:
            assert cls == want_cls[c], c
        for acc in vals[:6]:
            for w in vals:
                hs.hs_r1cs_term(_limbs(acc), _limbs(c), _limbs(w), out)
                assert _val(out) == (acc + c * w) % R, (acc, c, w)
    assert hs.hs_r1cs_classify(_limbs(R), ctypes.byref(small)) == 101        # not canonical
    assert hs.hs_r1cs_classify(_limbs(2**256 - 1), ctypes.byref(small)) == 101
