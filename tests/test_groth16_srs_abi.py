"""The SRS setup, the contributions and the point transforms at the C ABI, without a GPU: the seven new symbols are declared,
exported and bound; NULL contexts, descriptors, keys and out-pointers give a status (or NULL) and a message, never a crash; and
the host-callable pieces of the kernels - the 256-bit scalar multiplication on operands in memory, in both its forms, and the
butterfly, twiddle and bit-reversal indexing of the transform - agree with the oracle and with Python integers
(tests/pointsim: the library's own code built for the CPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

import cityprover
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cp_groth16_srs_create_bls12381", "cp_groth16_srs_destroy", "cp_groth16_setup_srs_bls12381", "cp_groth16_key_contribute_bls12381",
       "cp_groth16_key_check_contribution_bls12381", "cp_point_ntt_bls12381_g1_dev", "cp_point_ntt_bls12381_g2_dev")
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
u64p = ctypes.POINTER(ctypes.c_uint64)


def test_the_seven_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "cityprover.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = cityprover.load_library()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", src), s
        assert s in cityprover.ABI, s
        assert hasattr(lib, s), s
    assert lib.cp_abi_version() == 4
    for name in ("Groth16Srs", "Groth16SrsDesc", "point_ntt_g1_dev", "point_ntt_g2_dev"):
        assert hasattr(cityprover, name), name
    for m in ("setup_srs", "contribute", "check_contribution"):
        assert hasattr(cityprover.Groth16Key, m), m
    assert "CP_GROTH16_SRS_CHECK_TORSION 1u" in src and cityprover.GROTH16_SRS_CHECK_TORSION == 1


def test_the_descriptor_mirror_has_the_layout_of_the_header():
    """int, four pointers, 24 words: the C compiler pads the int to the pointers' alignment, and so must ctypes"""
    d = cityprover.Groth16SrsDesc
    assert ctypes.sizeof(d) == 8 + 4 * 8 + 24 * 8
    assert (d.log_size.offset, d.tau_g1.offset, d.beta_tau_g1.offset, d.beta_g2.offset) == (0, 8, 32, 40)


def test_null_arguments_give_a_status_and_a_message():
    lib = cityprover.load_library()
    desc = cityprover.Groth16SrsDesc()
    assert not lib.cp_groth16_srs_create_bls12381(None, ctypes.byref(desc), 0)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert not lib.cp_groth16_srs_create_bls12381(None, None, 0)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    lib.cp_groth16_srs_destroy(None)             # returns
    lib.cp_groth16_srs_destroy(None)
    sysd, keep = cityprover.r1cs_desc(2, 1, np.array([[1, 0, 0, 0]], np.uint64),
                                      [(np.array([0, 1, 2], np.uint64), np.array([0, 0], np.uint32), np.array([0, 0], np.uint32))] * 3)
    assert not lib.cp_groth16_setup_srs_bls12381(None, ctypes.byref(sysd), 1, None)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert not lib.cp_groth16_setup_srs_bls12381(None, None, 1, None)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    d = np.array([2, 0, 0, 0], np.uint64)
    out = ctypes.c_void_p(77)
    assert lib.cp_groth16_key_contribute_bls12381(None, None, d.ctypes.data_as(u64p), ctypes.byref(out)) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert out.value == 77                       # refused before anything is written
    assert lib.cp_groth16_key_contribute_bls12381(None, None, None, None) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    verdict = ctypes.c_int(9)
    assert lib.cp_groth16_key_check_contribution_bls12381(None, None, None, None, ctypes.byref(verdict)) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert verdict.value == 9
    assert lib.cp_groth16_key_check_contribution_bls12381(None, None, None, None, None) != 0
    for fn in (lib.cp_point_ntt_bls12381_g1_dev, lib.cp_point_ntt_bls12381_g2_dev):
        assert fn(None, None, None, 3, 0) != 0
        assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_abi_version() == 4


# ---- the host-callable code of the kernels on the CPU (tests/pointsim) ------------------------------------------------------
@pytest.fixture(scope="module")
def ps():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("pointsim"))
    for f in (lib.ps_g1_mul, lib.ps_g2_mul):
        f.argtypes = [ctypes.c_int, u64p, ctypes.c_int, u64p, u64p]
    lib.ps_top_bit.argtypes = [u64p]
    lib.ps_butterfly.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, u64p]
    lib.ps_bit_reverse.argtypes = [ctypes.c_uint64, ctypes.c_int]
    lib.ps_bit_reverse.restype = ctypes.c_uint64
    return lib


def scalars():
    rng = np.random.default_rng(381)
    seeded = [int.from_bytes(rng.bytes(32), "little") for _ in range(3)] + [int.from_bytes(rng.bytes(4), "little")]
    return [0, 1, 2, R - 1, R, R + 1, 2**255, 2**256 - 1] + seeded


def limbs(v, n):
    return np.array([(int(v) >> (64 * j)) & (2**64 - 1) for j in range(n)], np.uint64)


def test_top_bit(ps):
    for k in scalars() + [1 << b for b in (0, 31, 32, 63, 64, 255)]:
        assert ps.ps_top_bit(limbs(k, 4).ctypes.data_as(u64p)) == k.bit_length() - 1, hex(k)


@pytest.mark.parametrize("form", [0, 1])
def test_g1_scalar_multiplication_on_the_host_build(ps, form):
    """k P for k = 0, 1, 2, r - 1, r, r + 1, 2^255, 2^256 - 1 and seeded k, P the generator and a multiple of it; through the
    Jacobian-operand form of the transform and the affine-operand form of the column sums"""
    G = O.bls_constants()[2]
    for P in (G, O.bls_g1_mul(G, 0xfeedbeef12345)):
        xy, _ = O.bls_point(P)
        for k in scalars():
            out = np.zeros(12, np.uint64)
            inf = ps.ps_g1_mul(form, xy.ctypes.data_as(u64p), 0, limbs(k, 4).ctypes.data_as(u64p), out.ctypes.data_as(u64p))
            got = None if inf else (O._int(out[:6]), O._int(out[6:]))
            assert got == O.bls_g1_mul(P, k), (form, hex(k))
            assert (got is None) == (k % R == 0)
    # an operand at infinity (the Jacobian form alone: an affine operand cannot be)
    xy, _ = O.bls_point(G)
    out = np.zeros(12, np.uint64)
    assert ps.ps_g1_mul(0, xy.ctypes.data_as(u64p), 1, limbs(12345, 4).ctypes.data_as(u64p), out.ctypes.data_as(u64p)) == 1


@pytest.mark.parametrize("form", [0, 1])
def test_g2_scalar_multiplication_on_the_host_build(ps, form):
    G = O.bls_g2_generator()
    xy, _ = O.bls_point2(G)
    for k in scalars():
        out = np.zeros(24, np.uint64)
        inf = ps.ps_g2_mul(form, xy.ctypes.data_as(u64p), 0, limbs(k, 4).ctypes.data_as(u64p), out.ctypes.data_as(u64p))
        got = None if inf else ((O._int(out[0:6]), O._int(out[6:12])), (O._int(out[12:18]), O._int(out[18:24])))
        assert got == O.bls_g2_mul(G, k), (form, hex(k))
    out = np.zeros(24, np.uint64)
    assert ps.ps_g2_mul(0, xy.ctypes.data_as(u64p), 1, limbs(7, 4).ctypes.data_as(u64p), out.ctypes.data_as(u64p)) == 1


@pytest.mark.parametrize("log_n", [1, 2, 4])
def test_the_indexing_of_the_transform_is_an_ntt(ps, log_n):
    """Python integers pushed through the kernels' own indexing - the bit-reversed load, then for every stage every butterfly's
    pair and twiddle exponent - give the F_r transform; at 2^4 every twiddle exponent is held against the root of its stage"""
    n = 1 << log_n
    omega = pow(7, (R - 1) // n, R)
    rng = np.random.default_rng(log_n)
    e = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    work = [0] * n
    for i in range(n):
        work[ps.ps_bit_reverse(i, log_n)] = e[i]
    assert sorted(ps.ps_bit_reverse(i, log_n) for i in range(n)) == list(range(n))
    for s in range(log_n):
        seen = set()
        stage_root = pow(7, (R - 1) >> (s + 1), R)          # omega of a transform of 2^(s+1) points
        for t in range(n // 2):
            b = np.zeros(3, np.uint64)
            ps.ps_butterfly(t, s, log_n, b.ctypes.data_as(u64p))
            lo, hi, tw = (int(v) for v in b)
            assert hi == lo + (1 << s) and hi < n and tw < n // 2
            assert pow(omega, tw, R) == pow(stage_root, lo % (1 << s), R), (s, t)
            seen |= {lo, hi}
            p, wq = work[lo], work[hi] * pow(omega, tw, R) % R
            work[lo], work[hi] = (p + wq) % R, (p - wq) % R
        assert seen == set(range(n))
    assert work == [sum(e[k] * pow(omega, j * k, R) for k in range(n)) % R for j in range(n)]
