"""Phase 1 of the Groth16 ceremony at the C ABI, without a GPU: the four new symbols are declared, exported, bound and present in
the Rust block; NULL contexts, handles and out-pointers give a status (or NULL) and a message, never a crash, and no out-pointer
is written on refusal; and the host-callable per-lane code of g16srs::k_scale_each - which scalar entry k of an SRS array takes
under a contribution (t, a, b), and the multiplication that scalar steers - agrees with the oracle and with Python integers
(tests/srsphase1sim: the library's own code built for the CPU). The multiplication itself is g16srs::affine_mul_u256_at, which
tests/test_groth16_srs_abi.py already holds against the oracle on its own; here it is reached through the lane's code."""
import ctypes
import os
import re

import numpy as np
import pytest

import cityprover
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cp_groth16_srs_unit_bls12381", "cp_groth16_srs_contribute_bls12381", "cp_groth16_srs_points_bls12381", "cp_groth16_srs_check_bls12381")
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
u64p = ctypes.POINTER(ctypes.c_uint64)
TAU_G1, TAU_G2, ALPHA_TAU_G1, BETA_TAU_G1 = range(4)


def test_the_four_symbols_are_declared_exported_bound_and_in_the_rust_block():
    src = open(os.path.join(ROOT, "include", "cityprover.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    lib = cityprover.load_library()
    for s in NEW:
        assert re.search(r"\b" + s + r"\s*\(", src), s
        assert s in cityprover.ABI, s
        assert hasattr(lib, s), s
        assert re.search(r"\bfn " + s + r"\s*\(", ffi), s
    assert lib.cp_abi_version() == 4
    for m in ("unit", "contribute", "points", "check"):
        assert hasattr(cityprover.Groth16Srs, m), m


def test_null_arguments_give_a_status_and_a_message():
    lib = cityprover.load_library()
    assert not lib.cp_groth16_srs_unit_bls12381(None, 3)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    one = np.array([1, 0, 0, 0], np.uint64)
    p = one.ctypes.data_as(u64p)
    out = ctypes.c_void_p(77)
    assert lib.cp_groth16_srs_contribute_bls12381(None, None, p, p, p, ctypes.byref(out)) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert out.value == 77                       # refused before anything is written
    assert lib.cp_groth16_srs_contribute_bls12381(None, None, None, None, None, None) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    L = ctypes.c_int(9)
    beta = np.full(24, 5, np.uint64)
    assert lib.cp_groth16_srs_points_bls12381(None, None, ctypes.byref(L), None, None, None, None, beta.ctypes.data_as(u64p)) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert L.value == 9 and (beta == 5).all()
    assert lib.cp_groth16_srs_points_bls12381(None, None, None, None, None, None, None, None) != 0
    verdict = ctypes.c_int(9)
    assert lib.cp_groth16_srs_check_bls12381(None, None, None, ctypes.byref(verdict)) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert verdict.value == 9
    assert lib.cp_groth16_srs_check_bls12381(None, None, None, None) != 0
    assert lib.cp_abi_version() == 4


# ---- the per-lane code of k_scale_each on the CPU (tests/srsphase1sim) -----------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("srsphase1sim"))
    lib.sp_each_scalar.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, u64p, u64p, u64p, u64p]
    lib.sp_each_scalar.restype = None
    for f in (lib.sp_g1_lane, lib.sp_g2_lane):
        f.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, u64p, u64p, u64p, u64p, u64p, u64p]
    return lib


def limbs(v):
    return np.array([(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)], np.uint64)


def ptr(a):
    return a.ctypes.data_as(u64p)


def each_scalar(sim, array, k, count, t, a, b):
    out = np.zeros(4, np.uint64)
    sim.sp_each_scalar(array, k, count, ptr(limbs(t)), ptr(limbs(a)), ptr(limbs(b)), ptr(out))
    return sum(int(v) << (64 * j) for j, v in enumerate(out))


def seeded():
    rng = np.random.default_rng(20)
    return [int.from_bytes(rng.bytes(32), "little") % (R - 1) + 1 for _ in range(3)]


@pytest.mark.parametrize("log_size", [1, 2])
def test_the_scalar_of_every_entry_of_every_array(sim, log_size):
    """(array, k) -> exponent: t^k for the two tau arrays (tau_g1 runs to 2n - 2), a t^k and b t^k for the other two, out of one
    table of 2n - 1 powers; canonical (fully reduced) words"""
    n = 1 << log_size
    count = 2 * n - 1
    for t, a, b in (tuple(seeded()), (1, R - 1, 1), (R - 1, 1, R - 1), (2, 3, 5)):
        for array, entries, c in ((TAU_G1, count, 1), (TAU_G2, n, 1), (ALPHA_TAU_G1, n, a), (BETA_TAU_G1, n, b)):
            for k in range(entries):
                assert each_scalar(sim, array, k, count, t, a, b) == c * pow(t, k, R) % R, (array, k)


def multipliers():
    """1, 2, r - 1, seeded values, and values with long runs of zero and of one bits (the conditional addition of a lane is
    taken for none, or for all, of many steps in a row)"""
    runs = [(1 << 254) | 1, (1 << 254) - 1, ((1 << 100) - 1) << 77, (1 << 200) | (((1 << 64) - 1) << 3), R - (1 << 128)]
    return [1, 2, R - 1] + seeded() + [v % R for v in runs]


def test_g1_lane_multiplies_its_own_entry_by_its_own_scalar(sim):
    G = O.bls_constants()[2]
    P, other = O.bls_g1_mul(G, 0xfeedbeef12345), O.bls_g1_mul(G, 77)
    xy, oxy = O.bls_point(P)[0], O.bls_point(other)[0]
    one = limbs(1)
    for k in multipliers():
        # the scalar as t at index 1 of a tau array (t^1), and as the constant of the alpha and beta arrays at index 0 (c t^0)
        for array, index, t, a, b in ((TAU_G1, 1, k, 1, 1), (ALPHA_TAU_G1, 0, 3, k, 1), (BETA_TAU_G1, 0, 3, 1, k)):
            out = np.zeros(12, np.uint64)
            inf = sim.sp_g1_lane(array, index, 3, ptr(limbs(t)), ptr(limbs(a)), ptr(limbs(b)), ptr(xy), ptr(oxy), ptr(out))
            assert inf == 0
            assert (O._int(out[:6]), O._int(out[6:])) == O.bls_g1_mul(P, k), (array, hex(k))
    # a product of the table and the constant: a t^2 at index 2
    t, a, _ = seeded()
    out = np.zeros(12, np.uint64)
    assert sim.sp_g1_lane(ALPHA_TAU_G1, 2, 3, ptr(limbs(t)), ptr(limbs(a)), ptr(one), ptr(xy), ptr(oxy), ptr(out)) == 0
    assert (O._int(out[:6]), O._int(out[6:])) == O.bls_g1_mul(P, a * t * t % R)


def test_g2_lane_multiplies_its_own_entry_by_its_own_scalar(sim):
    G = O.bls_g2_generator()
    P, other = O.bls_g2_mul(G, 0xabcdef987), O.bls_g2_mul(G, 5)
    xy, oxy = O.bls_point2(P)[0], O.bls_point2(other)[0]
    for k in multipliers():
        out = np.zeros(24, np.uint64)
        assert sim.sp_g2_lane(TAU_G2, 1, 2, ptr(limbs(k)), ptr(limbs(1)), ptr(limbs(1)), ptr(xy), ptr(oxy), ptr(out)) == 0
        got = ((O._int(out[0:6]), O._int(out[6:12])), (O._int(out[12:18]), O._int(out[18:24])))
        assert got == O.bls_g2_mul(P, k), hex(k)
