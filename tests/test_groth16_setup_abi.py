"""The Groth16 setup and the fixed-base multiplication at the C ABI, without a GPU: the new symbols exist and are bound, NULL
contexts and handles give a status and a message and leave the outputs alone, the ctypes mirrors of the two new structures have
the sizes the C compiler gives them, and the host-callable pieces of the feature - the signed byte digits of the fixed-base
kernel and the transposition of the constraint matrices - agree with Python integers (tests/setupsim: the library's own code
built for the CPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cityprover
import groth16_setup_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cp_fixed_base_mul_bls12381_g1_dev", "cp_fixed_base_mul_bls12381_g2_dev", "cp_groth16_setup_bls12381", "cp_groth16_key_destroy",
       "cp_groth16_key_pk", "cp_groth16_key_vk")
u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)


def test_new_symbols_are_exported_and_bound():
    lib = cityprover.load_library()
    for s in NEW:
        assert s in cityprover.ABI, s
        assert hasattr(lib, s), s
    assert lib.cp_abi_version() == 4
    for name in ("Groth16Trapdoor", "Groth16Vk", "Groth16Key"):
        assert hasattr(cityprover, name), name
    for cls in (cityprover.G1Points, cityprover.G2Points):
        assert hasattr(cls, "fixed_base")
    for m in ("setup", "pk", "vk", "free"):
        assert hasattr(cityprover.Groth16Key, m), m


def test_null_context_and_handles_give_a_status_and_a_message():
    lib = cityprover.load_library()
    assert lib.cp_fixed_base_mul_bls12381_g1_dev(None, None, None, 0, None, None) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_fixed_base_mul_bls12381_g2_dev(None, None, None, 0, None, None) != 0
    assert b"ctx is NULL" in lib.cp_last_error(None)
    desc, keep = cityprover.r1cs_desc(2, 1, np.array([[1, 0, 0, 0]], np.uint64),
                                      [(np.array([0, 1, 2], np.uint64), np.array([0, 0], np.uint32), np.array([0, 0], np.uint32))] * 3)
    td = cityprover.Groth16Trapdoor()
    assert not lib.cp_groth16_setup_bls12381(None, ctypes.byref(desc), 1, ctypes.byref(td))
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert not lib.cp_groth16_setup_bls12381(None, None, 1, None)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    # NULL key: a status, and the outputs stay as they were
    pk = cityprover.Groth16Pk()
    pk.n_wires, pk.log_domain = 77, 7
    assert lib.cp_groth16_key_pk(None, ctypes.byref(pk)) != 0
    assert b"NULL" in lib.cp_last_error(None)
    assert (pk.n_wires, pk.log_domain) == (77, 7)
    vk = cityprover.Groth16Vk()
    vk.n_public = 5
    xy, inf = np.full(12, 9, np.uint64), np.full(1, 9, np.uint8)
    assert lib.cp_groth16_key_vk(None, ctypes.byref(vk), xy.ctypes.data_as(u64p), inf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) != 0
    assert b"NULL" in lib.cp_last_error(None)
    assert vk.n_public == 5 and (xy == 9).all() and (inf == 9).all()
    lib.cp_groth16_key_destroy(None)      # a no-op


def test_ctypes_mirrors_have_the_sizes_the_c_compiler_gives(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cityprover.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(cp_groth16_trapdoor), sizeof(cp_groth16_vk), '
                   'offsetof(cp_groth16_vk, n_public), offsetof(cp_groth16_trapdoor, delta)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(cityprover.Groth16Trapdoor), ctypes.sizeof(cityprover.Groth16Vk), cityprover.Groth16Vk.n_public.offset,
                   cityprover.Groth16Trapdoor.delta.offset]


# ---- the host-callable code of the feature on the CPU (tests/setupsim) ------------------------------------------------------
@pytest.fixture(scope="module")
def ss():
    import simlibs
    lib = ctypes.CDLL(simlibs.build("setupsim"))
    lib.ss_recode.argtypes = [u64p, ctypes.POINTER(ctypes.c_int32)]
    lib.ss_transpose.argtypes = [u64p, u32p, u32p, ctypes.c_size_t, ctypes.c_size_t, u64p, u32p, u32p]
    return lib


def test_signed_digits_resum_to_the_scalar(ss):
    """k = sum_w d_w 2^(c w) with |d_w| <= 2^(c-1) for every edge scalar of the GPU test and for random ones; the top window
    holds the last carry alone"""
    W, c, half = ss.ss_windows(), ss.ss_window_bits(), ss.ss_half()
    assert W * c >= 257 and half == 1 << (c - 1)
    digits = (ctypes.c_int32 * W)()
    for k in GC.edge_scalars() + GC.random_scalars(500, 1):
        limbs = (ctypes.c_uint64 * 4)(*[(k >> (64 * i)) & (2**64 - 1) for i in range(4)])
        ss.ss_recode(limbs, digits)
        d = list(digits)
        assert all(-half <= x <= half for x in d), k
        assert sum(x << (c * w) for w, x in enumerate(d)) == k, k
        assert d[-1] in (0, 1), k
    # the carry boundary itself: a byte of 0x80 stays +128 (no carry), 0x81 becomes -127 and carries
    for byte, want in ((0x80, (128, 0)), (0x81, (-127, 1)), (0xff, (-1, 1))):
        limbs = (ctypes.c_uint64 * 4)(byte, 0, 0, 0)
        ss.ss_recode(limbs, digits)
        assert (digits[0], digits[1]) == want


def _csr(rows, n_cols):
    row_ptr, col, coeff = [0], [], []
    for row in rows:
        for c, k in row:
            col.append(c)
            coeff.append(k)
        row_ptr.append(len(col))
    return np.array(row_ptr, np.uint64), np.array(col, np.uint32), np.array(coeff, np.uint32)


def _transpose(ss, rows, n_cols):
    rp, col, coeff = _csr(rows, n_cols)
    nnz = len(col)
    out_rp, out_col, out_coeff = np.zeros(n_cols + 1, np.uint64), np.zeros(max(nnz, 1), np.uint32), np.zeros(max(nnz, 1), np.uint32)
    p32 = lambda a: a.ctypes.data_as(u32p) if a.size else None
    ss.ss_transpose(rp.ctypes.data_as(u64p), p32(col), p32(coeff), len(rows), n_cols, out_rp.ctypes.data_as(u64p), p32(out_col), p32(out_coeff))
    assert out_rp[0] == 0 and out_rp[-1] == nnz and (np.diff(out_rp.astype(np.int64)) >= 0).all()
    return [[(int(out_col[t]), int(out_coeff[t])) for t in range(int(out_rp[i]), int(out_rp[i + 1]))] for i in range(n_cols)]


def test_transposed_matrix_is_the_same_matrix(ss):
    """every term (row j, wire i, coefficient k) comes out once as (row i, column j, coefficient k), in the order of the rows:
    a wire named several times in one row, empty rows, empty columns, a column that every row names, and random matrices"""
    rows = [[(0, 5), (3, 1), (0, 6), (0, 5)],      # wire 0 three times, twice with the same coefficient
            [],                                     # an empty row
            [(4, 2), (0, 7)],
            [],
            [(0, 1), (4, 9), (4, 9)]]
    got = _transpose(ss, rows, 6)                   # wires 1, 2, 5 occur nowhere
    assert got == [[(0, 5), (0, 6), (0, 5), (2, 7), (4, 1)], [], [], [(0, 1)], [(2, 2), (4, 9), (4, 9)], []]
    assert _transpose(ss, [[], []], 3) == [[], [], []]
    rng = np.random.default_rng(5)
    for n_rows, n_cols in ((1, 1), (7, 3), (50, 200), (300, 40)):
        rows = [[(int(rng.integers(0, n_cols)), int(rng.integers(0, 1000))) for _ in range(int(rng.integers(0, 9)))] for _ in range(n_rows)]
        got = _transpose(ss, rows, n_cols)
        want = [[] for _ in range(n_cols)]
        for j, row in enumerate(rows):
            for c, k in row:
                want[c].append((j, k))
        assert got == want
