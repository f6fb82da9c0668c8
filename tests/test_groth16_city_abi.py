"""The batched entry points for stored Groth16 proofs at the C ABI, without a GPU: the header declares them, the built library
exports them, the ctypes table and the Rust block name them with as many arguments, and without a context both refuse
with a status and a message."""
import ctypes
import os
import re

import numpy as np

import cityprover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cp_groth16_proofs_unpack_city_bls12381", "cp_groth16_verify_city_bls12381")
u64p = ctypes.POINTER(ctypes.c_uint64)
u8p = ctypes.POINTER(ctypes.c_uint8)


def n_args(text, pattern):
    m = re.search(pattern + r"\(([^)]*)\)", text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_bindings_and_rust_agree():
    header = open(os.path.join(ROOT, "include", "cityprover.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    lib = cityprover.load_library()
    for s in NEW:
        assert s in cityprover.ABI, s
        assert hasattr(lib, s), s
        n = len(cityprover.ABI[s][1])
        assert n_args(header, r"\bint %s" % s) == n, s
        assert n_args(ffi, r"pub fn %s" % s) == n, s
    assert len(cityprover.ABI[NEW[0]][1]) == 5 and len(cityprover.ABI[NEW[1]][1]) == 7
    assert lib.cp_abi_version() == 4
    assert callable(cityprover.groth16_unpack_city_batch) and hasattr(cityprover.Groth16Verifier, "verify_city")


def test_without_a_context_both_refuse_with_a_message():
    lib = cityprover.load_library()
    blob = np.zeros(192, np.uint8)
    words, st = np.full(48, 9, np.uint64), np.full(1, 9, np.uint8)
    assert lib.cp_groth16_proofs_unpack_city_bls12381(None, blob.ctypes.data_as(u8p), 1, words.ctypes.data_as(u64p), st.ctypes.data_as(u8p)) == -1
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_groth16_proofs_unpack_city_bls12381(None, None, 0, None, None) == -1
    assert lib.cp_groth16_verify_city_bls12381(None, None, blob.ctypes.data_as(u8p), None, 1, 0, st.ctypes.data_as(u8p)) == -1
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_groth16_verify_city_bls12381(None, None, None, None, 0, 0, None) == -1
    assert (words == 9).all() and (st == 9).all()


def test_blob_arguments_of_the_python_layer():
    a = cityprover._city_blobs([bytes(192), bytearray(192)])
    assert a.shape == (2, 192) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    assert cityprover._city_blobs(np.zeros((3, 192), np.uint8)).shape == (3, 192)
    for bad in ([bytes(191)], np.zeros((2, 191), np.uint8)):
        try:
            cityprover._city_blobs(bad)
        except ValueError:
            continue
        raise AssertionError("a blob that is not 192 bytes was accepted")
