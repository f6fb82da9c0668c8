"""cp_groth16_verify_all_bls12381 and its _city_ twin at the C ABI, without a GPU: the header declares them, the built library
exports them, the ctypes table and the Rust block name them with the header's argument list, and a NULL context gives a status
and a message and writes nothing."""
import ctypes
import os
import re

import numpy as np

import cityprover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cp_groth16_verify_all_bls12381", "cp_groth16_verify_all_city_bls12381")
u64p = ctypes.POINTER(ctypes.c_uint64)
u8p = ctypes.POINTER(ctypes.c_uint8)


def test_header_library_bindings_and_rust_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "cityprover.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    lib = cityprover.load_library()
    for s in NEW:
        decl = re.search(r"\bint %s\(([^;]*)\);" % s, header)
        assert decl, s
        params = [p.strip() for p in decl.group(1).replace("\n", " ").split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "v", "proofs_host", "public_inputs_host", "n_proofs", "weights_host", "flags",
                                                                "verdict_out_host", "path_out"], s
        assert s in cityprover.ABI and len(cityprover.ABI[s][1]) == len(params), s
        assert hasattr(lib, s), s
        assert "pub fn %s(" % s in ffi, s
    assert lib.cp_abi_version() == 4        # the change only adds to the ABI
    for m in ("verify_all", "verify_all_city"):
        assert hasattr(cityprover.Groth16Verifier, m), m


def test_a_null_context_gives_a_status_and_writes_nothing():
    lib = cityprover.load_library()
    proofs, blob, w = np.zeros(48, np.uint64), np.zeros(192, np.uint8), np.ones(2, np.uint64)
    out, path = np.full(1, 9, np.uint8), ctypes.c_int(9)
    for fn, pp in ((lib.cp_groth16_verify_all_bls12381, proofs.ctypes.data_as(u64p)), (lib.cp_groth16_verify_all_city_bls12381, blob.ctypes.data_as(u8p))):
        assert fn(None, None, pp, None, 1, w.ctypes.data_as(u64p), 0, out.ctypes.data_as(u8p), ctypes.byref(path)) == -1
        assert b"ctx is NULL" in lib.cp_last_error(None)
        assert fn(None, None, None, None, 0, None, 0, None, None) == -1
        assert out[0] == 9 and path.value == 9


def test_weights_of_the_python_wrapper():
    w = cityprover._weights128([1, (1 << 128) - 1, 5 << 64], 3)
    assert w.dtype == np.uint64 and w.tolist() == [[1, 0], [2**64 - 1, 2**64 - 1], [0, 5]]
    for bad in ([1, 2], [1, 2, 1 << 128], [1, 2, -1]):
        try:
            cityprover._weights128(bad, 3)
        except ValueError:
            continue
        raise AssertionError(bad)
