"""The pairing product and the Groth16 verifier at the C ABI, without a GPU: the header declares the new entry points, the built
library exports them, the ctypes table and the Rust block name them, NULL and zero arguments give a status and a message
without a context, and the committed table of constants is what its generator writes."""
import ctypes
import importlib.util
import os
import re

import numpy as np

import cityprover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cp_pairing_product_bls12381", "cp_groth16_verifier_create_bls12381", "cp_groth16_verifier_destroy", "cp_groth16_verify_bls12381")
u64p = ctypes.POINTER(ctypes.c_uint64)
u8p = ctypes.POINTER(ctypes.c_uint8)


def test_header_library_bindings_and_rust_name_the_entry_points():
    header = open(os.path.join(ROOT, "include", "cityprover.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "cityprover-sys", "src", "ffi.rs")).read()
    lib = cityprover.load_library()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in cityprover.ABI, s
        assert hasattr(lib, s), s
        assert "pub fn %s(" % s in ffi, s
    assert "#define CP_GT_WORDS 72" in header and "pub const CP_GT_WORDS: usize = 72;" in ffi
    assert "#define CP_PAIRING_TRUSTED 1u" in header and "pub const CP_PAIRING_TRUSTED: c_uint = 1;" in ffi
    assert "pub struct CpGroth16Verifier" in ffi
    assert (cityprover.GT_WORDS, cityprover.PAIRING_TRUSTED) == (72, 1)
    assert lib.cp_abi_version() == 4
    assert callable(cityprover.pairing_product)
    for m in ("create", "from_key", "verify", "close"):
        assert hasattr(cityprover.Groth16Verifier, m), m


def test_null_and_zero_arguments_give_a_status_without_a_context():
    lib = cityprover.load_library()
    g1, g2 = np.zeros(12, np.uint64), np.zeros(24, np.uint64)
    gt, flag = np.full(72, 9, np.uint64), np.full(1, 9, np.uint8)
    assert lib.cp_pairing_product_bls12381(None, g1.ctypes.data_as(u64p), None, g2.ctypes.data_as(u64p), None, 1, 1, 0, gt.ctypes.data_as(u64p),
                                           flag.ctypes.data_as(u8p), None) == -1
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_pairing_product_bls12381(None, None, None, None, None, 0, 0, 0, None, None, None) == -1
    assert (gt == 9).all() and (flag == 9).all()
    vk = cityprover.Groth16Vk()
    assert not lib.cp_groth16_verifier_create_bls12381(None, ctypes.byref(vk), g1.ctypes.data_as(u64p), None)
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert not lib.cp_groth16_verifier_create_bls12381(None, None, None, None)
    assert lib.cp_groth16_verify_bls12381(None, None, None, None, 0, 0, None) == -1
    assert b"ctx is NULL" in lib.cp_last_error(None)
    assert lib.cp_groth16_verify_bls12381(None, None, g1.ctypes.data_as(u64p), None, 1, 0, flag.ctypes.data_as(u8p)) == -1
    assert (flag == 9).all()
    lib.cp_groth16_verifier_destroy(None)      # a no-op


def test_committed_table_is_what_the_generator_writes(tmp_path, monkeypatch):
    csrc = os.path.join(ROOT, "city-rollup_amd", "csrc")
    spec = importlib.util.spec_from_file_location("gen_bls_tables_under_test", os.path.join(csrc, "gen_bls_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    written = {}

    class Sink:
        def __init__(self, path, mode):
            assert mode == "w"
            self.path = path

        def write(self, text):
            written[self.path] = text

    monkeypatch.setattr(gen, "open", Sink, raising=False)      # the generator writes through open(path, "w").write(text)
    gen.main()
    (path, text), = written.items()
    assert os.path.basename(path) == "bls12_381_tables.h"
    assert text == open(os.path.join(csrc, "bls12_381_tables.h")).read()
    for name in ("BLS_X_ABS", "BLS_FINAL_EXP_C", "BLS_FROB"):
        assert name in text
